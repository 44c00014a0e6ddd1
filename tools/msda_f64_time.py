#!/usr/bin/env python3
"""Forward + backward time of the float64 MSDA path (csrc/msda_f64.hip) beside the float32 kernels on the same inputs, on the
device: device events around windows of repeated calls, both dtypes warmed up first and alternated window by window, median
and range over the windows.  The float64 path is a checking path (gradcheck, a device-side float64 reference); the number
says what such a check costs, not what a training step pays.

    python tools/msda_f64_time.py [--windows 7] [--seconds 0.4]

Shapes: "case6" = the device-reference case of tests/test_gpu_msda_f64.py (N 2, one 40 x 56 level, M 8, D 16, Lq 3000, P 4);
"fusion" = the fusion layer's own (N 6, one 150 x 267 level, M 8, D 16, Lq 8000, P 4)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "3d-dual-fusion_amd")]

import numpy as np  # noqa: E402
import dualfusion  # noqa: E402,F401
import torch  # noqa: E402
from dualfusion import ops  # noqa: E402

SHAPES = {"case6": (2, 8, 16, 3000, 4, (40, 56)), "fusion": (6, 8, 16, 8000, 4, (150, 267))}


def inputs(N, M, D, Lq, P, hw, dev):
    rs = np.random.RandomState(66)
    H, W = hw
    value = rs.standard_normal((N, H * W, M, D)).astype(np.float32)
    loc = np.empty((N, Lq, M, 1, P, 2), np.float32)
    for axis, size in ((0, W), (1, H)):
        loc[..., 0, :, axis] = (rs.randint(-2, size + 1, (N, Lq, M, P)) + rs.uniform(0.1, 0.9, (N, Lq, M, P)) + 0.5) / size
    aw = rs.uniform(0.1, 1, (N, Lq, M, 1, P)).astype(np.float32)
    aw /= aw.sum((-1, -2), keepdims=True)
    gout = rs.standard_normal((N, Lq, M * D)).astype(np.float32)
    shapes = torch.as_tensor([hw], dtype=torch.long, device=dev)
    return [torch.from_numpy(a).to(dev) for a in (value, loc, aw, gout)], shapes, shapes.new_zeros((1,))


def step(t, shapes, lstart):
    out = ops.ms_deform_attn_forward(t[0], shapes, lstart, t[1], t[2])
    return out, ops.ms_deform_attn_backward(t[0], shapes, lstart, t[1], t[2], t[3])


def window(t, shapes, lstart, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        step(t, shapes, lstart)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--seconds", type=float, default=0.4)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    for name, (N, M, D, Lq, P, hw) in SHAPES.items():
        t32, shapes, lstart = inputs(N, M, D, Lq, P, hw, dev)
        t64 = [x.double() for x in t32]
        sides = {"float32": t32, "float64": t64}
        calls = {}
        for k, t in sides.items():                                 # warm up, then size the window from a first estimate
            for _ in range(3):
                step(t, shapes, lstart)
            torch.cuda.synchronize()
            calls[k] = max(5, int(args.seconds * 1e3 / max(window(t, shapes, lstart, 5), 1e-3)))
        ms = {k: [] for k in sides}
        for _ in range(args.windows):
            for k, t in sides.items():
                ms[k].append(window(t, shapes, lstart, calls[k]))
        o32, g32 = step(t32, shapes, lstart)
        o64, g64 = step(t64, shapes, lstart)
        err = max(float((a.double() - b).abs().max()) / max(1.0, float(b.abs().max())) for a, b in zip((o32,) + tuple(g32), (o64,) + tuple(g64)))
        row = dict(shape=name, N=N, M=M, D=D, Lq=Lq, P=P, hw=list(hw), device=torch.cuda.get_device_name(0), windows=args.windows,
                   float32_vs_float64_max_err_of_scale=err)
        for k in sides:
            row[k + "_fwd_bwd_ms"] = dict(median=float(np.median(ms[k])), min=float(min(ms[k])), max=float(max(ms[k])), calls_per_window=calls[k])
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
