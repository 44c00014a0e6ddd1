#!/usr/bin/env python3
"""Time of the native dynamic scatter (csrc/dynscatter.hip: plan + reduce, and its backward) beside what a user can write in
torch on the same device: forward = `torch.unique(dim=0, return_inverse=True)` over the valid rows + `index_add` (mean) or
`scatter_reduce(amax)` (max), backward = autograd's indexing.  Both sides take the same (feats [N, C], coors [N, ndim]) and
include everything from the coordinates on (the native plan is rebuilt in every call, as the composition sorts in every
call).  Device events around windows of repeated calls, both sides warmed up first and alternated window by window; median
and range over the windows.

    python tools/bench_dynscatter.py [--windows 7] [--seconds 0.25] [--out FILE]

Shapes: "nusc" = one synthetic nuScenes sweep of dualfusion.synth (about 52 k points) on the 0.075 m grid, the five point
features; "nusc6" = six sweeps (about 3.1e5 points); "kitti64" = a KITTI-shaped frame on the 0.05 m grid with 64-channel rows,
the inner width of DynamicVFE.  One JSON line per (shape, reduce, pass)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "3d-dual-fusion_amd")]

import numpy as np  # noqa: E402
import dualfusion  # noqa: E402,F401
import torch  # noqa: E402
from dualfusion import ops, synth  # noqa: E402


def shapes(dev):
    out = {}
    for name, pts, voxel, rng, width in (
            ("nusc", synth.nusc_sweep(seed=0), synth.NUSC_VOXEL, synth.NUSC_RANGE, None),
            ("nusc6", synth.nusc_sweep(seed=0, sweeps=6), synth.NUSC_VOXEL, synth.NUSC_RANGE, None),
            ("kitti64", synth.kitti_sweep(seed=0), synth.KITTI_VOXEL, synth.KITTI_RANGE, 64)):
        p = torch.from_numpy(pts).to(dev)
        coors = ops.dynamic_voxelize(p, voxel, rng)
        if width is None:
            feats = p.contiguous()
        else:
            feats = torch.from_numpy(np.random.RandomState(1).standard_normal((len(pts), width)).astype(np.float32)).to(dev)
        out[name] = (feats, coors)
    return out


def native(feats, coors, reduce, grad):
    out, _ = ops.dynamic_scatter(feats, coors, reduce)
    if grad is not None:
        feats.grad = None
        out.backward(grad)
    return out


def composition(feats, coors, reduce, grad):
    idx = (coors >= 0).all(1).nonzero().squeeze(1)
    uniq, inv = torch.unique(coors[idx], dim=0, return_inverse=True)
    rows = feats[idx]
    M, C = uniq.shape[0], feats.shape[1]
    if reduce == "mean":
        out = torch.zeros((M, C), dtype=feats.dtype, device=feats.device).index_add(0, inv, rows)
        cnt = torch.zeros((M,), dtype=feats.dtype, device=feats.device).index_add(0, inv, torch.ones_like(rows[:, 0]))
        out = out / cnt[:, None]
    else:
        out = torch.full((M, C), float("-inf"), dtype=feats.dtype, device=feats.device).scatter_reduce(
            0, inv[:, None].expand(-1, C), rows, "amax")
    if grad is not None:
        feats.grad = None
        out.backward(grad)
    return out


def window(fn, args, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn(*args)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls          # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--seconds", type=float, default=0.25)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    lines = []
    for name, (feats, coors) in shapes(dev).items():
        for reduce in ("mean", "max"):
            for with_backward in (False, True):
                x = feats.clone().requires_grad_(with_backward)
                ref_out = native(x, coors, reduce, None)
                grad = torch.randn_like(ref_out) if with_backward else None
                sides = {"native": native, "composition": composition}
                call_args = (x, coors, reduce, grad)
                calls = {}
                for k, fn in sides.items():                          # warm up, then size the window from a first estimate
                    for _ in range(3):
                        fn(*call_args)
                    torch.cuda.synchronize()
                    calls[k] = max(5, int(args.seconds * 1e6 / max(window(fn, call_args, 5), 1.0)))
                us = {k: [] for k in sides}
                for _ in range(args.windows):
                    for k, fn in sides.items():
                        us[k].append(window(fn, call_args, calls[k]))
                diff = float((native(x, coors, reduce, None) - composition(x, coors, reduce, None)).abs().max())
                row = dict(shape=name, points=int(feats.shape[0]), channels=int(feats.shape[1]), voxels=int(ref_out.shape[0]),
                           reduce=reduce, what="forward+backward" if with_backward else "forward",
                           device=torch.cuda.get_device_name(0), windows=args.windows, max_abs_diff=diff)
                for k in sides:
                    row[k + "_us"] = dict(median=round(float(np.median(us[k])), 1), min=round(min(us[k]), 1),
                                          max=round(max(us[k]), 1), calls_per_window=calls[k])
                row["speedup"] = round(row["composition_us"]["median"] / row["native_us"]["median"], 2)
                lines.append(json.dumps(row))
                print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
