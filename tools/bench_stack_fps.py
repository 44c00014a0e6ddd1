#!/usr/bin/env python3
"""Time of furthest point sampling, the stacked kernel (csrc/pointops.hip: stack_fps_kernel, one workgroup per segment, all
segments in one launch) against the batch kernel (df3d_furthest_point_sample, one launch per frame):

  (a) one segment of 4 k / 12 k / 24 k / 25 k / 30 k / 32 k / 40 k points x 2048 picks: the batch kernel at B = 1, the
      stacked kernel on the same segment (once more with DF3D_STACK_FPS_LDS=0: the variant for 24 577 .. 32 768 rows that
      keeps the minima in registers instead of LDS), on 8 equal segments, and on 8 `synth.kitti_sweep` frames of unequal
      size -- microseconds per pick;
  (b) `VoxelSetAbstraction.forward` at the shipped PV-RCNN size (the scene of tools/bench_vsa.py) with DF3D_VSA_STACK_FPS on
      and off, at B = 2 and B = 8.

The method of tools/bench_vsa.py: device events around windows of repeated calls, all sides warmed up first and alternated
window by window, median [min .. max] over the windows.  Every row also says whether the sides gave the same indices /
keypoints.

    python tools/bench_stack_fps.py [--windows 7] [--calls 3] [--batches 2 8] [--out profiles/stack_fps_ab.txt]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "3d-dual-fusion_amd"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402
import dualfusion  # noqa: E402,F401
import torch  # noqa: E402
from dualfusion import ops, pfe, synth  # noqa: E402

import bench_vsa as bv  # noqa: E402  (the scene, the window timer, host_reads)

PICKS = 2048
SIZES = (4096, 12288, 24576, 25000, 30000, 32768, 40000)


def cloud(n, dev):
    rows, seed = [], 0
    while sum(len(r) for r in rows) < n:
        rows.append(synth.kitti_sweep(seed=100 + seed)[:, :3])
        seed += 1
    return torch.from_numpy(np.ascontiguousarray(np.concatenate(rows)[:n], np.float32)).to(dev)


def counts(c, dev):
    return torch.tensor(list(c), dtype=torch.int32, device=dev)


def lds_off(fn):
    os.environ["DF3D_STACK_FPS_LDS"] = "0"
    try:
        return fn()
    finally:
        del os.environ["DF3D_STACK_FPS_LDS"]


def kernel_rows(dev, args):
    lines = []
    sweeps = [torch.from_numpy(np.ascontiguousarray(synth.kitti_sweep(seed=b)[:, :3])).to(dev) for b in range(8)]
    uneven, uneven_cnt = torch.cat(sweeps).contiguous(), counts([len(s) for s in sweeps], dev)
    num8 = counts([PICKS] * 8, dev)
    for n in SIZES:
        one = cloud(n, dev)
        eight = one.repeat(8, 1).contiguous()
        cnt1, cnt8, num1 = counts([n], dev), counts([n] * 8, dev), counts([PICKS], dev)
        sides = {
            "batch_B1": lambda: ops.furthest_point_sample(one[None], PICKS),
            "stacked_1": lambda: ops.stack_furthest_point_sample(one, cnt1, num1, total=PICKS, mode="frames"),
            "stacked_1_lds_off": lambda: lds_off(lambda: ops.stack_furthest_point_sample(one, cnt1, num1, total=PICKS, mode="frames")),
            "stacked_8_equal": lambda: ops.stack_furthest_point_sample(eight, cnt8, num8, total=8 * PICKS, mode="frames"),
            "stacked_8_sweeps": lambda: ops.stack_furthest_point_sample(uneven, uneven_cnt, num8, total=8 * PICKS, mode="frames"),
        }
        a, b = sides["batch_B1"]()[0], sides["stacked_1"]()
        same_off = bool(torch.equal(b, sides["stacked_1_lds_off"]()))
        c = sides["stacked_8_equal"]().view(8, PICKS) - (torch.arange(8, device=dev) * n)[:, None].int()
        row = dict(what="one segment x %d picks" % PICKS, points=n, device=torch.cuda.get_device_name(0), windows=args.windows,
                   calls_per_window=args.calls, same_indices=bool(torch.equal(a, b) and bool((c == a[None]).all()) and same_off),
                   sweep_points=[len(s) for s in sweeps])
        ms = bv.alternate(sides, args.windows, args.calls)
        for k in sides:
            row[k + "_us_per_pick"] = bv.stats([v * 1000.0 / PICKS for v in ms[k]])
        row["stacked_1_no_slower_than_slowest_batch_window"] = bool(np.median(ms["stacked_1"]) <= max(ms["batch_B1"]))
        row["every_lds_window_faster_than_lds_off"] = bool(max(ms["stacked_1"]) < min(ms["stacked_1_lds_off"]))
        row["stacked_1_over_batch_median"] = round(float(np.median(ms["stacked_1"]) / np.median(ms["batch_B1"])), 3)
        print(json.dumps(row), flush=True)
        lines.append(json.dumps(row))
    return lines


def forward_rows(dev, args):
    lines = []
    torch.manual_seed(0)
    vsa = pfe.VoxelSetAbstraction(bv.PFE_CFG, synth.KITTI_VOXEL, synth.KITTI_RANGE, num_bev_features=256, num_rawpoint_features=4)
    bv.randomize_norms(vsa)
    vsa = vsa.to(dev).eval()

    def side(on, scene):
        def run():
            os.environ["DF3D_VSA_STACK_FPS"] = "1" if on else "0"
            with torch.no_grad():
                return vsa(dict(scene))
        return run
    for batch in args.batches:
        scene = bv.build(dev, batch)
        sides = {"stacked": side(True, scene), "per_frame": side(False, scene)}
        a, b = sides["stacked"]()["point_coords"], sides["per_frame"]()["point_coords"]
        row = dict(what="VoxelSetAbstraction.forward", batch=batch, points=int(scene["points"].shape[0]),
                   keypoints_per_frame=bv.PFE_CFG["NUM_KEYPOINTS"], device=torch.cuda.get_device_name(0), windows=args.windows,
                   calls_per_window=args.calls, same_keypoints=bool(torch.equal(a, b)))
        ms = bv.alternate(sides, args.windows, args.calls)
        for k in sides:
            row[k + "_ms"] = bv.stats(ms[k])
            row[k + "_host_reads"] = bv.host_reads(sides[k])
        row["speedup_median"] = round(row["per_frame_ms"]["median"] / row["stacked_ms"]["median"], 2)
        row["every_stacked_window_faster"] = bool(max(ms["stacked"]) < min(ms["per_frame"]))
        os.environ.pop("DF3D_VSA_STACK_FPS", None)
        print(json.dumps(row), flush=True)
        lines.append(json.dumps(row))
        del scene
        torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--batches", type=int, nargs="+", default=[2, 8])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    lines = kernel_rows(dev, args) + forward_rows(dev, args)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
