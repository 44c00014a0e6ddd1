#!/usr/bin/env python3
"""Time of the Voxel-RCNN RoI grid pooling (csrc/roipool.hip) at the shipped configuration:

  (a) the fused path: one kernel per level (query + gather + position term + ReLU + max), eval mode;
  (b) the composed path on the new ops (voxel query -> stack grouping -> Conv2d / BatchNorm2d / ReLU / max_pool in torch):
      the reference's formulation, `DF3D_ROI_POOL_FUSED=0`;
  (c) the voxel query alone through the occupancy directory against the reference's dense [B, Z, Y, X] tensor, each side
      INCLUDING the construction of its look-up structure (the reference rebuilds the dense tensor for every level of
      every step).

Levels: B = 8 `synth.kitti_sweep` frames on the KITTI grid [41, 1600, 1408], strided to x_conv2 / 3 / 4 (strides 2 / 4 / 8,
32 / 64 / 64 channels, random features; the occupancy of a real backbone is somewhat denser: strided convolutions dilate
it).  RoIs: 100 car-sized boxes per frame centred on occupied x_conv4 cells, random headings.  GRID_SIZE 6 and the
POOL_LAYERS of voxel_rcnn_car_mm_mvx+actrv2_hybrid_ifat.yaml: M = 8 * 100 * 216 = 172 800 grid points per level.

Device events around windows of repeated calls; all sides warmed up first and alternated window by window; median and
range over the windows, and torch.cuda.max_memory_allocated of one call of each side.

    python tools/bench_roi_pool.py [--windows 7] [--calls 5] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "3d-dual-fusion_amd")]

import numpy as np  # noqa: E402
import dualfusion  # noqa: E402,F401
import torch  # noqa: E402
from dualfusion import ops, roi_heads, synth  # noqa: E402
from dualfusion.spconv import SparseConvTensor  # noqa: E402

GRID = [41, 1600, 1408]
LEVELS = (("x_conv2", 2, 32), ("x_conv3", 4, 64), ("x_conv4", 8, 64))


def pool_layer(radius):
    return {"MLPS": [[32, 32]], "QUERY_RANGES": [[4, 4, 4]], "POOL_RADIUS": [radius], "NSAMPLE": [16], "POOL_METHOD": "max_pool"}


HEAD_CFG = {"CLASS_AGNOSTIC": True, "SHARED_FC": [256, 256], "CLS_FC": [256, 256], "REG_FC": [256, 256], "DP_RATIO": 0.3,
            "ROI_GRID_POOL": {"FEATURES_SOURCE": [n for n, _, _ in LEVELS], "GRID_SIZE": 6,
                              "POOL_LAYERS": {"x_conv2": pool_layer(0.4), "x_conv3": pool_layer(0.8), "x_conv4": pool_layer(1.6)}}}


def build(dev, batch, rois_per_frame):
    frames = []
    for b in range(batch):
        pts = torch.from_numpy(synth.kitti_sweep(seed=b)).to(dev)
        c = ops.dynamic_voxelize(pts, synth.KITTI_VOXEL, synth.KITTI_RANGE)
        c = torch.unique(c[(c >= 0).all(1)].long(), dim=0)
        frames.append(torch.cat([torch.full_like(c[:, :1], b), c], 1))
    base = torch.cat(frames)
    gen = torch.Generator().manual_seed(0)
    tensors = {}
    for name, stride, ch in LEVELS:
        ind = torch.unique(torch.cat([base[:, :1], base[:, 1:] // stride], 1), dim=0).int().contiguous()
        shape = [-(-s // stride) for s in GRID]
        feats = torch.randn((ind.shape[0], ch), generator=gen).to(dev)
        tensors[name] = SparseConvTensor(feats, ind, shape, batch)
    # RoIs on occupied x_conv4 cells
    ind4 = tensors["x_conv4"].indices
    xyz4 = roi_heads.get_voxel_centers(ind4[:, 1:4], 8, synth.KITTI_VOXEL, synth.KITTI_RANGE)
    rs = np.random.RandomState(1)
    rois = torch.zeros((batch, rois_per_frame, 7), device=dev)
    for b in range(batch):
        rows = (ind4[:, 0] == b).nonzero().squeeze(1)
        pick = rows[torch.from_numpy(rs.choice(len(rows), rois_per_frame, replace=len(rows) < rois_per_frame)).to(dev)]
        rois[b, :, 0:3] = xyz4[pick]
        rois[b, :, 3:6] = torch.tensor([3.9, 1.6, 1.56], device=dev)
        rois[b, :, 6] = torch.from_numpy(rs.uniform(-np.pi, np.pi, rois_per_frame).astype(np.float32)).to(dev)
    return tensors, rois


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls                 # ms per call


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 1)


def alternate(sides, windows, calls):
    for fn in sides.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in sides}
    for _ in range(windows):
        for k, fn in sides.items():
            ms[k].append(window(fn, calls))
    return ms


def stats(v):
    return dict(median=round(float(np.median(v)), 3), min=round(min(v), 3), max=round(max(v), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rois", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    tensors, rois = build(dev, args.batch, args.rois)
    torch.manual_seed(0)
    head = roi_heads.VoxelRCNNHead({n: c for n, _, c in LEVELS}, HEAD_CFG, synth.KITTI_RANGE, synth.KITTI_VOXEL).to(dev).eval()
    batch_dict = {"batch_size": args.batch, "rois": rois, "multi_scale_3d_features": tensors,
                  "multi_scale_3d_strides": {n: s for n, s, _ in LEVELS}}
    for t in tensors.values():
        t.directory()                                   # as after the backbone: every level carries its directory

    def pool(fused):
        def run():
            os.environ["DF3D_ROI_POOL_FUSED"] = "1" if fused else "0"
            with torch.no_grad():
                return head.roi_grid_pool(batch_dict)
        return run

    lines = []
    common = dict(device=torch.cuda.get_device_name(0), batch=args.batch, rois_per_frame=args.rois,
                  grid_points=args.batch * args.rois * 216, windows=args.windows, calls_per_window=args.calls,
                  voxels={n: int(t.indices.shape[0]) for n, t in tensors.items()})
    sides = {"fused": pool(True), "composed": pool(False)}
    a, b = sides["fused"](), sides["composed"]()
    diff = float((a - b).abs().max() / b.abs().max())
    ms = alternate(sides, args.windows, args.calls)
    row = dict(what="roi_grid_pool, three levels", max_rel_diff=diff, **common)
    for k in sides:
        row[k + "_ms"] = stats(ms[k])
        row[k + "_peak_mib"] = peak_mib(sides[k])
    row["speedup_median"] = round(row["composed_ms"]["median"] / row["fused_ms"]["median"], 2)
    row["every_fused_window_faster"] = bool(max(ms["fused"]) < min(ms["composed"]))
    os.environ.pop("DF3D_ROI_POOL_FUSED", None)
    lines.append(json.dumps(row))
    print(lines[-1], flush=True)

    # (c) the query alone, each side building its look-up structure
    g = 6
    grid_xyz = head.get_global_grid_points_of_roi(rois, g)[0].view(-1, 3).contiguous()
    frame = torch.arange(args.batch, device=dev).repeat_interleave(args.rois * g ** 3)
    for name, stride, _ in LEVELS:
        t = tensors[name]
        ind = t.indices
        xyz = roi_heads.get_voxel_centers(ind[:, 1:4], stride, synth.KITTI_VOXEL, synth.KITTI_RANGE).contiguous()
        cz = [torch.div(torch.div(grid_xyz[:, a] - synth.KITTI_RANGE[a], synth.KITTI_VOXEL[a], rounding_mode="floor"), stride,
                        rounding_mode="floor") for a in (2, 1, 0)]
        coords = torch.stack([frame.float()] + cz, 1).int().contiguous()
        layer = head.roi_grid_pool_layers[[n for n, _, _ in LEVELS].index(name)].groupers[0]
        q = (layer.max_range, layer.radius, layer.nsample, xyz, grid_xyz, coords)
        long_ind = ind.long()
        rows = torch.arange(ind.shape[0], dtype=torch.int32, device=dev)

        def with_directory():
            return ops.voxel_query(*q, ops.grid_build(ind, args.batch, t.spatial_shape))

        def with_dense():                               # generate_voxel2pinds (VR/pcdet/utils/common_utils.py) + the query
            table = torch.full([args.batch] + t.spatial_shape, -1, dtype=torch.int32, device=dev)
            table[long_ind[:, 0], long_ind[:, 1], long_ind[:, 2], long_ind[:, 3]] = rows
            return ops.voxel_query(*q, table)

        sides = {"directory": with_directory, "dense": with_dense}
        same = bool(torch.equal(with_directory(), with_dense()))
        ms = alternate(sides, args.windows, args.calls)
        row = dict(what="voxel query + look-up structure", level=name, shape=t.spatial_shape, same_indices=same, **common)
        for k in sides:
            row[k + "_ms"] = stats(ms[k])
            row[k + "_peak_mib"] = peak_mib(sides[k])
        row["speedup_median"] = round(row["dense_ms"]["median"] / row["directory_ms"]["median"], 2)
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
