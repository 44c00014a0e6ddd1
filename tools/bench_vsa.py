#!/usr/bin/env python3
"""Time of the PV-RCNN point branch (csrc/stackpool.hip) at the shipped configuration, fused against composed:

  (a) `VoxelSetAbstraction.forward` (dualfusion/pfe.py): 2048 keypoints per frame by FPS, the bilinear BEV sample, and ten
      set-abstraction scales over the raw points and x_conv1..4; once more with the keypoints given, since the B sequential
      FPS calls (the same on both sides) are most of the forward;
  (b) `PVRCNNHead.roi_grid_pool` (dualfusion/roi_heads.py): 100 RoIs x 6^3 grid points per frame over the keypoints, two
      scales.

fused = one kernel per scale (ball query + gather + both MLP layers + max; eval mode); composed = DF3D_STACK_SA_FUSED=0: ball
query, stack grouping, linears over the [M * nsample, C] rows, BatchNorm, max in torch -- the reference's formulation.

Scene: B `synth.kitti_sweep` frames (points with intensity) on the KITTI grid [41, 1600, 1408]; the sparse levels are the
occupied cells strided by 1 / 2 / 4 / 8 with 16 / 32 / 64 / 64 channels of random features (a real backbone's levels are
somewhat denser: strided convolutions dilate them); a random [B, 256, 200, 176] BEV map; RoIs are car-sized boxes centred on
keypoints with random headings; random keypoint scores.  B = 2 is the config's batch per GPU, B = 8 the size of the other
A/B tools.

Device events around windows of repeated calls; both sides warmed up first and alternated window by window; median and range
over the windows, torch.cuda.max_memory_allocated of one call of each side, the kernel launches of one call (torch.profiler's
device events) and the values the host waits for (torch's synchronisation debug mode).

    python tools/bench_vsa.py [--windows 7] [--calls 3] [--batches 2 8] [--out profiles/vsa_ab.txt]"""
import argparse
import json
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "3d-dual-fusion_amd")]

import numpy as np  # noqa: E402
import dualfusion  # noqa: E402,F401
import torch  # noqa: E402
from dualfusion import ops, pfe, roi_heads, synth  # noqa: E402
from dualfusion.spconv import SparseConvTensor  # noqa: E402

GRID = [41, 1600, 1408]
LEVELS = (("x_conv1", 1, 16), ("x_conv2", 2, 32), ("x_conv3", 4, 64), ("x_conv4", 8, 64))


def sa(mlp, radii, nsample, factor=None):
    d = {"MLPS": [[mlp, mlp], [mlp, mlp]], "POOL_RADIUS": radii, "NSAMPLE": nsample}
    if factor:
        d["DOWNSAMPLE_FACTOR"] = factor
    return d


# PFE and ROI_HEAD.ROI_GRID_POOL of kitti_models/pv_rcnn_mm_mvx+actrv2_hybrid*.yaml
PFE_CFG = {"NAME": "VoxelSetAbstraction", "POINT_SOURCE": "raw_points", "NUM_KEYPOINTS": 2048, "NUM_OUTPUT_FEATURES": 128,
           "SAMPLE_METHOD": "FPS", "FEATURES_SOURCE": ["bev", "x_conv1", "x_conv2", "x_conv3", "x_conv4", "raw_points"],
           "SA_LAYER": {"raw_points": sa(16, [0.4, 0.8], [16, 16]), "x_conv1": sa(16, [0.4, 0.8], [16, 16], 1),
                        "x_conv2": sa(32, [0.8, 1.2], [16, 32], 2), "x_conv3": sa(64, [1.2, 2.4], [16, 32], 4),
                        "x_conv4": sa(64, [2.4, 4.8], [16, 32], 8)}}
HEAD_CFG = {"CLASS_AGNOSTIC": True, "SHARED_FC": [256, 256], "CLS_FC": [256, 256], "REG_FC": [256, 256], "DP_RATIO": 0.3,
            "ROI_GRID_POOL": {"GRID_SIZE": 6, "MLPS": [[64, 64], [64, 64]], "POOL_RADIUS": [0.8, 1.6], "NSAMPLE": [16, 16],
                              "POOL_METHOD": "max_pool"}}


def build(dev, batch):
    pts, frames = [], []
    for b in range(batch):
        p = torch.from_numpy(synth.kitti_sweep(seed=b)).to(dev)
        pts.append(torch.cat([torch.full_like(p[:, :1], b), p], 1))
        c = ops.dynamic_voxelize(p, synth.KITTI_VOXEL, synth.KITTI_RANGE)
        c = torch.unique(c[(c >= 0).all(1)].long(), dim=0)
        frames.append(torch.cat([torch.full_like(c[:, :1], b), c], 1))
    base = torch.cat(frames)
    gen = torch.Generator().manual_seed(0)
    tensors = {}
    for name, stride, ch in LEVELS:
        ind = torch.unique(torch.cat([base[:, :1], base[:, 1:] // stride], 1), dim=0).int().contiguous()
        feats = torch.randn((ind.shape[0], ch), generator=gen).to(dev)
        tensors[name] = SparseConvTensor(feats, ind, [-(-s // stride) for s in GRID], batch)
    bev = torch.randn((batch, 256, 200, 176), generator=gen).to(dev)
    return {"batch_size": batch, "points": torch.cat(pts).contiguous(), "spatial_features": bev, "spatial_features_stride": 8,
            "multi_scale_3d_features": tensors}


def randomize_norms(module):
    for m in module.modules():
        if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)


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


def launches(fn):
    """kernel launches of one call: the device-side kernel events torch.profiler records (None where it records none)"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
            and not any(w in e.name.lower() for w in ("memcpy", "memset", "copybuffer", "fillbuffer")))
    return n or None


def host_reads(fn):
    """device values the host waits for during one call: the warnings of torch's synchronisation debug mode"""
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return sum("synchroniz" in str(w.message).lower() for w in caught)


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


def side(fn, fused):
    def run():
        os.environ["DF3D_STACK_SA_FUSED"] = "1" if fused else "0"
        with torch.no_grad():
            return fn()
    return run


def compare(what, fn, key, common, args):
    sides = {"fused": side(fn, True), "composed": side(fn, False)}
    a, b = key(sides["fused"]()), key(sides["composed"]())
    row = dict(what=what, max_rel_diff=float((a - b).abs().max() / b.abs().max()), **common)
    ms = alternate(sides, args.windows, args.calls)
    for k in sides:
        row[k + "_ms"] = stats(ms[k])
        row[k + "_peak_mib"] = peak_mib(sides[k])
        row[k + "_launches"] = launches(sides[k])
        row[k + "_host_reads"] = host_reads(sides[k])
    row["speedup_median"] = round(row["composed_ms"]["median"] / row["fused_ms"]["median"], 2)
    row["every_fused_window_faster"] = bool(max(ms["fused"]) < min(ms["composed"]))
    os.environ.pop("DF3D_STACK_SA_FUSED", None)
    print(json.dumps(row), flush=True)
    return json.dumps(row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--batches", type=int, nargs="+", default=[2, 8])
    ap.add_argument("--rois", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    vsa = pfe.VoxelSetAbstraction(PFE_CFG, synth.KITTI_VOXEL, synth.KITTI_RANGE, num_bev_features=256, num_rawpoint_features=4)
    head = roi_heads.PVRCNNHead(128, HEAD_CFG, num_class=1)
    randomize_norms(vsa)
    randomize_norms(head)
    vsa, head = vsa.to(dev).eval(), head.to(dev).eval()
    lines = []
    for batch in args.batches:
        scene = build(dev, batch)
        common = dict(device=torch.cuda.get_device_name(0), batch=batch, keypoints_per_frame=PFE_CFG["NUM_KEYPOINTS"],
                      points=int(scene["points"].shape[0]), windows=args.windows, calls_per_window=args.calls,
                      voxels={n: int(t.indices.shape[0]) for n, t in scene["multi_scale_3d_features"].items()})
        lines.append(compare("VoxelSetAbstraction.forward", lambda: vsa(dict(scene)), lambda d: d["point_features"], common, args))
        with torch.no_grad():
            out = vsa(dict(scene))
        # the same without the keypoint sampling (B sequential FPS calls of 2048 picks, the same on both sides)
        keypoints = out["point_coords"]
        vsa.get_sampled_points = lambda batch_dict: keypoints
        lines.append(compare("VoxelSetAbstraction.forward, keypoints given", lambda: vsa(dict(scene)), lambda d: d["point_features"],
                             common, args))
        del vsa.get_sampled_points
        rs = np.random.RandomState(1)
        kp = out["point_coords"].view(batch, -1, 4)
        pick = torch.from_numpy(rs.randint(0, kp.shape[1], (batch, args.rois))).to(dev)
        rois = torch.zeros((batch, args.rois, 7), device=dev)
        rois[:, :, 0:3] = torch.gather(kp[:, :, 1:4], 1, pick[:, :, None].expand(-1, -1, 3))
        rois[:, :, 3:6] = torch.tensor([3.9, 1.6, 1.56], device=dev)
        rois[:, :, 6] = torch.from_numpy(rs.uniform(-np.pi, np.pi, (batch, args.rois)).astype(np.float32)).to(dev)
        bd = {"batch_size": batch, "rois": rois, "point_coords": out["point_coords"], "point_features": out["point_features"],
              "point_cls_scores": torch.from_numpy(rs.uniform(0, 1, kp.shape[0] * kp.shape[1]).astype(np.float32)).to(dev)}
        lines.append(compare("PVRCNNHead.roi_grid_pool", lambda: head.roi_grid_pool(bd), lambda t: t,
                             dict(common, rois_per_frame=args.rois, grid_points=batch * args.rois * 216), args))
        del scene, out, bd
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
