#!/usr/bin/env python3
"""Time of the Voxel-RCNN tail (csrc/proposals.hip) at the shipped size, fused against composed (`DF3D_VR_TAIL_FUSED=0`):

  proposals   head maps -> RoIs: B = 8 frames, 200 x 176 x 2 anchors, NMS_PRE_MAXSIZE 2048 / NMS_POST_MAXSIZE 100, threshold 0.7.
              fused = VoxelRCNNHead.proposal_layer on the maps and anchor tables (ops.anchor_proposals: keys, top-k, decode of the
              selected anchors, NMS, compaction); composed = AnchorHeadSingle.generate_predicted_boxes (every anchor decoded
              in torch) + the reference's per-frame proposal loop on iou3d_nms.nms_gpu.
  final       100 RoIs per frame + RCNN outputs -> pred_dicts: SCORE_THRESH 0.3, NMS 0.1.  fused = ops.roi_decode_select + one
              read of the counts; composed = generate_predicted_boxes in torch + the reference's per-frame post_processing loop.

Random maps (logits 2 N(0, 1), residuals 0.05 N(0, 1): neighbouring anchors overlap above the threshold, NMS suppresses).
The same inputs for both sides, warmed up, alternating window by window in one process, device events around the windows;
median and range per side, torch.cuda.max_memory_allocated of one call of each side.  Kernel launches and traced memory
copies per call are counted from rocprofv3 traces of child processes of their own (`--count SIDE`: two runs with different
numbers of calls, the difference divided by the difference of the calls), where rocprofv3 is installed.  The memory-copy
trace of this platform lists no entry for the few-byte reads `.item()` / `.tolist()` make (a traced composed call, which
reads one count per frame, showed host-to-device rows only), so the device-to-host reads of a call are ALSO counted in the
process itself: torch's synchronisation debug mode reports every operation that makes the host wait for a device value.

    python tools/bench_vr_tail.py [--windows 7] [--calls 5] [--out FILE] [--no-trace]"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "3d-dual-fusion_amd")]

import numpy as np  # noqa: E402
import dualfusion  # noqa: E402,F401
import torch  # noqa: E402
from dualfusion import dense_heads, roi_heads, synth, vr_detector  # noqa: E402

GRID = np.array([1408, 1600, 40])
HEAD_CFG = {"NAME": "AnchorHeadSingle", "CLASS_AGNOSTIC": False, "USE_DIRECTION_CLASSIFIER": True, "DIR_OFFSET": 0.78539,
            "DIR_LIMIT_OFFSET": 0.0, "NUM_DIR_BINS": 2,
            "ANCHOR_GENERATOR_CONFIG": [{"class_name": "Car", "anchor_sizes": [[3.9, 1.6, 1.56]], "anchor_rotations": [0, 1.57],
                                         "anchor_bottom_heights": [-1.78], "align_center": False, "feature_map_stride": 8}],
            "TARGET_ASSIGNER_CONFIG": {"NAME": "AxisAlignedTargetAssigner", "BOX_CODER": "ResidualCoder"}}
NMS_TEST = {"NMS_TYPE": "nms_gpu", "MULTI_CLASSES_NMS": False, "NMS_PRE_MAXSIZE": 2048, "NMS_POST_MAXSIZE": 100, "NMS_THRESH": 0.7}
POST = {"SCORE_THRESH": 0.3, "OUTPUT_RAW_SCORE": False,
        "NMS_CONFIG": {"MULTI_CLASSES_NMS": False, "NMS_TYPE": "nms_gpu", "NMS_THRESH": 0.1, "NMS_PRE_MAXSIZE": 4096,
                       "NMS_POST_MAXSIZE": 500}}
SIDES = ("proposals_fused", "proposals_composed", "final_fused", "final_composed")


def pool_layer(radius):
    return {"MLPS": [[32, 32]], "QUERY_RANGES": [[4, 4, 4]], "POOL_RADIUS": [radius], "NSAMPLE": [16], "POOL_METHOD": "max_pool"}


ROI_CFG = {"CLASS_AGNOSTIC": True, "SHARED_FC": [256, 256], "CLS_FC": [256, 256], "REG_FC": [256, 256], "DP_RATIO": 0.3,
           "NMS_CONFIG": {"TEST": NMS_TEST},
           "ROI_GRID_POOL": {"FEATURES_SOURCE": ["x_conv2", "x_conv3", "x_conv4"], "GRID_SIZE": 6,
                             "POOL_LAYERS": {"x_conv2": pool_layer(0.4), "x_conv3": pool_layer(0.8), "x_conv4": pool_layer(1.6)}}}


def build(dev, batch):
    """-> {side: callable}, the shapes"""
    torch.manual_seed(0)
    head = dense_heads.AnchorHeadSingle(HEAD_CFG, 256, 1, ["Car"], GRID, synth.KITTI_RANGE).to(dev).eval()
    rh = roi_heads.VoxelRCNNHead({"x_conv2": 32, "x_conv3": 64, "x_conv4": 64}, ROI_CFG, synth.KITTI_RANGE, synth.KITTI_VOXEL).to(dev).eval()
    H, W, A = head.tables.H, head.tables.W, head.num_anchors_per_location
    gen = torch.Generator().manual_seed(1)
    rows = batch * H * W
    cls = (2 * torch.randn((rows, A), generator=gen)).to(dev)
    box = (0.05 * torch.randn((rows, A * 7), generator=gen)).to(dev)
    dirs = torch.randn((rows, A * 2), generator=gen).to(dev)
    tables = {"tables": head.tables, "H": H, "W": W, "num_class": 1, "dir_offset": 0.78539, "dir_limit_offset": 0.0}

    def proposals_fused():
        bd = {"batch_size": batch, "dense_cls_rows": cls, "dense_box_rows": box, "dense_dir_rows": dirs, "dense_anchor_tables": tables}
        return rh.proposal_layer(bd, NMS_TEST)

    def proposals_composed():
        view = lambda r: r.view(batch, H, W, -1)
        cls_preds, box_preds = head.generate_predicted_boxes(batch, view(cls), view(box), view(dirs))
        bd = {"batch_size": batch, "batch_cls_preds": cls_preds, "batch_box_preds": box_preds, "cls_preds_normalized": False}
        return rh.proposal_layer(bd, NMS_TEST)

    with torch.no_grad():
        first = proposals_fused()
    rois = first["rois"]
    n = rois.shape[1]
    rcnn_cls = (2 * torch.randn((batch * n, 1), generator=gen)).to(dev)
    rcnn_reg = (0.05 * torch.randn((batch * n, 7), generator=gen)).to(dev)

    def final_fused():
        os.environ["DF3D_VR_TAIL_FUSED"] = "1"
        bd = {"batch_size": batch, "rois": rois, "rcnn_cls": rcnn_cls, "rcnn_reg": rcnn_reg, "has_class_labels": False}
        vr_detector.final_selection(bd, POST)
        return vr_detector.post_processing(bd, POST)

    def final_composed():
        os.environ["DF3D_VR_TAIL_FUSED"] = "0"
        cls_preds, box_preds = rh.generate_predicted_boxes(batch, rois, rcnn_cls, rcnn_reg)
        bd = {"batch_size": batch, "rois": rois, "batch_cls_preds": cls_preds, "batch_box_preds": box_preds,
              "cls_preds_normalized": False, "has_class_labels": False}
        return vr_detector.post_processing(bd, POST)

    def no_grad(fn):
        def run():
            with torch.no_grad():
                return fn()
        return run
    sides = {"proposals_fused": no_grad(proposals_fused), "proposals_composed": no_grad(proposals_composed),
             "final_fused": no_grad(final_fused), "final_composed": no_grad(final_composed)}
    return sides, dict(batch=batch, H=H, W=W, anchors_per_frame=H * W * A, rois_per_frame=int(n))


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


def host_reads(fn):
    """device values the host waits for during one call (item, tolist, nonzero, boolean masks ...): the warnings of torch's
    synchronisation debug mode"""
    import warnings
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return sum("synchroniz" in str(w.message).lower() for w in caught)


def trace_rows(directory):
    """(kernel launches, device-to-host copies) in the rocprofv3 CSV traces under `directory`; None where no kernel trace is"""
    kernels = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    if not kernels:
        return None
    launches = sum(max(sum(1 for _ in open(p)) - 1, 0) for p in kernels)
    d2h = 0
    for p in glob.glob(os.path.join(directory, "**", "*memory_copy_trace.csv"), recursive=True):
        for row in csv.reader(open(p)):
            d2h += any("DEVICE_TO_HOST" in f.upper() or f.upper() == "DTOH" for f in row)
    return launches, d2h


def traced_counts(side, batch, few=2, many=12):
    """per call: (rows of a run with `many` calls - rows of a run with `few`) / (many - few)"""
    rows = []
    for calls in (few, many):
        with tempfile.TemporaryDirectory() as tmp:
            cmd = ["rocprofv3", "--kernel-trace", "--memory-copy-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "t", "--",
                   sys.executable, os.path.abspath(__file__), "--count", side, "--calls", str(calls), "--batch", str(batch)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            got = trace_rows(tmp) if r.returncode == 0 else None
            if got is None:
                return dict(error="rocprofv3 run failed (rc %d)" % r.returncode)
            rows.append(got)
    return dict(launches_per_call=(rows[1][0] - rows[0][0]) / (many - few),
                traced_d2h_copies_per_call=(rows[1][1] - rows[0][1]) / (many - few))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--count", choices=SIDES, default=None, help="run only this side --calls times (under rocprofv3)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    sides, shapes = build(dev, args.batch)
    if args.count:
        for _ in range(args.calls):
            sides[args.count]()
        torch.cuda.synchronize()
        return
    lines = []
    common = dict(device=torch.cuda.get_device_name(0), windows=args.windows, calls_per_window=args.calls, **shapes)
    a, b = sides["proposals_fused"](), sides["proposals_composed"]()
    same_rois = bool(torch.equal(a["roi_labels"], b["roi_labels"]) and torch.equal(a["roi_scores"], b["roi_scores"]))
    fa, fb = sides["final_fused"](), sides["final_composed"]()
    same_final = all(len(x["pred_scores"]) == len(y["pred_scores"]) for x, y in zip(fa, fb))
    for stage, same in (("proposals", same_rois), ("final", same_final)):
        pair = {k: sides[stage + "_" + k] for k in ("fused", "composed")}
        ms = alternate(pair, args.windows, args.calls)
        row = dict(what=stage, same_selection=same, **common)
        for k in pair:
            row[k + "_ms"] = stats(ms[k])
            row[k + "_peak_mib"] = peak_mib(pair[k])
            row[k + "_host_reads_per_call"] = host_reads(pair[k])
        row["speedup_median"] = round(row["composed_ms"]["median"] / row["fused_ms"]["median"], 2)
        row["every_fused_window_faster"] = bool(max(ms["fused"]) < min(ms["composed"]))
        if not args.no_trace:
            for k in pair:
                row[k + "_trace"] = traced_counts(stage + "_" + k, args.batch) if shutil.which("rocprofv3") else dict(error="no rocprofv3")
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
    os.environ.pop("DF3D_VR_TAIL_FUSED", None)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
