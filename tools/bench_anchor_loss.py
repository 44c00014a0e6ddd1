#!/usr/bin/env python3
"""Time of the Voxel-RCNN first-stage training tail (csrc/anchorloss.hip) at the shipped size, fused against composed
(`DF3D_ANCHOR_LOSS_FUSED=0`): target assignment + the three RPN losses + the gradient of the head maps.

  B = 8 frames, 200 x 176 x 2 car anchors (563 200 anchors), 20 seeded car boxes per frame in 24 ground-truth rows.
  fused     AnchorHeadSingle.assign_targets (ops.anchor_assign) + get_loss (ops.anchor_loss) + backward (one gradient launch);
  composed  the reference's formulation in torch: per-frame dense IoU matrices, dense regression targets, one-hot tensors and
            three dense loss maps under autograd.

Random maps (logits 2 N(0, 1), residuals 0.3 N(0, 1)).  The same inputs for both sides, warmed up, alternating window by
window in one process, device events around the windows; median and range per side, torch.cuda.max_memory_allocated of one
call of each side.  Kernel launches and traced memory copies per call come from rocprofv3 traces of child processes
(`--count SIDE`), and the device-to-host reads of a call from torch's synchronisation debug mode, both as
tools/bench_vr_tail.py counts them.

    python tools/bench_anchor_loss.py [--windows 7] [--calls 5] [--out FILE] [--no-trace]"""
import argparse
import json
import os
import shutil
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "3d-dual-fusion_amd"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402
import dualfusion  # noqa: E402,F401
import torch  # noqa: E402
import bench_vr_tail as bt  # noqa: E402  (window, alternate, stats, peak_mib, host_reads, trace_rows)
from dualfusion import dense_heads, synth  # noqa: E402

HEAD_CFG = {"NAME": "AnchorHeadSingle", "CLASS_AGNOSTIC": False, "USE_DIRECTION_CLASSIFIER": True, "DIR_OFFSET": 0.78539,
            "DIR_LIMIT_OFFSET": 0.0, "NUM_DIR_BINS": 2,
            "ANCHOR_GENERATOR_CONFIG": [{"class_name": "Car", "anchor_sizes": [[3.9, 1.6, 1.56]], "anchor_rotations": [0, 1.57],
                                         "anchor_bottom_heights": [-1.78], "align_center": False, "feature_map_stride": 8,
                                         "matched_threshold": 0.6, "unmatched_threshold": 0.45}],
            "TARGET_ASSIGNER_CONFIG": {"NAME": "AxisAlignedTargetAssigner", "POS_FRACTION": -1.0, "SAMPLE_SIZE": 512,
                                       "NORM_BY_NUM_EXAMPLES": False, "MATCH_HEIGHT": False, "BOX_CODER": "ResidualCoder"},
            "LOSS_CONFIG": {"LOSS_WEIGHTS": {"cls_weight": 1.0, "loc_weight": 2.0, "dir_weight": 0.2,
                                             "code_weights": [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]}}}
SIDES = ("fused", "composed")
GT_PER_FRAME, GT_ROWS = 20, 24


def ground_truth(batch):
    rs = np.random.RandomState(7)
    rng = synth.KITTI_RANGE
    gt = np.zeros((batch, GT_ROWS, 8), np.float32)
    for b in range(batch):
        size = np.asarray([3.9, 1.6, 1.56]) * rs.uniform(0.8, 1.25, (GT_PER_FRAME, 3))
        gt[b, :GT_PER_FRAME, 0] = rs.uniform(rng[0], rng[3], GT_PER_FRAME)
        gt[b, :GT_PER_FRAME, 1] = rs.uniform(rng[1], rng[4], GT_PER_FRAME)
        gt[b, :GT_PER_FRAME, 2] = -1.0
        gt[b, :GT_PER_FRAME, 3:6] = size
        gt[b, :GT_PER_FRAME, 6] = rs.uniform(-np.pi, np.pi, GT_PER_FRAME)
        gt[b, :GT_PER_FRAME, 7] = 1
    return gt


def build(dev, batch):
    """-> {side: callable -> (labels, losses [3], gradient of the rows)}, the shapes"""
    torch.manual_seed(0)
    head = dense_heads.AnchorHeadSingle(HEAD_CFG, 256, 1, ["Car"], bt.GRID, synth.KITTI_RANGE).to(dev).train()
    H, W, A = head.tables.H, head.tables.W, head.num_anchors_per_location
    gen = torch.Generator().manual_seed(1)
    n = batch * H * W
    rows = torch.cat([2 * torch.randn((n, A), generator=gen), 0.3 * torch.randn((n, A * 7), generator=gen),
                      torch.randn((n, A * 2), generator=gen)], dim=1).to(dev).requires_grad_(True)
    gt = torch.from_numpy(ground_truth(batch)).to(dev)
    head.tables.on(dev)

    def step(mode):
        def run():
            os.environ["DF3D_ANCHOR_LOSS_FUSED"] = mode
            rows.grad = None
            ret = {"rows": rows, "cls_preds": rows[:, :A].view(batch, H, W, A), "box_preds": rows[:, A:A * 8].view(batch, H, W, A * 7),
                   "dir_cls_preds": rows[:, A * 8:].view(batch, H, W, A * 2), "gt_boxes": gt}
            ret.update(head.assign_targets(gt))
            head.forward_ret_dict = ret
            loss, tb = head.get_loss()
            loss.backward()
            return ret["box_cls_labels"], torch.stack([tb["rpn_loss_cls"], tb["rpn_loss_loc"], tb["rpn_loss_dir"]]), rows.grad
        return run
    return {"fused": step("1"), "composed": step("0")}, dict(batch=batch, H=H, W=W, anchors=batch * H * W * A, gt_per_frame=GT_PER_FRAME,
                                                             gt_rows=GT_ROWS)


def traced_counts(side, batch, few=2, many=12):
    """per call: (rows of a run with `many` calls - rows of a run with `few`) / (many - few)"""
    import subprocess
    import tempfile
    rows = []
    for calls in (few, many):
        with tempfile.TemporaryDirectory() as tmp:
            cmd = ["rocprofv3", "--kernel-trace", "--memory-copy-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "t", "--",
                   sys.executable, os.path.abspath(__file__), "--count", side, "--calls", str(calls), "--batch", str(batch)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            got = bt.trace_rows(tmp) if r.returncode == 0 else None
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
    la, lossa, ga = sides["fused"]()
    la, lossa, ga = la.clone(), lossa.clone(), ga.clone()
    lb, lossb, gb = sides["composed"]()
    row = dict(what="assign + loss + grad", device=torch.cuda.get_device_name(0), windows=args.windows, calls_per_window=args.calls,
               same_labels=bool(torch.equal(la, lb)), positives=int((la > 0).sum()), ignored=int((la < 0).sum()),
               losses_fused=[round(float(v), 6) for v in lossa], losses_composed=[round(float(v), 6) for v in lossb],
               max_grad_difference=float((ga - gb).abs().max()), max_grad=float(gb.abs().max()), **shapes)
    ms = bt.alternate(sides, args.windows, args.calls)
    for k in SIDES:
        row[k + "_ms"] = bt.stats(ms[k])
        row[k + "_windows_ms"] = [round(v, 3) for v in ms[k]]
        row[k + "_peak_mib"] = bt.peak_mib(sides[k])
        row[k + "_host_reads_per_call"] = bt.host_reads(sides[k])
    row["speedup_median"] = round(row["composed_ms"]["median"] / row["fused_ms"]["median"], 2)
    row["every_fused_window_faster"] = bool(max(ms["fused"]) < min(ms["composed"]))
    if not args.no_trace:
        for k in SIDES:
            row[k + "_trace"] = traced_counts(k, args.batch) if shutil.which("rocprofv3") else dict(error="no rocprofv3")
    line = json.dumps(row)
    print(line, flush=True)
    os.environ.pop("DF3D_ANCHOR_LOSS_FUSED", None)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
