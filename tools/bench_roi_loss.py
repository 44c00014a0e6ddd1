#!/usr/bin/env python3
"""Time of the Voxel-RCNN second-stage training tail (csrc/roiloss.hip) at the shipped size, fused against composed
(`DF3D_ROI_LOSS_FUSED=0`): proposal targets + the three RCNN losses + the gradient of rcnn_cls and rcnn_reg.

  B = 8 frames, 512 RoIs per frame -> 128 sampled (the shipped TARGET_CONFIG), 20 seeded boxes of three classes per frame in
  24 ground-truth rows; the RoIs are the boxes under small, medium and large perturbations.
  fused     ProposalTargetLayer.forward (ops.roi_targets) + get_loss (ops.rcnn_loss) + backward (one gradient launch);
  composed  the reference's formulation in torch: a per-frame loop, nonzero() compactions, counts read back, boolean-mask
            gathers and the corner loss under autograd (roi_heads.composed_roi_targets / composed_rcnn_losses).

The same inputs and the same draws for both sides, warmed up, alternating window by window in one process, device events
around the windows; median and range per side, torch.cuda.max_memory_allocated of one call of each side.  Kernel launches
and traced memory copies per call come from rocprofv3 traces of child processes (`--count SIDE`), and the device-to-host
reads of a call from torch's synchronisation debug mode, both as tools/bench_vr_tail.py counts them.

    python tools/bench_roi_loss.py [--windows 7] [--calls 5] [--out FILE] [--no-trace]"""
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
import bench_vr_tail as bt  # noqa: E402  (alternate, stats, peak_mib, host_reads, trace_rows)
from dualfusion import ops, roi_heads  # noqa: E402

TARGET_CFG = {"ROI_PER_IMAGE": 128, "FG_RATIO": 0.5, "SAMPLE_ROI_BY_EACH_CLASS": True, "CLS_SCORE_TYPE": "roi_iou", "CLS_FG_THRESH": 0.75,
              "CLS_BG_THRESH": 0.25, "CLS_BG_THRESH_LO": 0.1, "HARD_BG_RATIO": 0.8, "REG_FG_THRESH": 0.55}
SIDES = ("fused", "composed")
ROIS, GT_PER_FRAME, GT_ROWS = 512, 20, 24
SIZES = np.array([[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]])


def inputs(batch):
    rs = np.random.RandomState(7)
    gt = np.zeros((batch, GT_ROWS, 8), np.float32)
    cls = rs.randint(1, 4, (batch, GT_PER_FRAME))
    gt[:, :GT_PER_FRAME, 0], gt[:, :GT_PER_FRAME, 1] = rs.uniform(2, 68, cls.shape), rs.uniform(-38, 38, cls.shape)
    gt[:, :GT_PER_FRAME, 2] = -1.0
    gt[:, :GT_PER_FRAME, 3:6] = SIZES[cls - 1] * rs.uniform(0.8, 1.25, cls.shape + (3,))
    gt[:, :GT_PER_FRAME, 6], gt[:, :GT_PER_FRAME, 7] = rs.uniform(-np.pi, np.pi, cls.shape), cls
    src = gt[np.arange(batch)[:, None], rs.randint(0, GT_PER_FRAME, (batch, ROIS))]
    scale = rs.choice([0.03, 0.12, 0.3, 3.0], (batch, ROIS, 1))
    rois = src[..., :7].copy()
    rois[..., 0:3] += rs.normal(0, 1, (batch, ROIS, 3)) * scale * src[..., 3:6]
    rois[..., 3:6] *= np.exp(rs.normal(0, 0.1, (batch, ROIS, 3)))
    rois[..., 6] += rs.normal(0, 0.2, (batch, ROIS)) + np.pi * (rs.uniform(0, 1, (batch, ROIS)) < 0.3)
    return (rois.astype(np.float32), rs.normal(0, 2, (batch, ROIS)).astype(np.float32), src[..., 7].astype(np.int64), gt,
            rs.uniform(0, 1, (batch, ROIS)).astype(np.float32), rs.uniform(0, 0.999, (batch, TARGET_CFG["ROI_PER_IMAGE"])).astype(np.float32))


def build(dev, batch):
    """-> {side: callable -> (sampled indices, losses [3], gradient of rcnn_reg)}, the shapes"""
    rois, scores, labels, gt, u_fg, u_slot = [torch.from_numpy(v).to(dev) for v in inputs(batch)]
    n = batch * TARGET_CFG["ROI_PER_IMAGE"]
    gen = torch.Generator().manual_seed(1)
    rcnn_cls = (2 * torch.randn((n, 1), generator=gen)).to(dev).requires_grad_(True)
    rcnn_reg = (0.2 * torch.randn((n, 7), generator=gen)).to(dev).requires_grad_(True)
    layer = roi_heads.ProposalTargetLayer(TARGET_CFG)
    spec = ops.RcnnLossSpec(1.0, 1.0, 1.0, [1.0] * 7, corner_loss=True)
    batch_dict = {"batch_size": batch, "rois": rois, "roi_scores": scores, "roi_labels": labels, "gt_boxes": gt}

    def step(mode):
        def run():
            os.environ["DF3D_ROI_LOSS_FUSED"] = mode
            rcnn_cls.grad = rcnn_reg.grad = None
            t = layer(batch_dict, u_fg=u_fg, u_slot=u_slot)
            fn = ops.rcnn_loss if mode == "1" else roi_heads.composed_rcnn_losses
            losses = fn(rcnn_cls, rcnn_reg, t, spec)
            losses.sum().backward()
            return t["roi_inds"], losses.detach(), rcnn_reg.grad
        return run
    return {"fused": step("1"), "composed": step("0")}, dict(batch=batch, rois_per_frame=ROIS, sampled_per_frame=TARGET_CFG["ROI_PER_IMAGE"],
                                                             gt_per_frame=GT_PER_FRAME, gt_rows=GT_ROWS)


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
    ia, lossa, ga = sides["fused"]()
    ia, lossa, ga = ia.clone(), lossa.clone(), ga.clone()
    ib, lossb, gb = sides["composed"]()
    row = dict(what="targets + loss + grad", device=torch.cuda.get_device_name(0), windows=args.windows, calls_per_window=args.calls,
               same_samples=bool(torch.equal(ia, ib)), losses_fused=[round(float(v), 6) for v in lossa],
               losses_composed=[round(float(v), 6) for v in lossb], max_grad_difference=float((ga - gb).abs().max()),
               max_grad=float(gb.abs().max()), **shapes)
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
    os.environ.pop("DF3D_ROI_LOSS_FUSED", None)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
