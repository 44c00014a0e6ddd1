#!/usr/bin/env python3
"""Time of the PV-RCNN keypoint segmentation tail (csrc/pointhead.hip) at the shipped size, fused against composed
(`DF3D_POINT_HEAD_FUSED=0`): point targets + the focal segmentation loss + the gradient of point_cls_preds.

  B = 8 frames of 2048 keypoints (NUM_KEYPOINTS of the shipped PFE), three classes, 20 seeded boxes per frame in 24
  ground-truth rows, GT_EXTRA_WIDTH 0.2; two thirds of the keypoints lie around the boxes.
  fused     ops.point_head_targets (one launch for all frames) + ops.point_cls_loss + backward (one gradient launch);
  composed  the reference's formulation in torch, vectorised over [P, G] with no per-frame loop
            (dense_heads.composed_point_targets / composed_point_cls_loss under autograd): one-hot and weights tensors.

The same inputs for both sides, warmed up, alternating window by window in one process, device events around the windows;
median and range per side, torch.cuda.max_memory_allocated of one call of each side.  Kernel launches and traced memory
copies per call come from rocprofv3 traces of child processes (`--count SIDE`), and the device-to-host reads of a call from
torch's synchronisation debug mode, both as tools/bench_vr_tail.py counts them.

    python tools/bench_point_head.py [--windows 7] [--calls 5] [--out FILE] [--no-trace]"""
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
from dualfusion import dense_heads, ops  # noqa: E402

SIDES = ("fused", "composed")
KEYPOINTS, GT_PER_FRAME, GT_ROWS, NUM_CLASS = 2048, 20, 24, 3
EXTRA = (0.2, 0.2, 0.2)
SIZES = np.array([[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]])


def inputs(batch):
    rs = np.random.RandomState(7)
    gt = np.zeros((batch, GT_ROWS, 8), np.float32)
    cls = rs.randint(1, 4, (batch, GT_PER_FRAME))
    gt[:, :GT_PER_FRAME, 0], gt[:, :GT_PER_FRAME, 1] = rs.uniform(2, 68, cls.shape), rs.uniform(-38, 38, cls.shape)
    gt[:, :GT_PER_FRAME, 2] = -1.0
    gt[:, :GT_PER_FRAME, 3:6] = SIZES[cls - 1] * rs.uniform(0.8, 1.25, cls.shape + (3,))
    gt[:, :GT_PER_FRAME, 6], gt[:, :GT_PER_FRAME, 7] = rs.uniform(-np.pi, np.pi, cls.shape), cls
    src = gt[np.arange(batch)[:, None], rs.randint(0, GT_PER_FRAME, (batch, KEYPOINTS))]
    near = src[..., :3] + rs.uniform(-0.8, 0.8, (batch, KEYPOINTS, 3)) * (src[..., 3:6] + 0.6)
    far = np.stack([rs.uniform(0, 70.4, (batch, KEYPOINTS)), rs.uniform(-40, 40, (batch, KEYPOINTS)), rs.uniform(-3, 1, (batch, KEYPOINTS))], -1)
    xyz = np.where(rs.uniform(0, 1, (batch, KEYPOINTS, 1)) < 0.67, near, far)
    frame = np.broadcast_to(np.arange(batch, dtype=np.float64)[:, None, None], (batch, KEYPOINTS, 1))
    return np.concatenate([frame, xyz], -1).reshape(-1, 4).astype(np.float32), gt


def build(dev, batch):
    """-> {side: callable -> (labels, loss [1], gradient of point_cls_preds)}, the shapes"""
    points, gt = [torch.from_numpy(v).to(dev) for v in inputs(batch)]
    gen = torch.Generator().manual_seed(1)
    preds = (2 * torch.randn((points.shape[0], NUM_CLASS), generator=gen)).to(dev).requires_grad_(True)

    def step(mode):
        def run():
            os.environ["DF3D_POINT_HEAD_FUSED"] = mode
            preds.grad = None
            if mode == "1":
                labels = ops.point_head_targets(points, gt, EXTRA, NUM_CLASS)
                loss, _ = ops.point_cls_loss(preds, labels, 1.0)
            else:
                with torch.no_grad():
                    labels, _ = dense_heads.composed_point_targets(points, gt, EXTRA, NUM_CLASS)
                loss, _ = dense_heads.composed_point_cls_loss(preds, labels, 1.0)
            loss[0].backward()
            return labels, loss.detach(), preds.grad
        return run
    return {"fused": step("1"), "composed": step("0")}, dict(batch=batch, keypoints_per_frame=KEYPOINTS, num_class=NUM_CLASS,
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
    la, lossa, ga = sides["fused"]()
    la, lossa, ga = la.clone(), lossa.clone(), ga.clone()
    lb, lossb, gb = sides["composed"]()
    row = dict(what="point targets + loss + grad", device=torch.cuda.get_device_name(0), windows=args.windows,
               calls_per_window=args.calls, labels_differ=int((la != lb).sum()), positives=int((la > 0).sum()),
               ignored=int((la < 0).sum()), loss_fused=round(float(lossa), 6), loss_composed=round(float(lossb), 6),
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
    os.environ.pop("DF3D_POINT_HEAD_FUSED", None)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
