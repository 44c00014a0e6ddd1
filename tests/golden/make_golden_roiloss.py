#!/usr/bin/env python3
"""Generate tests/golden/roi_loss.npz FROM THE REFERENCE ITSELF: the proposal targets and the RCNN losses of Voxel-RCNN's
second stage.

Runs only where the reference checkout exists.  The reference's own ProposalTargetLayer.forward, RoIHeadTemplate.assign_targets,
get_box_cls_layer_loss and get_box_reg_layer_loss (with ResidualCoder, WeightedSmoothL1Loss and get_corner_loss_lidar) run on
the CPU, with the package stubs of make_golden_vrtail.import_reference_vr_tail (`Tensor.cuda` is the identity, the methods are
called with a SimpleNamespace as `self`).  The CUDA-only `boxes_iou3d_gpu` is bound to the float64 restatement
(roiloss_reference.iou3d, returned as the float32 tensor the reference's op returns), as `nms_gpu` is bound to the NMS oracle.

The reference's three host random sources are replaced per frame, and nothing else of its code:
    np.random.permutation(n)        -> argsort(u_fg[b, :n], stable)
    np.random.rand(M)               -> u_slot[b]
    torch.randint(0, h, (k,))       -> floor(float64(u_slot[b, c:c+k]) * h), the cursor c starting at the frame's fg count and
                                       advancing by k per call
(`subsample_rois` is wrapped only to tell the replacements which frame is running and how many fg slots it fills).  Its
fg-only branch hands `torch.cat` a Python list (`bg_inds = []`), which this torch refuses: while the reference samples,
`torch.cat` takes an empty list for an empty index tensor.  Likewise `F.binary_cross_entropy` of this torch refuses the -1
labels of CLS_SCORE_TYPE 'cls' that the reference masks out AFTER the call: during the classification loss the targets are
clamped to [0, 1] for the call; the masked rows are multiplied by zero as the reference does.

Arrays only are stored: the inputs with the draws, all of the reference's target tensors (the class labels for both
CLS_SCORE_TYPEs), the three float32 losses and the float32 autograd gradients of rcnn_cls and rcnn_reg.  Seeds are searched
until the margin predicates of tests/roiloss_reference.py hold; margins and coverage are asserted on the stored file."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg  # noqa: E402  (save)
import make_golden_vrtail as mv  # noqa: E402  (the package stubs, attr)
import roiloss_reference as rl  # noqa: E402

STATE = {}


def boxes_iou3d_gpu(boxes_a, boxes_b):
    return torch.from_numpy(rl.iou3d(boxes_a.numpy(), boxes_b.numpy()).astype(np.float32))


def install_draws(mods):
    layer = mods["ptl"].ProposalTargetLayer
    original = layer.subsample_rois

    def subsample_rois(self, max_overlaps):
        cfg = self.roi_sampler_cfg
        n_fg = int((max_overlaps >= min(cfg.REG_FG_THRESH, cfg.CLS_FG_THRESH)).sum())
        per_image = int(np.round(cfg.FG_RATIO * cfg.ROI_PER_IMAGE))
        STATE["frame"] = STATE.get("frame", -1) + 1
        STATE["cursor"] = min(per_image, n_fg) if 0 < n_fg < max_overlaps.numel() else 0
        cat = torch.cat
        torch.cat = lambda ts, dim=0: cat([max_overlaps.new_zeros((0,), dtype=torch.long) if isinstance(v, list) and not v else v
                                           for v in ts], dim=dim)
        try:
            return original(self, max_overlaps)
        finally:
            torch.cat = cat

    def permutation(n):
        return np.argsort(STATE["u_fg"][STATE["frame"], :n], kind="stable")

    def rand(m):
        return STATE["u_slot"][STATE["frame"]].astype(np.float64)[:m]

    def randint(low, high, size):
        k, c = int(size[0]), STATE["cursor"]
        STATE["cursor"] = c + k
        return torch.from_numpy(np.floor(STATE["u_slot"][STATE["frame"], c:c + k].astype(np.float64) * high).astype(np.int64)) + low

    layer.subsample_rois = subsample_rois
    np.random.permutation, np.random.rand, torch.randint = permutation, rand, randint


def run_targets(mods, cfg, rois, scores, labels, gt, u_fg, u_slot):
    STATE.update(frame=-1, u_fg=u_fg, u_slot=u_slot)
    head = types.SimpleNamespace(proposal_target_layer=mods["ptl"].ProposalTargetLayer(roi_sampler_cfg=mv.attr(cfg)))
    batch = {"batch_size": rois.shape[0], "rois": torch.from_numpy(rois.copy()), "roi_scores": torch.from_numpy(scores.copy()),
             "roi_labels": torch.from_numpy(labels.copy()), "gt_boxes": torch.from_numpy(gt.copy())}
    return mods["roi"].RoIHeadTemplate.assign_targets(head, batch)


def run_losses(mods, t, rcnn_cls, rcnn_reg):
    T, lu = mods["roi"].RoIHeadTemplate, mods["loss"]
    w = rl.LOSS_CFG["LOSS_WEIGHTS"]
    head = types.SimpleNamespace(model_cfg=mv.attr({"LOSS_CONFIG": rl.LOSS_CFG}), box_coder=mods["coder"].ResidualCoder(),
                                 reg_loss_func=lu.WeightedSmoothL1Loss(code_weights=w["code_weights"]))
    p_cls, p_reg = torch.from_numpy(rcnn_cls.copy()).requires_grad_(True), torch.from_numpy(rcnn_reg.copy()).requires_grad_(True)
    ret = {k: v.clone() for k, v in t.items()}                       # (encode_torch clamps the sizes of gt_of_rois in place)
    ret.update(rcnn_cls=p_cls, rcnn_reg=p_reg)
    F = mods["roi"].F
    bce = F.binary_cross_entropy
    F.binary_cross_entropy = lambda x, target, **kw: bce(x, target.clamp(0, 1), **kw)
    try:
        cls_loss, tb = T.get_box_cls_layer_loss(head, ret)
    finally:
        F.binary_cross_entropy = bce
    reg_loss, tb_reg = T.get_box_reg_layer_loss(head, ret)
    (cls_loss + reg_loss).backward()
    loss = np.array([tb["rcnn_loss_cls"], tb_reg["rcnn_loss_reg"], tb_reg.get("rcnn_loss_corner", 0.0)], np.float32)
    return loss, p_cls.grad.numpy(), p_reg.grad.numpy()


def gen_roi_loss():
    import importlib
    mods = mv.import_reference_vr_tail()
    mods["ptl"] = importlib.import_module("pcdet.models.roi_heads.target_assigner.proposal_target_layer")
    mods["loss"] = importlib.import_module("pcdet.utils.loss_utils")
    sys.modules["pcdet.ops.iou3d_nms.iou3d_nms_utils"].boxes_iou3d_gpu = boxes_iou3d_gpu
    install_draws(mods)
    out = {}
    for name in rl.CASES:
        cfg = rl.sampler_cfg(name)
        for seed in range(256):
            rois, scores, labels, gt, u_fg, u_slot = rl.make_inputs(name, seed)
            rcnn_cls, rcnn_reg = rl.make_preds(seed, rl.B * rl.M)
            g = {name + "_" + k: v for k, v in dict(rois=rois, roi_scores=scores, roi_labels=labels, gt=gt, u_fg=u_fg, u_slot=u_slot,
                                                   rcnn_cls=rcnn_cls, rcnn_reg=rcnn_reg).items()}
            t, l = rl.restate(name, g)
            cov = rl.coverage(name, g, t, l)
            if rl.targets_clean(t) and rl.keys_distinct(u_fg) and rl.loss_clean(l) and covered(name, cov):
                break
        else:
            raise AssertionError("%s: no clean seed" % name)
        print("%s seed %d: counts %s thresh %.2e gap %.2e heading %.2e beta %.2e corner %.2e flip %.2e" % (
            name, seed, t["counts"].tolist(), t["thresh_dist"], t["gap"], t["heading_dist"], l["beta_dist"], l["corner_dist"], l["flip_gap"]))
        out.update(g)
        for score in ("roi_iou", "cls"):
            ref = run_targets(mods, dict(cfg, CLS_SCORE_TYPE=score), rois, scores, labels, gt, u_fg, u_slot)
            out[name + "_t_cls_labels_" + score] = ref["rcnn_cls_labels"].numpy()
            if score == cfg["CLS_SCORE_TYPE"]:
                own = ref
        for k in ("rois", "gt_of_rois", "gt_of_rois_src", "gt_iou_of_rois", "roi_scores", "roi_labels", "reg_valid_mask", "rcnn_cls_labels"):
            out[name + "_t_" + k] = own[k].numpy()
        loss, grad_cls, grad_reg = run_losses(mods, own, rcnn_cls, rcnn_reg)
        out.update({name + "_loss": loss, name + "_grad_cls": grad_cls, name + "_grad_reg": grad_reg})
        print("%s losses %s" % (name, loss))
    mg.save("roi_loss.npz", **out)
    check_fixture(dict(np.load(os.path.join(HERE, "roi_loss.npz"))))


def covered(name, cov):
    frames = all(cov[k] for k in ("more_fg", "fewer_fg", "hard_only", "easy_only", "fg_only", "empty_frame", "interior_zero"))
    return (frames and cov["fold"] == {True, False} and cov["huber"] == {True, False} and cov["reg"] == {True, False} and
            (cov["unserved"] or not rl.CASES[name]["by_class"]))


def check_fixture(g):
    """the margin and coverage conditions, and the restatement's exact agreement, on the stored arrays"""
    for name in rl.CASES:
        t, l = rl.restate(name, g)
        assert rl.targets_clean(t) and rl.keys_distinct(g[name + "_u_fg"]) and rl.loss_clean(l), name
        cov = rl.coverage(name, g, t, l)
        print(name, "coverage:", cov)
        assert covered(name, cov), (name, cov)
        assert np.array_equal(t["rois"].astype(np.float32), g[name + "_t_rois"]), name
        assert np.array_equal(t["roi_labels"], g[name + "_t_roi_labels"]) and np.array_equal(t["reg_valid_mask"], g[name + "_t_reg_valid_mask"])
        assert np.array_equal(t["cls_labels_cls"], g[name + "_t_cls_labels_cls"]), name
    assert {rl.CASES[n]["score"] for n in rl.CASES} == {"roi_iou", "cls"} and {rl.CASES[n]["by_class"] for n in rl.CASES} == {True, False}
    for k, v in g.items():
        assert v.nbytes < 400 * 1024, (k, v.nbytes)


if __name__ == "__main__":
    gen_roi_loss()
