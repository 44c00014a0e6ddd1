#!/usr/bin/env python3
"""Generate tests/golden/anchor_loss.npz FROM THE REFERENCE ITSELF: anchor targets and the RPN losses of Voxel-RCNN's first stage.

Runs only where the reference checkout exists.  The reference's own AnchorGenerator, ResidualCoder,
AxisAlignedTargetAssigner.assign_targets and AnchorHeadTemplate.get_cls_layer_loss / get_box_reg_layer_loss run on the CPU,
with the package stubs of make_golden_vrtail.import_reference_vr_tail (`Tensor.cuda` is the identity, the methods are called
with a SimpleNamespace as `self`).  Arrays only are stored: the inputs (anchors, ground truth, head maps), labels, dense
targets and weights, the three losses and the float32 autograd gradients of the three maps (the float32 yardstick).

Ground truth and head maps come from the seeded generators of tests/anchorloss_reference.py.  Seeds are searched until its
margin predicates hold (no anchor-max IoU within 1e-4 of a threshold, no arg-max ties, best and second-best IoU of a GT equal
or 1e-6 apart, direction-bin quotient 1e-3 from an integer, no |diff| within 1e-4 of beta), so that a label mismatch in a
test is a bug and not rounding; the coverage conditions are asserted on the stored fixture."""
import importlib
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
import anchorloss_reference as al  # noqa: E402
import vrtail_reference as vt  # noqa: E402


def run_reference(mods, name, anchors_list, per_loc, gt, cls, box, dirs):
    """-> labels, targets, weights, losses [3], gradients of the three maps (float32, the reference's own arithmetic)"""
    c = vt.CASES[name]
    B, H, W = c["B"], c["H"], c["W"]
    cfg = mv.attr(al.train_head_cfg(name))
    coder = mods["coder"].ResidualCoder()
    assigner = mods["assigner"].AxisAlignedTargetAssigner(model_cfg=cfg, class_names=al.TRAIN[name]["class_names"], box_coder=coder,
                                                          match_height=False)
    with torch.no_grad():
        t = assigner.assign_targets([a.clone() for a in anchors_list], torch.from_numpy(gt.copy()))
    labels, targets, weights = t["box_cls_labels"], t["box_reg_targets"], t["reg_weights"]
    T, lu = mods["head"].AnchorHeadTemplate, mods["loss"]
    leaf = lambda v: torch.from_numpy(v.copy()).view(B, H, W, -1).requires_grad_(True)
    p_cls, p_box, p_dir = leaf(cls), leaf(box), leaf(dirs) if c["NB"] else None
    ret = {"cls_preds": p_cls, "box_preds": p_box, "box_cls_labels": labels.clone(), "box_reg_targets": targets.clone()}
    if p_dir is not None:
        ret["dir_cls_preds"] = p_dir
    head = types.SimpleNamespace(forward_ret_dict=ret, num_class=c["C"], model_cfg=cfg, anchors=[a.clone() for a in anchors_list],
                                 use_multihead=False, num_anchors_per_location=sum(per_loc),
                                 cls_loss_func=lu.SigmoidFocalClassificationLoss(alpha=0.25, gamma=2.0),
                                 reg_loss_func=lu.WeightedSmoothL1Loss(code_weights=al.LOSS_WEIGHTS["code_weights"]),
                                 dir_loss_func=lu.WeightedCrossEntropyLoss(), add_sin_difference=T.add_sin_difference,
                                 get_direction_target=T.get_direction_target)
    cls_loss, tb = T.get_cls_layer_loss(head)
    box_loss, tb_box = T.get_box_reg_layer_loss(head)
    (cls_loss + box_loss).backward()
    out = np.array([tb["rpn_loss_cls"], tb_box["rpn_loss_loc"], tb_box.get("rpn_loss_dir", 0.0)], np.float32)
    grads = [p.grad.reshape(B, H * W * sum(per_loc), -1).numpy() if p is not None else None for p in (p_cls, p_box, p_dir)]
    return labels.numpy(), targets.numpy(), weights.numpy(), out, grads


def gen_anchor_loss():
    mods = mv.import_reference_vr_tail()
    mods["assigner"] = importlib.import_module("pcdet.models.dense_heads.target_assigner.axis_aligned_target_assigner")
    mods["loss"] = importlib.import_module("pcdet.utils.loss_utils")
    out = {}
    for name in ("car", "small", "multi"):
        c = vt.CASES[name]
        grid, rng = vt.case_geometry(name)
        gen = mods["gen"].AnchorGenerator(anchor_range=rng, anchor_generator_config=[mv.attr(s) for s in c["sets"]])
        anchors_list, per_loc = gen.generate_anchors([grid[:2] // 8 for _ in c["sets"]])
        anchors = torch.cat(anchors_list, dim=-3).numpy()
        flat = anchors.reshape(-1, 7)
        variants = [name] + (["nodir"] if name == "car" else [])
        sc, matched, unmatched = al.set_params(name)
        for seed in range(512):
            gt = al.make_gt(name, seed)
            cls, box, dirs = al.make_preds(name, seed)
            a = al.assign(flat, al.anchor_sets(name), sum(per_loc), gt, sc, matched, unmatched)
            l = al.losses(cls, box, dirs, flat, a["labels"], a["targets"], c["C"])
            ok = al.assign_clean(a) and al.loss_clean(l, True) and l["bins"] == {0, 1} and a["ignored"] > 0
            if name == "multi":                                    # pedestrian anchors at a 0.4 m pitch: GTs between the thresholds
                ok = ok and a["forced_only"] > 0
            if name == "car":                                      # the GT past the border of the range
                ok = ok and a["forced_below"] > 0
            if ok:
                break
        else:
            raise AssertionError("%s: no clean seed" % name)
        print("%s seed %d: num_pos %s thresh %.2e gap %.2e floor %.2e beta %.2e forced_only %d forced_below %d ignored %d" % (
            name, seed, a["num_pos"], a["thresh_dist"], a["positive_gap"], l["floor_dist"], l["beta_dist"], a["forced_only"],
            a["forced_below"], a["ignored"]))
        out.update({name + "_anchors": anchors, name + "_gt": gt, name + "_cls": cls, name + "_box": box, name + "_dir": dirs})
        for v in variants:
            labels, targets, weights, loss, grads = run_reference(mods, v, anchors_list, per_loc, gt, cls, box, dirs)
            out.update({v + "_labels": labels, v + "_targets": targets, v + "_weights": weights, v + "_loss": loss,
                        v + "_grad_cls": grads[0], v + "_grad_box": grads[1]})
            if grads[2] is not None:
                out[v + "_grad_dir"] = grads[2]
            print("%s losses %s" % (v, loss))
    mg.save("anchor_loss.npz", **out)
    check_fixture(dict(np.load(os.path.join(HERE, "anchor_loss.npz"))))


def check_fixture(g):
    """the margin and coverage conditions, on the stored arrays"""
    cover = dict(empty_frame=False, forced_only=0, forced_below=0, ignored=0, interior_zero=False, full_frame=False, outside=False,
                 unserved=False, bins=set())
    for name in vt.CASES:
        c, src = vt.CASES[name], al.source(name)
        a, l = al.restate(name, g)
        assert al.assign_clean(a), (name, a["thresh_dist"], a["argmax_ties"], a["positive_gap"], a["gt_gap_bad"])
        assert al.loss_clean(l, c["NB"] > 0), (name, l["beta_dist"], l["floor_dist"])
        assert np.array_equal(a["labels"], g[name + "_labels"]), name
        gt = g[src + "_gt"]
        _, rng = vt.case_geometry(name)
        served = al.set_params(name)[0]
        for b in range(c["B"]):
            n = al.valid_count(gt[b])
            zero = np.abs(gt[b, :, :7]).sum(1) == 0
            cover["empty_frame"] |= bool(zero.all())
            cover["interior_zero"] |= bool(zero[:n].any() and not zero.all())
            cover["full_frame"] |= not zero.any()
            cover["outside"] |= bool(((gt[b, :, 0] - gt[b, :, 3:5].max(1) > rng[3] + 5) & ~zero).any())
            cover["unserved"] |= bool((~zero & ~np.isin(gt[b, :, 7].astype(int), served)).any())
        assert a["num_pos"][-1] == 0 and (g[name + "_labels"][-1] == 0).all(), name
        cover["forced_only"] += a["forced_only"]
        cover["forced_below"] += a["forced_below"]
        cover["ignored"] += a["ignored"]
        cover["bins"] |= l["bins"]
        assert a["unmatched_gt"] > 0 or name != "car"
    print("coverage:", cover)
    assert cover["empty_frame"] and cover["forced_only"] > 0 and cover["forced_below"] > 0 and cover["ignored"] > 0
    assert cover["interior_zero"] and cover["full_frame"] and cover["outside"] and cover["unserved"] and cover["bins"] == {0, 1}
    for k, v in g.items():
        assert v.nbytes < 400 * 1024, (k, v.nbytes)


if __name__ == "__main__":
    gen_anchor_loss()
