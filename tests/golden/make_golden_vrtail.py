#!/usr/bin/env python3
"""Generate tests/golden/vr_tail.npz FROM THE REFERENCE ITSELF: the Voxel-RCNN tail from head maps to final boxes.

Runs only where the reference checkout exists.  The reference's own AnchorGenerator, ResidualCoder,
AnchorHeadTemplate.generate_predicted_boxes, model_nms_utils.class_agnostic_nms, RoIHeadTemplate.proposal_layer /
generate_predicted_boxes and Detector3DTemplate.post_processing run on the CPU: their packages are stubbed in sys.modules the
way make_golden.import_reference_vr_backbone does it (the stubs only satisfy `import`), `Tensor.cuda` is the identity, the
methods are called with a SimpleNamespace as `self`, and the CUDA-only `nms_gpu` is bound to the project's NMS oracle
(oracle.nms_bev), as the point ops are bound to the oracle elsewhere.

The inputs come from seeded generators.  Seeds are searched until the margin predicates of tests/vrtail_reference.py hold
(distinct selection scores, floor distance >= 1e-3, no IoU within 1e-4 of a threshold), so that an index mismatch in a test
is a bug and not rounding; the coverage conditions are asserted on the stored fixture."""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg  # noqa: E402  (paths, _stub, save)
import vrtail_reference as vt  # noqa: E402
from oracle import oracle as orc  # noqa: E402

R = "/root/reference/VoxelRCNN/pcdet"


class AttrDict(dict):
    """what the reference's configs are: a mapping with attribute access"""
    __getattr__ = dict.__getitem__

    def get(self, k, d=None):
        return dict.get(self, k, d)


def attr(d):
    return AttrDict({k: attr(v) if isinstance(v, dict) else v for k, v in d.items()})


def nms_gpu(boxes, scores, thresh, pre_maxsize=None, **kwargs):
    """the interface of pcdet.ops.iou3d_nms.iou3d_nms_utils.nms_gpu on the NMS oracle"""
    order = torch.sort(scores, descending=True, stable=True)[1]
    if pre_maxsize is not None:
        order = order[:pre_maxsize]
    keep, _ = orc.nms_bev(boxes[order].numpy(), thresh, rotated=True)
    return order[torch.from_numpy(keep)].contiguous(), None


def import_reference_vr_tail():
    for pkg, path in [("pcdet", R), ("pcdet.models", R + "/models"), ("pcdet.models.model_utils", R + "/models/model_utils"),
                      ("pcdet.ops", R + "/ops"), ("pcdet.utils", R + "/utils"), ("pcdet.models.dense_heads", R + "/models/dense_heads"),
                      ("pcdet.models.dense_heads.target_assigner", R + "/models/dense_heads/target_assigner"),
                      ("pcdet.models.roi_heads", R + "/models/roi_heads"),
                      ("pcdet.models.roi_heads.target_assigner", R + "/models/roi_heads/target_assigner"),
                      ("pcdet.models.detectors", R + "/models/detectors")]:
        mg._stub(pkg).__path__ = [path]
    mg._stub("SharedArray")
    mg._stub("pcdet.ops.iou3d_nms")
    mg._stub("pcdet.ops.iou3d_nms.iou3d_nms_utils", nms_gpu=nms_gpu)
    sys.modules["pcdet.ops.iou3d_nms"].iou3d_nms_utils = sys.modules["pcdet.ops.iou3d_nms.iou3d_nms_utils"]
    mg._stub("pcdet.ops.roiaware_pool3d")
    mg._stub("pcdet.ops.roiaware_pool3d.roiaware_pool3d_utils")
    sys.modules["pcdet.ops.roiaware_pool3d"].roiaware_pool3d_utils = sys.modules["pcdet.ops.roiaware_pool3d.roiaware_pool3d_utils"]
    mg._stub("pcdet.utils.spconv_utils", find_all_spconv_keys=None)
    for name in ("backbones_2d", "backbones_3d"):
        sys.modules["pcdet.models"].__dict__[name] = mg._stub("pcdet.models." + name)
    sys.modules["pcdet.models"].dense_heads = sys.modules["pcdet.models.dense_heads"]
    sys.modules["pcdet.models"].roi_heads = sys.modules["pcdet.models.roi_heads"]
    sys.modules["pcdet.models.backbones_2d"].map_to_bev = mg._stub("pcdet.models.backbones_2d.map_to_bev")
    sys.modules["pcdet.models.backbones_3d"].pfe = mg._stub("pcdet.models.backbones_3d.pfe")
    sys.modules["pcdet.models.backbones_3d"].vfe = mg._stub("pcdet.models.backbones_3d.vfe")
    torch.Tensor.cuda = lambda self, *a, **k: self
    mods = {}
    mods["gen"] = importlib.import_module("pcdet.models.dense_heads.target_assigner.anchor_generator")
    mods["coder"] = importlib.import_module("pcdet.utils.box_coder_utils")
    mods["head"] = importlib.import_module("pcdet.models.dense_heads.anchor_head_template")
    mods["nms"] = importlib.import_module("pcdet.models.model_utils.model_nms_utils")
    mods["roi"] = importlib.import_module("pcdet.models.roi_heads.roi_head_template")
    mods["det"] = importlib.import_module("pcdet.models.detectors.detector3d_template")
    return mods


def case_inputs(name, seed, anchors):
    """seeded head maps of a case: logits ~ 2 N(0, 1), residuals 0.05 N(0, 1) (neighbouring anchors of a 0.4 m pitch then
    overlap above 0.7); the LAST frame of 'car' draws every box tightly towards one of eight centres, so that fewer than POST
    remain"""
    c = vt.CASES[name]
    rs = np.random.RandomState(seed)
    per = anchors.reshape(-1, 7).shape[0]
    cls = (2 * rs.standard_normal((c["B"], per, c["C"]))).astype(np.float32)
    box = (0.05 * rs.standard_normal((c["B"], per, 7))).astype(np.float32)
    dirs = rs.standard_normal((c["B"], per, 2)).astype(np.float32)
    if name == "car":
        a = anchors.reshape(-1, 7).astype(np.float64)
        centres = np.stack([rs.uniform(1.0, 7.4, 8), rs.uniform(-4.0, 4.0, 8)], 1)
        pick = centres[rs.randint(0, 8, per)]
        diag = np.sqrt(a[:, 3] ** 2 + a[:, 4] ** 2)
        box[-1] *= np.float32(0.2)
        box[-1, :, 0] += ((pick[:, 0] - a[:, 0]) / diag).astype(np.float32)
        box[-1, :, 1] += ((pick[:, 1] - a[:, 1]) / diag).astype(np.float32)
    return cls, box, dirs


def run_proposals(mods, name, cls, box, dirs, anchors_list):
    c = vt.CASES[name]
    B, H, W = c["B"], c["H"], c["W"]
    self_head = types.SimpleNamespace(anchors=anchors_list, use_multihead=False, box_coder=mods["coder"].ResidualCoder(),
                                      model_cfg=attr({"DIR_OFFSET": vt.DIR_OFFSET, "DIR_LIMIT_OFFSET": vt.DIR_LIMIT_OFFSET,
                                                      "NUM_DIR_BINS": 2}))
    t = lambda v: torch.from_numpy(v).view(B, H, W, -1)
    with torch.no_grad():
        batch_cls, batch_box = mods["head"].AnchorHeadTemplate.generate_predicted_boxes(
            self_head, B, t(cls), t(box), t(dirs) if c["NB"] else None)
        bd = {"batch_size": B, "batch_cls_preds": batch_cls, "batch_box_preds": batch_box, "cls_preds_normalized": False}
        mods["roi"].RoIHeadTemplate.proposal_layer(types.SimpleNamespace(), bd, attr(vt.nms_cfg(name)))
    return batch_box.numpy(), bd


def run_final(mods, bd, rcnn_cls, rcnn_reg, raw):
    B = bd["batch_size"]
    with torch.no_grad():
        self_roi = types.SimpleNamespace(box_coder=mods["coder"].ResidualCoder())
        cls_preds, box_preds = mods["roi"].RoIHeadTemplate.generate_predicted_boxes(
            self_roi, B, bd["rois"], torch.from_numpy(rcnn_cls), torch.from_numpy(rcnn_reg))
        batch = dict(bd)
        batch.update(batch_cls_preds=cls_preds, batch_box_preds=box_preds, cls_preds_normalized=False)
        det = mods["det"].Detector3DTemplate
        self_det = types.SimpleNamespace(model_cfg=attr({"POST_PROCESSING": vt.post_cfg(raw)}), num_class=3,
                                         generate_recall_record=det.generate_recall_record)
        pred_dicts, _ = det.post_processing(self_det, batch)
    post = vt.FINAL["post"]
    boxes, scores = np.zeros((B, post, 7), np.float32), np.zeros((B, post), np.float32)
    labels, counts = np.zeros((B, post), np.int64), np.zeros((B,), np.int64)
    for b, p in enumerate(pred_dicts):
        m = counts[b] = len(p["pred_scores"])
        boxes[b, :m], scores[b, :m], labels[b, :m] = p["pred_boxes"].numpy(), p["pred_scores"].numpy(), p["pred_labels"].numpy()
    return box_preds.numpy(), boxes, scores, labels, counts


def rcnn_inputs(seed, B, N, empty_frame):
    rs = np.random.RandomState(seed)
    rcnn_cls = (2 * rs.standard_normal((B * N, 1))).astype(np.float32)
    if empty_frame is not None:                                    # nothing of this frame passes SCORE_THRESH
        rcnn_cls[empty_frame * N:(empty_frame + 1) * N] = -3 - np.abs(rcnn_cls[empty_frame * N:(empty_frame + 1) * N])
    rcnn_reg = (0.05 * rs.standard_normal((B * N, 7))).astype(np.float32)
    return rcnn_cls, rcnn_reg


def clean(ref, with_dir):
    return ref["min_gap"] > 0 and ref["close"] == 0 and (not with_dir or ref["floor_dist"] >= vt.FLOOR_MARGIN)


def gen_vr_tail():
    mods = import_reference_vr_tail()
    out, seeds = {}, {}
    for name in ("car", "small", "multi"):
        c = vt.CASES[name]
        grid, rng = vt.case_geometry(name)
        gen = mods["gen"].AnchorGenerator(anchor_range=rng, anchor_generator_config=[attr(s) for s in c["sets"]])
        anchors_list, per_loc = gen.generate_anchors([grid[:2] // 8 for _ in c["sets"]])
        anchors = torch.cat(anchors_list, dim=-3).numpy()           # [1, H, W, sizes, rotations, 7]
        assert anchors.shape[1:3] == (c["H"], c["W"]) and sum(per_loc) == anchors.shape[3] * anchors.shape[4]
        variants = [name] + (["nodir"] if name == "car" else [])
        for seed in range(64):
            cls, box, dirs = case_inputs(name, seed, anchors)
            refs = {v: vt.proposals(cls, box, dirs if vt.CASES[v]["NB"] else None, anchors.reshape(-1, 7), c["pre"], c["post"],
                                    c["thresh"], vt.DIR_OFFSET, vt.DIR_LIMIT_OFFSET) for v in variants}
            if all(clean(r, vt.CASES[v]["NB"]) for v, r in refs.items()):
                break
        else:
            raise AssertionError("%s: no clean seed" % name)
        seeds[name] = seed
        out.update({name + "_cls": cls, name + "_box": box, name + "_dir": dirs, name + "_anchors": anchors})
        for v in variants:
            dense, bd = run_proposals(mods, v, cls, box, dirs, anchors_list)
            out.update({v + "_dense": dense, v + "_rois": bd["rois"].numpy(), v + "_roi_scores": bd["roi_scores"].numpy(),
                        v + "_roi_labels": bd["roi_labels"].numpy()})
            print("%s seed %d: num %s suppressed %s gap %.2e floor %.2e close %d" % (
                v, seed, refs[v]["num"], refs[v]["suppressed"], refs[v]["min_gap"], refs[v]["floor_dist"], refs[v]["close"]))
            if v != "nodir":
                # the RCNN stage on these RoIs: 'car' is class agnostic with an empty frame, 'multi' carries the RoI labels
                if v == "small":
                    continue
                for rseed in range(64):
                    rcnn_cls, rcnn_reg = rcnn_inputs(1000 + rseed, c["B"], c["post"], 1 if v == "car" else None)
                    ref_boxes = vt.roi_decode(bd["rois"].numpy(), rcnn_reg)
                    fin = vt.final_select(ref_boxes, rcnn_cls, None, vt.FINAL["score_thresh"], vt.FINAL["thresh"],
                                          vt.FINAL["pre"], vt.FINAL["post"])
                    if fin["min_gap"] > 0 and fin["close"] == 0 and fin["thresh_dist"] >= 1e-4:
                        break
                else:
                    raise AssertionError("%s: no clean RCNN seed" % v)
                out.update({v + "_rcnn_cls": rcnn_cls, v + "_rcnn_reg": rcnn_reg})
                for raw in (False, True):
                    box_preds, fb, fs, fl, fc = run_final(mods, bd, rcnn_cls, rcnn_reg, raw)
                    tag = v + ("_raw" if raw else "")
                    out.update({v + "_box_preds": box_preds, tag + "_final_boxes": fb, tag + "_final_scores": fs,
                                tag + "_final_labels": fl, tag + "_final_counts": fc})
                print("%s rcnn seed %d: counts %s gap %.2e close %d thresh dist %.2e" % (
                    v, 1000 + rseed, fc, fin["min_gap"], fin["close"], fin["thresh_dist"]))
    mg.save("vr_tail.npz", **out)
    check_fixture(dict(np.load(os.path.join(HERE, "vr_tail.npz"))))


def check_fixture(g):
    """the margin and coverage conditions, on the stored arrays"""
    cover = dict(clipped=False, padded=False, suppressed=0, few_anchors=False, empty_final=False, zero_rois_pass=False)
    for v, c in vt.CASES.items():
        src = "car" if v == "nodir" else v
        ref = vt.proposals(g[src + "_cls"], g[src + "_box"], g[src + "_dir"] if c["NB"] else None, g[src + "_anchors"].reshape(-1, 7),
                           c["pre"], c["post"], c["thresh"], vt.DIR_OFFSET, vt.DIR_LIMIT_OFFSET)
        assert ref["min_gap"] > 0 and ref["close"] == 0, (v, ref["min_gap"], ref["close"])
        assert not c["NB"] or ref["floor_dist"] >= vt.FLOOR_MARGIN, (v, ref["floor_dist"])
        per = g[src + "_cls"].shape[1]
        cover["few_anchors"] |= per < c["pre"]
        for b in range(c["B"]):
            kept = min(c["pre"], per) - ref["suppressed"][b]
            cover["clipped"] |= kept > c["post"]
            cover["padded"] |= kept < c["post"]
            cover["suppressed"] = max(cover["suppressed"], int(ref["suppressed"][b]))
        # the reference's results are the restatement's, index by index
        want = np.where(ref["index"][..., None] >= 0, g[v + "_dense"][np.arange(c["B"])[:, None], np.maximum(ref["index"], 0)], 0)
        assert np.array_equal(want, g[v + "_rois"]), v
        assert np.array_equal(ref["roi_labels"], g[v + "_roi_labels"]), v
    for v in ("car", "multi"):
        fin = vt.final_select(vt.roi_decode(g[v + "_rois"], g[v + "_rcnn_reg"]), g[v + "_rcnn_cls"], None, vt.FINAL["score_thresh"],
                              vt.FINAL["thresh"], vt.FINAL["pre"], vt.FINAL["post"])
        assert fin["min_gap"] > 0 and fin["close"] == 0 and fin["thresh_dist"] >= 1e-4, v
        assert np.array_equal(fin["counts"], g[v + "_final_counts"]), v
        cover["empty_final"] |= bool((fin["counts"] == 0).any())
        zero = np.abs(g[v + "_rois"]).sum(-1) == 0
        cover["zero_rois_pass"] |= bool((zero[np.arange(len(zero))[:, None], np.maximum(fin["index"], 0)] & (fin["index"] >= 0)).any())
    print("coverage:", cover)
    assert cover["clipped"] and cover["padded"] and cover["suppressed"] >= 50 and cover["few_anchors"] and cover["empty_final"]
    assert cover["zero_rois_pass"]


if __name__ == "__main__":
    gen_vr_tail()
