#!/usr/bin/env python3
"""Generate tests/golden/point_head.npz FROM THE REFERENCE ITSELF: the targets and the loss of PointHeadSimple.

Runs only where the reference checkout exists.  The reference's own PointHeadSimple.assign_targets (over
PointHeadTemplate.assign_stack_targets and box_utils.enlarge_box3d) and get_cls_layer_loss (over
SigmoidFocalClassificationLoss) run on the CPU in float32, their packages stubbed in sys.modules the way make_golden_vsa does it
(the stubs only satisfy `import`).

The compiled `points_in_boxes_gpu` cannot be built here, so it is replaced by the float32 restatement of its kernel
(tests/pointhead_reference.py: points_in_boxes).  THIS FIXTURE THEREFORE PINS THE PYTHON AROUND THE KERNEL -- the per-frame
masks, the enlarged boxes, the ignore flag, the class lookup, the one-hot loss -- AND NOT THE KERNEL (the caveat of
mmdet_restated.py).  The kernel's geometry is pinned separately: tests/test_pointhead_host.py checks the restatement against a
float64 brute force on these margin-clean cases (near_face == 0).

Inputs are the seeded cases of tests/pointhead_reference.py, which the tests rebuild from the same seeds; the fixture stores
the reference's OUTPUTS only (labels per case and class count; loss, positive count and gradient per loss case)."""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg  # noqa: E402  (_stub, save)
import make_golden_vrtail as mv  # noqa: E402  (attr, import_reference_vr_tail)
import pointhead_reference as pr  # noqa: E402

UPSTREAM = 2.5


def points_in_boxes_gpu(points, boxes):
    """roiaware_pool3d_utils.points_in_boxes_gpu (points [B, M, 3], boxes [B, T, 7]) on the host restatement of the kernel"""
    return torch.from_numpy(pr.points_in_boxes(boxes.numpy(), points.numpy())).int()


def import_reference():
    mv.import_reference_vr_tail()
    sys.modules["pcdet.ops.roiaware_pool3d.roiaware_pool3d_utils"].points_in_boxes_gpu = points_in_boxes_gpu
    return importlib.import_module("pcdet.models.dense_heads.point_head_simple")


def make_head(mod, num_class, extra):
    cfg = mv.attr({"CLS_FC": [8], "CLASS_AGNOSTIC": False, "TARGET_CONFIG": {"GT_EXTRA_WIDTH": list(extra)},
                   "LOSS_CONFIG": {"LOSS_REG": "smooth-l1", "LOSS_WEIGHTS": {"point_cls_weight": pr.LOSS_WEIGHT}}})
    return mod.PointHeadSimple(num_class=num_class, input_channels=4, model_cfg=cfg)


def gen_point_head():
    mod = import_reference()
    out = {}
    for name in pr.TARGET_CASES:
        points, gt, extra = pr.target_case(name)
        assert pr.near_face(points, gt, extra) == 0, name
        for num_class in (1, 3):
            head = make_head(mod, num_class, extra)
            got = head.assign_targets({"point_coords": torch.from_numpy(points), "gt_boxes": torch.from_numpy(gt)})
            labels = got["point_cls_labels"].numpy()
            assert labels.dtype == np.int64
            assert np.array_equal(labels, pr.assign_targets(points, gt, extra, num_class)[0]), (name, num_class)
            out["%s_labels_c%d" % (name, num_class)] = labels
    for name in pr.LOSS_CASES:
        preds, labels = pr.loss_case(name)
        head = make_head(mod, preds.shape[1], pr.EXTRA)
        x = torch.from_numpy(preds).requires_grad_(True)
        head.forward_ret_dict = {"point_cls_preds": x, "point_cls_labels": torch.from_numpy(labels)}
        loss, tb = head.get_cls_layer_loss()
        (UPSTREAM * loss).backward()
        want = pr.loss_and_grad(preds, labels, pr.LOSS_WEIGHT, torch.float32, UPSTREAM)
        assert float(loss) == want[0] and tb["point_pos_num"] == want[1] and np.array_equal(x.grad.double().numpy(), want[2]), name
        out[name + "_loss"] = np.float32(float(loss))
        out[name + "_pos_num"] = np.float32(tb["point_pos_num"])
        out[name + "_grad"] = x.grad.numpy()
    return out


if __name__ == "__main__":
    arrs = gen_point_head()
    mg.save("point_head.npz", **arrs)
    print("point_head.npz: %d arrays, %d bytes" % (len(arrs), os.path.getsize(os.path.join(HERE, "point_head.npz"))))
