"""AnchorHeadSingle (VR/pcdet/models/dense_heads/anchor_head_single.py over anchor_head_template.py) for inference, plus the
two plain-torch modules in front of it: HeightCompression and BaseBEVBackbone (VR/pcdet/models/backbones_2d/).  The
reference's constructor signatures, config keys and parameter names, so its checkpoints load.

In eval the head has two modes, chosen per call by DF3D_VR_TAIL_FUSED (default 1):
  fused     the three 1x1 convolutions run as ONE convolution into channels-last pixel rows; the rows and the anchor TABLES go
            into batch_dict (`dense_cls_rows`, `dense_box_rows`, `dense_dir_rows`, `dense_anchor_tables`) and no anchor is
            decoded here: VoxelRCNNHead.proposal_layer decodes the NMS_PRE_MAXSIZE selected ones (csrc/proposals.hip);
  composed  `batch_cls_preds`, `batch_box_preds`, `cls_preds_normalized=False` as the reference's generate_predicted_boxes
            makes them (every anchor decoded in torch).
`forward` makes proposals and stays an eval-mode call: in training mode it raises NotImplementedError.

Training of this first stage is `forward_train` + `get_loss`: AxisAlignedTargetAssigner and the RPN losses (classification focal
loss, smooth-L1 regression, direction cross entropy), chosen per call by DF3D_ANCHOR_LOSS_FUSED (default 1):
  fused     ops.anchor_assign + ops.anchor_loss (csrc/anchorloss.hip): one call each for all frames and anchor sets, anchors
            from the tables, the regression target encoded only at the positives, no device-to-host read;
  composed  the reference's formulation in torch under autograd: per-frame dense IoU matrices, one-hot targets and three
            dense loss maps.
TRAIN-mode proposals are not made here: forward_train returns no RoIs (the RoI head's targets and losses are in roi_heads.py);
`write_train_predictions` hands a RoI head the detached predictions of that pass, as the PVRCNN detector does.

PointHeadSimple, the keypoint segmentation head of the PV-RCNN tree, is at the end of this file."""
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .registry import BACKBONES_2D, DENSE_HEADS, MAP_TO_BEV


def _get(cfg, key, default=None):
    """config nodes are EasyDicts in pcdet and plain dicts here"""
    if isinstance(cfg, dict):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


def tail_fused():
    """DF3D_VR_TAIL_FUSED, read per call (default: fused)"""
    return os.environ.get("DF3D_VR_TAIL_FUSED", "1") != "0"


def limit_period(val, offset=0.5, period=np.pi):
    """VR/pcdet/utils/common_utils.py:limit_period"""
    return val - torch.floor(val / period + offset) * period


def residual_decode(box_encodings, anchors):
    """ResidualCoder.decode_torch (VR/pcdet/utils/box_coder_utils.py:45-77) without the sin/cos variant: [..., 7] each."""
    xa, ya, za, dxa, dya, dza, ra = torch.split(anchors, 1, dim=-1)
    xt, yt, zt, dxt, dyt, dzt, rt = torch.split(box_encodings, 1, dim=-1)
    diagonal = torch.sqrt(dxa ** 2 + dya ** 2)
    xg = xt * diagonal + xa
    yg = yt * diagonal + ya
    zg = zt * dza + za
    dxg = torch.exp(dxt) * dxa
    dyg = torch.exp(dyt) * dya
    dzg = torch.exp(dzt) * dza
    rg = rt + ra
    return torch.cat([xg, yg, zg, dxg, dyg, dzg, rg], dim=-1)


class AnchorTables(object):
    """The anchors of one head as the kernel reads them: x_shifts [sets, W], y_shifts [sets, H] float32, and per anchor
    a = size * rotations + rotation its set and (centre z, dx, dy, dz, rotation).  `dense()` is the reference's anchor
    tensor [1, H, W, sizes, rotations, 7] (AnchorGenerator.generate_anchors, sets concatenated along the size axis)."""

    def __init__(self, anchor_generator_cfg, grid_size, point_cloud_range):
        sets = list(anchor_generator_cfg)
        if not sets:
            raise ValueError("ANCHOR_GENERATOR_CONFIG is empty")
        maps = [tuple(int(v) for v in (np.asarray(grid_size)[:2] // _get(c, "feature_map_stride"))) for c in sets]
        if any(m != maps[0] for m in maps):
            raise NotImplementedError("anchor sets whose feature-map sizes differ are not supported (got %s)" % (maps,))
        self.W, self.H = maps[0]
        rng = point_cloud_range
        xs, ys, self.anchor_set, rows = [], [], [], []
        num_rot = None
        for s, c in enumerate(sets):
            sizes, rots, heights = _get(c, "anchor_sizes"), _get(c, "anchor_rotations"), _get(c, "anchor_bottom_heights")
            if len(heights) != 1:
                raise NotImplementedError("more than one anchor_bottom_heights per anchor set is not supported: the reference's "
                                          "anchor order then no longer matches the [H, W, A] map layout")
            if num_rot is not None and len(rots) != num_rot:
                raise NotImplementedError("anchor sets with different numbers of anchor_rotations are not supported")
            num_rot = len(rots)
            if _get(c, "align_center", False):
                x_stride, y_stride = (rng[3] - rng[0]) / self.W, (rng[4] - rng[1]) / self.H
                x_offset, y_offset = x_stride / 2, y_stride / 2
            else:
                x_stride, y_stride = (rng[3] - rng[0]) / (self.W - 1), (rng[4] - rng[1]) / (self.H - 1)
                x_offset, y_offset = 0, 0
            x = torch.arange(rng[0] + x_offset, rng[3] + 1e-5, step=x_stride, dtype=torch.float32)
            y = torch.arange(rng[1] + y_offset, rng[4] + 1e-5, step=y_stride, dtype=torch.float32)
            if x.numel() != self.W or y.numel() != self.H:
                raise ValueError("anchor set %d: the shift tables have %d x %d entries for a %d x %d map"
                                 % (s, x.numel(), y.numel(), self.W, self.H))
            xs.append(x)
            ys.append(y)
            size_t = torch.tensor(sizes, dtype=torch.float32).view(-1, 3)
            z = torch.tensor(heights, dtype=torch.float32)[0] + size_t[:, 2] / 2         # bottom height -> box centre, in float32
            for k in range(size_t.shape[0]):
                for r in rots:
                    self.anchor_set.append(s)
                    rows.append(torch.stack([z[k], size_t[k, 0], size_t[k, 1], size_t[k, 2], torch.tensor(r, dtype=torch.float32)]))
        self.num_rotations = num_rot
        self.x_shifts, self.y_shifts = torch.stack(xs), torch.stack(ys)
        self.table = torch.stack(rows)                                                  # [A, 5]
        self.num_anchors_per_location = len(self.anchor_set)
        if self.num_anchors_per_location > ops.MAX_ANCHORS:
            raise NotImplementedError("at most %d anchors per location (got %d)" % (ops.MAX_ANCHORS, self.num_anchors_per_location))
        self._device = {}

    def dense(self):
        A, H, W = self.num_anchors_per_location, self.H, self.W
        sets = torch.tensor(self.anchor_set)
        out = torch.empty((1, H, W, A, 7), dtype=torch.float32)
        out[..., 0] = self.x_shifts[sets].t().view(1, 1, W, A)
        out[..., 1] = self.y_shifts[sets].t().view(1, H, 1, A)
        out[..., 2:] = self.table.view(1, 1, 1, A, 5)
        return out.view(1, H, W, A // self.num_rotations, self.num_rotations, 7)

    def on(self, device):
        """(x_shifts, y_shifts) on the device"""
        hit = self._device.get(str(device))
        if hit is None:
            hit = self._device[str(device)] = (self.x_shifts.to(device).contiguous(), self.y_shifts.to(device).contiguous())
        return hit

    def per_set(self):
        """the reference's anchor list: one [H*W*A_s, 7] tensor per anchor set"""
        flat = self.dense().view(self.H, self.W, self.num_anchors_per_location, 7)
        slots = [[a for a, s in enumerate(self.anchor_set) if s == k] for k in range(self.x_shifts.shape[0])]
        return [flat[:, :, idx, :].reshape(-1, 7) for idx in slots]


def anchor_loss_fused():
    """DF3D_ANCHOR_LOSS_FUSED, read per call (default: fused)"""
    return os.environ.get("DF3D_ANCHOR_LOSS_FUSED", "1") != "0"


class ResidualCoder(object):
    """VR/pcdet/utils/box_coder_utils.py:ResidualCoder without the sin/cos variant"""
    code_size = 7

    @staticmethod
    def encode_torch(boxes, anchors):
        anchors = torch.cat([anchors[:, :3], torch.clamp_min(anchors[:, 3:6], 1e-5), anchors[:, 6:]], dim=-1)
        boxes = torch.cat([boxes[:, :3], torch.clamp_min(boxes[:, 3:6], 1e-5), boxes[:, 6:]], dim=-1)
        xa, ya, za, dxa, dya, dza, ra = torch.split(anchors[:, :7], 1, dim=-1)
        xg, yg, zg, dxg, dyg, dzg, rg = torch.split(boxes[:, :7], 1, dim=-1)
        diagonal = torch.sqrt(dxa ** 2 + dya ** 2)
        return torch.cat([(xg - xa) / diagonal, (yg - ya) / diagonal, (zg - za) / dza, torch.log(dxg / dxa), torch.log(dyg / dya),
                          torch.log(dzg / dza), rg - ra], dim=-1)

    decode_torch = staticmethod(residual_decode)


def nearest_bev_iou(boxes_a, boxes_b):
    """boxes3d_nearest_bev_iou (VR/pcdet/utils/box_utils.py:286-335): [N, 7], [G, 7] -> [N, G]"""
    def aligned(b):
        rot = limit_period(b[:, 6], 0.5, np.pi).abs()
        dims = torch.where(rot[:, None] < np.pi / 4, b[:, [3, 4]], b[:, [4, 3]])
        return torch.cat((b[:, 0:2] - dims / 2, b[:, 0:2] + dims / 2), dim=1)
    a, b = aligned(boxes_a), aligned(boxes_b)
    x_len = torch.clamp_min(torch.min(a[:, 2, None], b[None, :, 2]) - torch.max(a[:, 0, None], b[None, :, 0]), 0)
    y_len = torch.clamp_min(torch.min(a[:, 3, None], b[None, :, 3]) - torch.max(a[:, 1, None], b[None, :, 1]), 0)
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    inter = x_len * y_len
    return inter / torch.clamp_min(area_a[:, None] + area_b[None, :] - inter, 1e-6)


class AxisAlignedTargetAssigner(object):
    """VR/pcdet/models/dense_heads/target_assigner/axis_aligned_target_assigner.py.  Fused (DF3D_ANCHOR_LOSS_FUSED=1, the
    default): one library call for all frames and anchor sets (ops.anchor_assign), anchors read from the AnchorTables.
    Composed (=0): the reference's formulation in torch, frame by frame with a dense IoU matrix per anchor set."""

    def __init__(self, model_cfg, class_names, box_coder, match_height=False):
        target_cfg = _get(model_cfg, "TARGET_ASSIGNER_CONFIG") or {}
        if _get(model_cfg, "USE_MULTIHEAD", False):
            raise NotImplementedError("USE_MULTIHEAD is not supported by the target assigner")
        if _get(target_cfg, "NAME", "AxisAlignedTargetAssigner") != "AxisAlignedTargetAssigner":
            raise NotImplementedError("TARGET_ASSIGNER_CONFIG.NAME: %s is not supported (ATSS has no kernel here)" % _get(target_cfg, "NAME"))
        if match_height or _get(target_cfg, "MATCH_HEIGHT", False):
            raise NotImplementedError("MATCH_HEIGHT is not supported: the anchors are matched by nearest-BEV IoU")
        if _get(target_cfg, "POS_FRACTION", -1.0) >= 0:
            raise NotImplementedError("POS_FRACTION >= 0 is not supported: the reference samples with the host's torch.randperm")
        if _get(target_cfg, "NORM_BY_NUM_EXAMPLES", False):
            raise NotImplementedError("NORM_BY_NUM_EXAMPLES is not supported")
        self.box_coder = box_coder
        self.match_height = False
        self.class_names = list(class_names)
        sets = list(_get(model_cfg, "ANCHOR_GENERATOR_CONFIG"))
        self.anchor_class_names = [_get(c, "class_name") for c in sets]
        for n in self.anchor_class_names:
            if n not in self.class_names:
                raise ValueError("anchor set class %r is not one of class_names %s" % (n, self.class_names))
        self.set_class = [self.class_names.index(n) + 1 for n in self.anchor_class_names]
        self.matched_thresholds = [float(_get(c, "matched_threshold")) for c in sets]
        self.unmatched_thresholds = [float(_get(c, "unmatched_threshold")) for c in sets]

    def assign_targets(self, all_anchors, gt_boxes_with_classes, dense=True):
        """all_anchors: the head's AnchorTables; gt_boxes_with_classes [B, M, 8] on the device.  -> box_cls_labels [B, H*W*A]
        int32, box_reg_targets [B, H*W*A, 7], reg_weights [B, H*W*A] float32 (the last two only with `dense`), and what the
        fused losses read instead of the dense targets: gt_ids [B, H*W*A] int32, num_pos [B] int32."""
        if not isinstance(all_anchors, AnchorTables):
            raise TypeError("assign_targets takes the head's AnchorTables (head.tables): anchors are not materialised")
        t = all_anchors
        gt = gt_boxes_with_classes.to(torch.float32).contiguous()
        if anchor_loss_fused():
            x_shifts, y_shifts = t.on(gt.device)
            out = ops.anchor_assign(x_shifts, y_shifts, gt, t.H, t.W, t.anchor_set, _table_list(t), self.set_class,
                                    self.matched_thresholds, self.unmatched_thresholds, dense=dense)
        else:
            out = self._assign_composed(t, gt)
        ret = {"box_cls_labels": out[0], "gt_ids": out[1], "num_pos": out[2]}
        if len(out) > 3:
            ret["box_reg_targets"], ret["reg_weights"] = out[3], out[4]
        return ret

    def _assign_composed(self, t, gt):
        anchors_list = [a.to(gt.device) for a in t.per_set()]
        B, A = gt.shape[0], t.num_anchors_per_location
        labels_all, ids_all, targets_all, weights_all = [], [], [], []
        for k in range(B):
            cur_gt = gt[k, :, :7]
            nz = (cur_gt.sum(dim=1) != 0).nonzero()[:, 0]
            cnt = int(nz[-1]) if nz.numel() else 0
            cur_gt = cur_gt[:cnt + 1]
            cur_cls = gt[k, :cnt + 1, 7].int()
            rows = torch.arange(cnt + 1, device=gt.device, dtype=torch.int32)
            per_set = []
            for s, anchors in enumerate(anchors_list):
                mask = cur_cls == self.set_class[s]
                per_set.append(self._assign_single(anchors, cur_gt[mask], cur_cls[mask], rows[mask], self.matched_thresholds[s],
                                                   self.unmatched_thresholds[s]))
            fm = (t.H, t.W)
            labels_all.append(torch.cat([p[0].view(*fm, -1) for p in per_set], dim=-1).view(-1))
            ids_all.append(torch.cat([p[1].view(*fm, -1) for p in per_set], dim=-1).view(-1))
            targets_all.append(torch.cat([p[2].view(*fm, -1, 7) for p in per_set], dim=-2).view(-1, 7))
            weights_all.append(torch.cat([p[3].view(*fm, -1) for p in per_set], dim=-1).view(-1))
        labels = torch.stack(labels_all)
        assert labels.shape[1] == t.H * t.W * A
        return labels, torch.stack(ids_all), (labels > 0).sum(1).int(), torch.stack(targets_all), torch.stack(weights_all)

    def _assign_single(self, anchors, gt_boxes, gt_classes, gt_rows, matched_threshold, unmatched_threshold):
        """assign_targets_single (lines 132-210) without sampling; gt_ids name rows of the frame's gt_boxes"""
        n, dev = anchors.shape[0], anchors.device
        labels = torch.full((n,), -1, dtype=torch.int32, device=dev)
        gt_ids = torch.full((n,), -1, dtype=torch.int32, device=dev)
        targets = anchors.new_zeros((n, 7))
        if gt_boxes.shape[0] == 0:
            labels[:] = 0
            return labels, gt_ids, targets, anchors.new_zeros((n,))
        overlap = nearest_bev_iou(anchors, gt_boxes)
        anchor_to_gt_argmax = overlap.argmax(dim=1)
        anchor_to_gt_max = overlap[torch.arange(n, device=dev), anchor_to_gt_argmax]
        gt_to_anchor_max = overlap.max(dim=0)[0]
        gt_to_anchor_max = torch.where(gt_to_anchor_max == 0, torch.full_like(gt_to_anchor_max, -1), gt_to_anchor_max)
        with_max = (overlap == gt_to_anchor_max).nonzero()[:, 0]
        force = anchor_to_gt_argmax[with_max]
        labels[with_max] = gt_classes[force]
        gt_ids[with_max] = gt_rows[force]
        pos = anchor_to_gt_max >= matched_threshold
        labels[pos] = gt_classes[anchor_to_gt_argmax[pos]]
        gt_ids[pos] = gt_rows[anchor_to_gt_argmax[pos]]
        labels[(anchor_to_gt_max < unmatched_threshold).nonzero()[:, 0]] = 0
        labels[with_max] = gt_classes[force]
        fg = (labels > 0).nonzero()[:, 0]
        targets[fg] = self.box_coder.encode_torch(gt_boxes[anchor_to_gt_argmax[fg]], anchors[fg])
        weights = anchors.new_zeros((n,))
        weights[labels > 0] = 1.0
        return labels, gt_ids, targets, weights


def _table_list(tables):
    hit = tables.__dict__.get("_table_list")
    if hit is None:
        hit = tables.__dict__["_table_list"] = tables.table.tolist()
    return hit


def sigmoid_focal_loss(logits, target, weights, alpha=0.25, gamma=2.0):
    """SigmoidFocalClassificationLoss.forward (VR/pcdet/utils/loss_utils.py:9-72)"""
    p = torch.sigmoid(logits)
    alpha_weight = target * alpha + (1 - target) * (1 - alpha)
    pt = target * (1.0 - p) + (1.0 - target) * p
    bce = torch.clamp(logits, min=0) - logits * target + torch.log1p(torch.exp(-torch.abs(logits)))
    return alpha_weight * torch.pow(pt, gamma) * bce * weights.unsqueeze(-1)


def weighted_smooth_l1(pred, target, code_weights, weights, beta):
    """WeightedSmoothL1Loss.forward (loss_utils.py:75-136)"""
    target = torch.where(torch.isnan(target), pred, target)
    n = torch.abs((pred - target) * code_weights.view(1, 1, -1))
    return torch.where(n < beta, 0.5 * n ** 2 / beta, n - 0.5 * beta) * weights.unsqueeze(-1)


@DENSE_HEADS.register_module
class AnchorHeadSingle(nn.Module):
    def __init__(self, model_cfg, input_channels, num_class, class_names, grid_size, point_cloud_range,
                 predict_boxes_when_training=True, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_class = num_class
        self.class_names = class_names
        self.predict_boxes_when_training = predict_boxes_when_training
        if _get(model_cfg, "USE_MULTIHEAD", False):
            raise NotImplementedError("USE_MULTIHEAD is not supported")
        target_cfg = _get(model_cfg, "TARGET_ASSIGNER_CONFIG") or {}
        coder = _get(target_cfg, "BOX_CODER", "ResidualCoder")
        if coder != "ResidualCoder":
            raise NotImplementedError("BOX_CODER %s is not supported (PreviousResidualDecoder and the others have no decode here)" % coder)
        if _get(_get(target_cfg, "BOX_CODER_CONFIG") or {}, "encode_angle_by_sincos", False):
            raise NotImplementedError("encode_angle_by_sincos is not supported")
        self.code_size = 7
        self.tables = AnchorTables(_get(model_cfg, "ANCHOR_GENERATOR_CONFIG"), grid_size, point_cloud_range)
        self.anchors = self.tables.dense()
        self.num_anchors_per_location = self.tables.num_anchors_per_location
        self.target_assigner = None              # made by the first training call (_training_setup)
        self.forward_ret_dict = {}

        A = self.num_anchors_per_location
        self.conv_cls = nn.Conv2d(input_channels, A * self.num_class, kernel_size=1)
        self.conv_box = nn.Conv2d(input_channels, A * self.code_size, kernel_size=1)
        if _get(model_cfg, "USE_DIRECTION_CLASSIFIER", None) is not None:
            self.num_dir_bins = int(_get(model_cfg, "NUM_DIR_BINS"))
            self.conv_dir_cls = nn.Conv2d(input_channels, A * self.num_dir_bins, kernel_size=1)
        else:
            self.num_dir_bins = 0
            self.conv_dir_cls = None
        self.init_weights()

    def init_weights(self):
        pi = 0.01
        nn.init.constant_(self.conv_cls.bias, -np.log((1 - pi) / pi))
        nn.init.normal_(self.conv_box.weight, mean=0, std=0.001)

    def _convs(self):
        return [c for c in (self.conv_cls, self.conv_box, self.conv_dir_cls) if c is not None]

    def head_rows(self, spatial_features_2d):
        """The three 1x1 convolutions as one -> channels-last pixel rows [B*H*W, A*(C + 7 + NB)] and their column views."""
        convs = self._convs()
        weight, bias = ops.derived(self.__dict__, "_df3d_cat", [p for c in convs for p in (c.weight, c.bias)],
                                   lambda: (torch.cat([c.weight for c in convs]).detach(), torch.cat([c.bias for c in convs]).detach()))
        y = F.conv2d(spatial_features_2d, weight, bias)
        rows = y.permute(0, 2, 3, 1).contiguous().view(-1, y.shape[1])
        n_cls, n_box = self.conv_cls.out_channels, self.conv_box.out_channels
        cls_rows, box_rows = rows[:, :n_cls], rows[:, n_cls:n_cls + n_box]
        dir_rows = rows[:, n_cls + n_box:] if self.conv_dir_cls is not None else None
        return cls_rows, box_rows, dir_rows

    def generate_predicted_boxes(self, batch_size, cls_preds, box_preds, dir_cls_preds=None):
        """anchor_head_template.py:225-272: every anchor decoded; cls_preds / box_preds / dir_cls_preds [B, H, W, channels]."""
        anchors = self.anchors.to(box_preds.device)
        num_anchors = anchors.view(-1, 7).shape[0]
        batch_anchors = anchors.view(1, -1, 7).repeat(batch_size, 1, 1)
        batch_cls_preds = cls_preds.reshape(batch_size, num_anchors, -1).float()
        batch_box_preds = residual_decode(box_preds.reshape(batch_size, num_anchors, -1), batch_anchors)
        if dir_cls_preds is not None:
            dir_offset, dir_limit_offset = _get(self.model_cfg, "DIR_OFFSET"), _get(self.model_cfg, "DIR_LIMIT_OFFSET")
            dir_labels = torch.max(dir_cls_preds.reshape(batch_size, num_anchors, -1), dim=-1)[1]
            period = 2 * np.pi / self.num_dir_bins
            dir_rot = limit_period(batch_box_preds[..., 6] - dir_offset, dir_limit_offset, period)
            batch_box_preds[..., 6] = dir_rot + dir_offset + period * dir_labels.to(batch_box_preds.dtype)
        return batch_cls_preds, batch_box_preds

    # ---- training: targets and RPN losses (csrc/anchorloss.hip) -------------------------------------------------------
    def _training_setup(self):
        """target assigner and loss weights, made on first use: an eval-only config needs neither key"""
        if self.target_assigner is None:
            loss_cfg = _get(self.model_cfg, "LOSS_CONFIG")
            if loss_cfg is None:
                raise KeyError("LOSS_CONFIG: the anchor losses need LOSS_WEIGHTS (cls_weight, loc_weight, dir_weight, code_weights)")
            reg = _get(loss_cfg, "REG_LOSS_TYPE", None)
            if reg not in (None, "WeightedSmoothL1Loss"):
                raise NotImplementedError("REG_LOSS_TYPE %s is not supported" % reg)
            w = _get(loss_cfg, "LOSS_WEIGHTS")
            self.loss_weights = {k: float(_get(w, k)) for k in ("cls_weight", "loc_weight", "dir_weight")}
            self.code_weights = [float(v) for v in _get(w, "code_weights")]
            if len(self.code_weights) != self.code_size:
                raise ValueError("code_weights must have %d entries" % self.code_size)
            target_cfg = _get(self.model_cfg, "TARGET_ASSIGNER_CONFIG") or {}
            self.target_assigner = AxisAlignedTargetAssigner(self.model_cfg, self.class_names, ResidualCoder(),
                                                             match_height=_get(target_cfg, "MATCH_HEIGHT", False))
        return self.target_assigner

    def assign_targets(self, gt_boxes):
        """gt_boxes [B, M, 8] on the device -> the targets dict of AxisAlignedTargetAssigner.assign_targets; the dense
        regression targets are made only where something reads them (the composed losses)"""
        return self._training_setup().assign_targets(self.tables, gt_boxes, dense=not anchor_loss_fused())

    def forward_train(self, data_dict):
        """The reference's training-mode forward: the three maps as [B, H, W, channels] views of ONE row buffer that carries
        gradient to the live conv_* parameters, and the targets of data_dict['gt_boxes'].  Returns no RoIs."""
        x = data_dict["spatial_features_2d"]
        B, _, H, W = x.shape
        if (H, W) != (self.tables.H, self.tables.W):
            raise ValueError("AnchorHeadSingle: the map is %d x %d, the anchors were built for %d x %d" % (H, W, self.tables.H, self.tables.W))
        convs = self._convs()
        y = F.conv2d(x, torch.cat([c.weight for c in convs]), torch.cat([c.bias for c in convs]))
        rows = y.permute(0, 2, 3, 1).contiguous().view(-1, y.shape[1])
        n_cls, n_box = self.conv_cls.out_channels, self.conv_box.out_channels
        ret = {"rows": rows, "cls_preds": rows[:, :n_cls].view(B, H, W, n_cls),
               "box_preds": rows[:, n_cls:n_cls + n_box].view(B, H, W, n_box), "gt_boxes": data_dict["gt_boxes"]}
        if self.conv_dir_cls is not None:
            ret["dir_cls_preds"] = rows[:, n_cls + n_box:].view(B, H, W, -1)
        ret.update(self.assign_targets(data_dict["gt_boxes"]))
        self.forward_ret_dict = ret
        return data_dict

    def _fused_losses(self):
        """[3] = rpn_loss_cls, rpn_loss_loc, rpn_loss_dir: one call per forward_train, shared by the two get_*_loss"""
        r = self.forward_ret_dict
        if "rpn_losses" not in r:
            rows = r["rows"]
            n_cls, n_box = self.conv_cls.out_channels, self.conv_box.out_channels
            gt = r["gt_boxes"].to(torch.float32).contiguous()
            x_shifts, y_shifts = self.tables.on(rows.device)
            has_dir = self.conv_dir_cls is not None
            spec = ops.AnchorLossSpec((0, n_cls, n_cls + n_box if has_dir else None), x_shifts, y_shifts, r["box_cls_labels"],
                                      r["gt_ids"], r["num_pos"], gt, self.tables.H, self.tables.W, self.num_class, self.num_dir_bins,
                                      self.tables.anchor_set, _table_list(self.tables), self.loss_weights["cls_weight"],
                                      self.loss_weights["loc_weight"], self.loss_weights["dir_weight"], self.code_weights,
                                      dir_offset=_get(self.model_cfg, "DIR_OFFSET", 0.0) if has_dir else 0.0)
            r["rpn_losses"] = ops.anchor_loss(rows, spec)
        return r["rpn_losses"]

    def get_cls_layer_loss(self):
        """anchor_head_template.py:101-135; tb_dict values are device tensors"""
        self._training_setup()
        if anchor_loss_fused():
            cls_loss = self._fused_losses()[0]
            return cls_loss, {"rpn_loss_cls": cls_loss.detach()}
        r = self.forward_ret_dict
        cls_preds, labels = r["cls_preds"], r["box_cls_labels"]
        B = int(cls_preds.shape[0])
        cared, positives = labels >= 0, labels > 0
        cls_weights = ((labels == 0) * 1.0 + 1.0 * positives).float()
        if self.num_class == 1:
            labels = torch.where(positives, torch.ones_like(labels), labels)
        cls_weights = cls_weights / torch.clamp(positives.sum(1, keepdim=True).float(), min=1.0)
        cls_targets = labels * cared.type_as(labels)
        one_hot = torch.zeros(*cls_targets.shape, self.num_class + 1, dtype=cls_preds.dtype, device=cls_preds.device)
        one_hot.scatter_(-1, cls_targets.unsqueeze(-1).long(), 1.0)
        loss = sigmoid_focal_loss(cls_preds.reshape(B, -1, self.num_class), one_hot[..., 1:], cls_weights)
        cls_loss = loss.sum() / B * self.loss_weights["cls_weight"]
        return cls_loss, {"rpn_loss_cls": cls_loss.detach()}

    def get_box_reg_layer_loss(self):
        """anchor_head_template.py:162-214; tb_dict values are device tensors"""
        self._training_setup()
        has_dir = self.conv_dir_cls is not None
        if anchor_loss_fused():
            losses = self._fused_losses()
            tb = {"rpn_loss_loc": losses[1].detach()}
            if has_dir:
                tb["rpn_loss_dir"] = losses[2].detach()
                return losses[1] + losses[2], tb
            return losses[1], tb
        r = self.forward_ret_dict
        box_preds, targets, labels = r["box_preds"], r["box_reg_targets"], r["box_cls_labels"]
        B = int(box_preds.shape[0])
        positives = labels > 0
        reg_weights = positives.float() / torch.clamp(positives.sum(1, keepdim=True).float(), min=1.0)
        anchors = self.anchors.to(box_preds.device).view(1, -1, 7).repeat(B, 1, 1)
        box_preds = box_preds.reshape(B, -1, self.code_size)
        sin_pred = torch.sin(box_preds[..., 6:7]) * torch.cos(targets[..., 6:7])          # add_sin_difference
        sin_tgt = torch.cos(box_preds[..., 6:7]) * torch.sin(targets[..., 6:7])
        pred = torch.cat([box_preds[..., :6], sin_pred], dim=-1)
        tgt = torch.cat([targets[..., :6], sin_tgt], dim=-1)
        code_weights = ops.device_constant(self.code_weights, torch.float32, pred.device)
        loc_loss = weighted_smooth_l1(pred, tgt, code_weights, reg_weights, 1.0 / 9.0).sum() / B * self.loss_weights["loc_weight"]
        tb = {"rpn_loss_loc": loc_loss.detach()}
        box_loss = loc_loss
        if has_dir:
            rot_gt = targets[..., 6] + anchors[..., 6]                                        # get_direction_target
            offset_rot = limit_period(rot_gt - _get(self.model_cfg, "DIR_OFFSET"), 0, 2 * np.pi)
            dir_targets = torch.clamp(torch.floor(offset_rot / (2 * np.pi / self.num_dir_bins)).long(), min=0, max=self.num_dir_bins - 1)
            dir_logits = r["dir_cls_preds"].reshape(B, -1, self.num_dir_bins)
            weights = positives.type_as(dir_logits)
            weights = weights / torch.clamp(weights.sum(-1, keepdim=True), min=1.0)
            dir_loss = (F.cross_entropy(dir_logits.permute(0, 2, 1), dir_targets, reduction="none") * weights).sum() / B
            dir_loss = dir_loss * self.loss_weights["dir_weight"]
            box_loss = box_loss + dir_loss
            tb["rpn_loss_dir"] = dir_loss.detach()
        return box_loss, tb

    def get_loss(self):
        """-> (rpn_loss, tb_dict): rpn_loss_cls, rpn_loss_loc, rpn_loss_dir (with direction classifier), rpn_loss"""
        cls_loss, tb_dict = self.get_cls_layer_loss()
        box_loss, tb_box = self.get_box_reg_layer_loss()
        tb_dict.update(tb_box)
        rpn_loss = cls_loss + box_loss
        tb_dict["rpn_loss"] = rpn_loss.detach()
        return rpn_loss, tb_dict

    def forward(self, data_dict):
        if self.training:
            raise NotImplementedError("AnchorHeadSingle.forward makes proposals and runs in eval mode only (TRAIN-mode proposals "
                                      "and the RoI head's targets are not implemented); the first-stage training pass is "
                                      "forward_train + get_loss")
        x = data_dict["spatial_features_2d"]
        B, _, H, W = x.shape
        if (H, W) != (self.tables.H, self.tables.W):
            raise ValueError("AnchorHeadSingle: the map is %d x %d, the anchors were built for %d x %d" % (H, W, self.tables.H, self.tables.W))
        cls_rows, box_rows, dir_rows = self.head_rows(x)
        return self.write_predictions(data_dict, cls_rows, box_rows, dir_rows, B, H, W)

    def write_predictions(self, data_dict, cls_rows, box_rows, dir_rows, B, H, W):
        """What `forward` leaves for the RoI head, from the three column views of the head's row buffer: the rows and the
        anchor tables (fused mode) or every anchor decoded (composed mode)."""
        if tail_fused():
            data_dict["dense_cls_rows"], data_dict["dense_box_rows"], data_dict["dense_dir_rows"] = cls_rows, box_rows, dir_rows
            data_dict["dense_anchor_tables"] = {
                "tables": self.tables, "H": H, "W": W, "num_class": self.num_class,
                "dir_offset": _get(self.model_cfg, "DIR_OFFSET", 0.0) if dir_rows is not None else 0.0,
                "dir_limit_offset": _get(self.model_cfg, "DIR_LIMIT_OFFSET", 0.0) if dir_rows is not None else 0.0}
            return data_dict
        view = lambda r: None if r is None else r.reshape(B, H, W, -1)
        batch_cls_preds, batch_box_preds = self.generate_predicted_boxes(B, view(cls_rows), view(box_rows), view(dir_rows))
        data_dict["batch_cls_preds"] = batch_cls_preds
        data_dict["batch_box_preds"] = batch_box_preds
        data_dict["cls_preds_normalized"] = False
        return data_dict

    def write_train_predictions(self, data_dict):
        """After `forward_train`: the first stage's predictions of that pass, DETACHED, under the keys `forward` writes, so
        that a RoI head can make its TRAIN proposals from them (the reference's predict_boxes_when_training; its
        generate_predicted_boxes runs on detached maps too: the RoIs carry no gradient into this head)."""
        r = self.forward_ret_dict
        if not r or "rows" not in r:
            raise KeyError("AnchorHeadSingle.write_train_predictions follows forward_train")
        rows = r["rows"].detach()
        B, H, W = r["cls_preds"].shape[:3]
        n_cls, n_box = self.conv_cls.out_channels, self.conv_box.out_channels
        dir_rows = rows[:, n_cls + n_box:] if self.conv_dir_cls is not None else None
        with torch.no_grad():
            return self.write_predictions(data_dict, rows[:, :n_cls], rows[:, n_cls:n_cls + n_box], dir_rows, int(B), int(H), int(W))


def point_head_fused():
    """DF3D_POINT_HEAD_FUSED, read per call (default: fused)"""
    return os.environ.get("DF3D_POINT_HEAD_FUSED", "1") != "0"


def composed_point_targets(points, gt_boxes, extra_width, num_class):
    """assign_stack_targets (point_head_template.py:49-129, ignore flag, no box or part labels) with points_in_boxes_gpu in
    torch, vectorised over [P, G] with no per-frame loop: float32 rotation, double comparisons, first box wins.
    -> labels [P] int64, box_idx [P] int64 (-1: in no box)."""
    P, (B, G) = points.shape[0], gt_boxes.shape[:2]
    labels = torch.zeros((P,), dtype=torch.int64, device=points.device)
    if G == 0 or P == 0 or B == 0:
        return labels, torch.full((P,), -1, dtype=torch.int64, device=points.device)
    points, gt_boxes = points.float(), gt_boxes.float()
    bf = points[:, 0]
    frame = torch.clamp(bf, 0, B - 1).long()
    valid = (bf >= 0) & (bf < B) & (frame.to(bf.dtype) == bf)
    boxes = gt_boxes[frame]                                                    # [P, G, 8]
    extra = ops.device_constant([float(v) for v in extra_width], torch.float32, points.device)
    x, y, z = points[:, 1:2], points[:, 2:3], points[:, 3:4]
    az = torch.abs(z - boxes[..., 2]).double()
    sx, sy = x - boxes[..., 0], y - boxes[..., 1]
    cosa, sina = torch.cos(-boxes[..., 6]), torch.sin(-boxes[..., 6])
    ax = torch.abs(sx * cosa + sy * (-sina)).double()
    ay = torch.abs(sx * sina + sy * cosa).double()
    margin = float(np.float32(1e-5))

    def inside(sizes):
        half = sizes.double() / 2.0
        return ~(az > half[..., 2]) & (ax < half[..., 0] + margin) & (ay < half[..., 1] + margin) & valid[:, None]
    plain, ext = inside(boxes[..., 3:6]), inside(boxes[..., 3:6] + extra)
    first = (torch.cumsum(plain.long(), dim=1) == 0).sum(dim=1)                # the first box that holds the point, G if none
    fg = first < G
    idx = torch.clamp(first, max=G - 1)
    cls = torch.ones_like(labels) if num_class == 1 else boxes[torch.arange(P, device=points.device), idx, 7].long()
    labels = torch.where(fg ^ ext.any(dim=1), torch.full_like(labels, -1), labels)      # the reference's order: ignore flag,
    labels = torch.where(fg, cls, labels)                                              # then the class over every fg row
    return labels, torch.where(fg, first, torch.full_like(first, -1))


def composed_point_cls_loss(point_cls_preds, point_cls_labels, weight):
    """get_cls_layer_loss (point_head_template.py:131-155) in torch under autograd: one-hot targets and a weights tensor.
    -> (loss, pos_num) as 1-element tensors."""
    num_class = point_cls_preds.shape[1]
    positives = point_cls_labels > 0
    cls_weights = ((point_cls_labels == 0) * 1.0 + 1.0 * positives).to(point_cls_preds.dtype)
    pos_normalizer = positives.sum(dim=0).to(point_cls_preds.dtype)
    cls_weights = cls_weights / torch.clamp(pos_normalizer, min=1.0)
    one_hot = point_cls_preds.new_zeros(point_cls_labels.shape[0], num_class + 1)
    one_hot.scatter_(-1, (point_cls_labels * (point_cls_labels >= 0).long()).unsqueeze(dim=-1), 1.0)
    loss = sigmoid_focal_loss(point_cls_preds, one_hot[..., 1:], cls_weights).sum() * weight
    return loss.view(1), pos_normalizer.view(1)


@DENSE_HEADS.register_module
class PointHeadSimple(nn.Module):
    """VR/pcdet/models/dense_heads/point_head_simple.py:7-97 over point_head_template.py: the keypoint segmentation head of
    PV-RCNN.  The reference's constructor, config keys (CLS_FC, CLASS_AGNOSTIC, USE_POINT_FEATURES_BEFORE_FUSION,
    TARGET_CONFIG.GT_EXTRA_WIDTH, LOSS_CONFIG.LOSS_WEIGHTS.point_cls_weight) and parameter names (cls_layers.{0,1,3,4,..}).

    `forward` writes batch_dict['point_cls_scores'] [P] (max over classes of the sigmoid) and, in training mode, assigns the
    targets of batch_dict['gt_boxes'] to batch_dict['point_coords']; `get_loss` is the focal segmentation loss.  The FC
    layers run on channels-last rows (F.linear + ops.batch_norm_rows).  Targets and loss are chosen per call by
    DF3D_POINT_HEAD_FUSED (default 1):
      fused     ops.point_head_targets + ops.point_cls_loss (csrc/pointhead.hip): one launch for all frames, no one-hot and
                no weights tensor, nothing read back; CPU tensors are refused;
      composed  the reference's formulation in torch under autograd, vectorised over [P, G] with no per-frame loop.
    PointHeadBox, PointIntraPartOffsetHead and this fork's AuxPointHeadSimple are not provided."""

    def __init__(self, num_class, input_channels, model_cfg, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_class = int(num_class)
        fc_cfg = _get(model_cfg, "CLS_FC")
        if fc_cfg is None:
            raise KeyError("PointHeadSimple: the config has no CLS_FC")
        self.cls_layers = self.make_fc_layers(list(fc_cfg), input_channels, self.num_class)
        self.forward_ret_dict = None

    @staticmethod
    def make_fc_layers(fc_cfg, input_channels, output_channels):
        """point_head_template.py:35-47"""
        fc_layers, c_in = [], input_channels
        for width in fc_cfg:
            fc_layers.extend([nn.Linear(c_in, width, bias=False), nn.BatchNorm1d(width), nn.ReLU()])
            c_in = width
        fc_layers.append(nn.Linear(c_in, output_channels, bias=True))
        return nn.Sequential(*fc_layers)

    def _training_setup(self):
        """extra width and loss weight, read on first use: an eval-only config needs neither key"""
        if getattr(self, "point_cls_weight", None) is None:
            target_cfg = _get(self.model_cfg, "TARGET_CONFIG")
            extra = _get(target_cfg, "GT_EXTRA_WIDTH") if target_cfg is not None else None
            if extra is None:
                raise KeyError("PointHeadSimple: the targets need TARGET_CONFIG.GT_EXTRA_WIDTH")
            if len(extra) != 3:
                raise ValueError("PointHeadSimple: GT_EXTRA_WIDTH must have 3 entries (got %d)" % len(extra))
            weights = _get(_get(self.model_cfg, "LOSS_CONFIG") or {}, "LOSS_WEIGHTS") or {}
            w = _get(weights, "point_cls_weight")
            if w is None:
                raise KeyError("PointHeadSimple: the loss needs LOSS_CONFIG.LOSS_WEIGHTS.point_cls_weight")
            self.gt_extra_width = [float(v) for v in extra]
            self.point_cls_weight = float(w)

    def assign_targets(self, input_dict):
        """point_head_simple.py:20-53: point_coords [P, 4] (b, x, y, z), gt_boxes [B, G, 8] -> {'point_cls_labels' [P] int64}"""
        self._training_setup()
        point_coords, gt_boxes = input_dict["point_coords"], input_dict["gt_boxes"]
        if gt_boxes.dim() != 3 or gt_boxes.shape[2] != 8 or point_coords.dim() != 2 or point_coords.shape[1] != 4:
            raise ValueError("PointHeadSimple: point_coords must be [P, 4] and gt_boxes [B, G, 8] (got %s, %s)"
                             % (tuple(point_coords.shape), tuple(gt_boxes.shape)))
        if point_head_fused():
            labels = ops.point_head_targets(point_coords.detach().to(torch.float32).contiguous(),
                                            gt_boxes.detach().to(torch.float32).contiguous(), self.gt_extra_width, self.num_class)
        else:
            with torch.no_grad():
                labels, _ = composed_point_targets(point_coords, gt_boxes, self.gt_extra_width, self.num_class)
        return {"point_cls_labels": labels}

    def cls_rows(self, point_features):
        """cls_layers on channels-last rows [P, C] -> point_cls_preds [P, num_class]"""
        x, layers = point_features, list(self.cls_layers)
        for k in range(0, len(layers) - 1, 3):
            x = ops.batch_norm_rows(layers[k + 1], F.linear(x, layers[k].weight), relu=True)
        return F.linear(x, layers[-1].weight, layers[-1].bias)

    def forward(self, batch_dict):
        key = "point_features_before_fusion" if _get(self.model_cfg, "USE_POINT_FEATURES_BEFORE_FUSION", False) else "point_features"
        point_features = batch_dict[key]
        if point_head_fused() and not point_features.is_cuda:
            raise ops._lib.Df3dError("PointHeadSimple: %s must live on the GPU (got %s); the fused mode has no CPU path "
                                     "(DF3D_POINT_HEAD_FUSED=0 is the torch composition)" % (key, point_features.device))
        point_cls_preds = self.cls_rows(point_features)
        ret_dict = {"point_cls_preds": point_cls_preds}
        batch_dict["point_cls_scores"] = torch.sigmoid(point_cls_preds).max(dim=-1)[0]
        if self.training:
            ret_dict["point_cls_labels"] = self.assign_targets(batch_dict)["point_cls_labels"]
        self.forward_ret_dict = ret_dict
        return batch_dict

    def get_cls_layer_loss(self, tb_dict=None):
        """point_head_template.py:131-155; the tb_dict values are detached device tensors (nothing is read back)"""
        self._training_setup()
        r = self.forward_ret_dict
        if not r or "point_cls_labels" not in r:
            raise KeyError("PointHeadSimple.get_loss follows a training-mode forward (no point_cls_labels)")
        preds = r["point_cls_preds"].view(-1, self.num_class)
        labels = r["point_cls_labels"].view(-1)
        if point_head_fused():
            loss, pos_num = ops.point_cls_loss(preds, labels, self.point_cls_weight)
        else:
            loss, pos_num = composed_point_cls_loss(preds, labels, self.point_cls_weight)
        point_loss_cls = loss[0]
        tb_dict = {} if tb_dict is None else tb_dict
        tb_dict.update(point_loss_cls=point_loss_cls.detach(), point_pos_num=pos_num[0].detach())
        return point_loss_cls, tb_dict

    def get_loss(self, tb_dict=None):
        """-> (point_loss, tb_dict) with point_loss_cls and point_pos_num"""
        tb_dict = {} if tb_dict is None else tb_dict
        point_loss_cls, tb_dict_1 = self.get_cls_layer_loss()
        tb_dict.update(tb_dict_1)
        return point_loss_cls, tb_dict


@MAP_TO_BEV.register_module
class HeightCompression(nn.Module):
    """VR/pcdet/models/backbones_2d/map_to_bev/height_compression.py: the sparse tensor's dense [B, C, D, H, W] as [B, C*D, H, W]."""

    def __init__(self, model_cfg, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_bev_features = _get(model_cfg, "NUM_BEV_FEATURES")

    def forward(self, batch_dict):
        spatial_features = batch_dict["encoded_spconv_tensor"].dense()
        N, C, D, H, W = spatial_features.shape
        batch_dict["spatial_features"] = spatial_features.reshape(N, C * D, H, W)
        batch_dict["spatial_features_stride"] = batch_dict["encoded_spconv_tensor_stride"]
        return batch_dict


def _bn(c):
    return nn.BatchNorm2d(c, eps=1e-3, momentum=0.01)


@BACKBONES_2D.register_module
class BaseBEVBackbone(nn.Module):
    """VR/pcdet/models/backbones_2d/base_bev_backbone.py in plain torch: parameters blocks.{i}.{j} / deblocks.{i}.{j}."""

    def __init__(self, model_cfg, input_channels):
        super().__init__()
        self.model_cfg = model_cfg
        layer_nums = list(_get(model_cfg, "LAYER_NUMS") or [])
        layer_strides = list(_get(model_cfg, "LAYER_STRIDES") or [])
        num_filters = list(_get(model_cfg, "NUM_FILTERS") or [])
        upsample_strides = list(_get(model_cfg, "UPSAMPLE_STRIDES") or [])
        num_upsample_filters = list(_get(model_cfg, "NUM_UPSAMPLE_FILTERS") or [])
        assert len(layer_nums) == len(layer_strides) == len(num_filters)
        assert len(upsample_strides) == len(num_upsample_filters)
        c_in_list = [input_channels] + num_filters[:-1]
        self.blocks, self.deblocks = nn.ModuleList(), nn.ModuleList()
        for idx, (n, stride, width) in enumerate(zip(layer_nums, layer_strides, num_filters)):
            layers = [nn.ZeroPad2d(1), nn.Conv2d(c_in_list[idx], width, kernel_size=3, stride=stride, padding=0, bias=False),
                      _bn(width), nn.ReLU()]
            for _ in range(n):
                layers.extend([nn.Conv2d(width, width, kernel_size=3, padding=1, bias=False), _bn(width), nn.ReLU()])
            self.blocks.append(nn.Sequential(*layers))
            if upsample_strides:
                up, up_width = upsample_strides[idx], num_upsample_filters[idx]
                if up >= 1:
                    conv = nn.ConvTranspose2d(width, up_width, up, stride=up, bias=False)
                else:
                    down = int(np.round(1 / up))
                    conv = nn.Conv2d(width, up_width, down, stride=down, bias=False)
                self.deblocks.append(nn.Sequential(conv, _bn(up_width), nn.ReLU()))
        c_in = sum(num_upsample_filters)
        if len(upsample_strides) > len(layer_nums):
            self.deblocks.append(nn.Sequential(nn.ConvTranspose2d(c_in, c_in, upsample_strides[-1], stride=upsample_strides[-1],
                                                                  bias=False), _bn(c_in), nn.ReLU()))
        self.num_bev_features = c_in

    def forward(self, data_dict):
        spatial_features = data_dict["spatial_features"]
        ups, x = [], spatial_features
        for i in range(len(self.blocks)):
            x = self.blocks[i](x)
            ups.append(self.deblocks[i](x) if len(self.deblocks) > 0 else x)
        if len(ups) > 1:
            x = torch.cat(ups, dim=1)
        elif len(ups) == 1:
            x = ups[0]
        if len(self.deblocks) > len(self.blocks):
            x = self.deblocks[-1](x)
        data_dict["spatial_features_2d"] = x
        return data_dict
