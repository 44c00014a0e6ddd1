"""VoxelRCNNHead (VR/pcdet/models/roi_heads/voxelrcnn_head.py over roi_head_template.py): the proposal layer, RoI grid
pooling over the backbone's sparse levels, the refinement layers, the decoding of their outputs and, for training, the
proposal targets and the RCNN losses.  The reference's constructor signature, config keys and parameter names, so its
checkpoints load.

Training is `forward_train` + `get_loss`, two formulations chosen per call by DF3D_ROI_LOSS_FUSED
(default 1): fused -- ops.roi_targets and ops.rcnn_loss (csrc/roiloss.hip), one launch for the targets of all frames, two for
the three losses, one for their gradients, no host round trip; composed -- the reference's per-frame formulation in torch
(`composed_roi_targets`, `composed_rcnn_losses`), the A/B baseline and a second implementation.  Both sample as a function
of the draws u_fg / u_slot that ProposalTargetLayer makes with torch.rand; the source of the random numbers is the one
intended difference from the reference.  `forward` itself is unchanged and still serves inference.

`forward` reads `batch_dict['rois']` where the caller supplies them; otherwise `proposal_layer` makes them from the dense
head's outputs and NMS_CONFIG['TEST'] -- from the head maps and anchor tables of AnchorHeadSingle's fused mode in one call
with no host round trip (ops.anchor_proposals, csrc/proposals.hip), or from `batch_cls_preds` /
`batch_box_preds` with the reference's per-frame loop on iou3d_nms.nms_gpu (composed mode, DF3D_VR_TAIL_FUSED=0).  It stores
`rcnn_cls` / `rcnn_reg` and, in eval, `batch_cls_preds`, `batch_box_preds` and `cls_preds_normalized=False`.

`roi_grid_pool` never builds the reference's dense voxel-to-point tensor (`generate_voxel2pinds`: B * Z * Y * X int32 per
level and step): every source level is looked up through its occupancy directory, the one its sparse tensor already
carries where a convolution built it.

`RoIHeadTemplate` holds what is not specific to that pooling -- the grid points, the proposal layer, the decoding, the
proposal targets and the RCNN losses -- for VoxelRCNNHead and for PVRCNNHead (VR/pcdet/models/roi_heads/pvrcnn_head.py,
DESIGN section 7.16), which pools the keypoints of VoxelSetAbstraction through one StackSAModuleMSG instead."""
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import iou3d_nms, ops
from .dense_heads import residual_decode, tail_fused
from .pointnet2_stack import NeighborVoxelSAModuleMSG, build_local_aggregation_module, frame_counts
from .registry import ROI_HEADS

BOX_CODE_SIZE = 7          # ResidualCoder (VR/pcdet/utils/box_coder_utils.py): x, y, z, dx, dy, dz, heading


def _get(cfg, key, default=None):
    """config nodes are EasyDicts in pcdet and plain dicts here"""
    if isinstance(cfg, dict):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


def _need(cfg, key):
    v = _get(cfg, key)
    if v is None:
        raise KeyError("VoxelRCNNHead: the config has no %s" % key)
    return v


def rotate_points_along_z(points, angle):
    """VR/pcdet/utils/common_utils.py:rotate_points_along_z: points [B, N, 3 + C], angle [B]."""
    cosa, sina = torch.cos(angle), torch.sin(angle)
    zeros, ones = angle.new_zeros(points.shape[0]), angle.new_ones(points.shape[0])
    rot = torch.stack((cosa, sina, zeros, -sina, cosa, zeros, zeros, zeros, ones), dim=1).view(-1, 3, 3).to(points.dtype)
    points_rot = torch.matmul(points[:, :, 0:3], rot)
    return torch.cat((points_rot, points[:, :, 3:]), dim=-1)


def get_voxel_centers(voxel_coords, downsample_times, voxel_size, point_cloud_range):
    """VR/pcdet/utils/common_utils.py:get_voxel_centers: voxel_coords [N, 3] (z, y, x) -> centres [N, 3] (x, y, z)."""
    centers = voxel_coords[:, 0:3].flip(1).float()            # (a list index would be copied to the device on every call)
    size = ops.device_constant([float(v) for v in voxel_size], torch.float32, centers.device) * downsample_times
    low = ops.device_constant([float(v) for v in point_cloud_range[0:3]], torch.float32, centers.device)
    return (centers + 0.5) * size + low


def _fc_stack(pre_channel, widths, dp_ratio, inplace=False):
    layers = []
    for k, width in enumerate(widths):
        layers.extend([nn.Linear(pre_channel, width, bias=False), nn.BatchNorm1d(width), nn.ReLU(inplace=True) if inplace else nn.ReLU()])
        pre_channel = width
        if k != len(widths) - 1 and dp_ratio > 0:
            layers.append(nn.Dropout(dp_ratio))
    return nn.Sequential(*layers), pre_channel


def roi_loss_fused():
    """DF3D_ROI_LOSS_FUSED, read per call (default: fused)"""
    return os.environ.get("DF3D_ROI_LOSS_FUSED", "1") != "0"


# ---- the composed formulation: the reference's per-frame steps in torch
def _footprint(b):
    hx, hy = b[:, 3] / 2, b[:, 4] / 2
    px, py = torch.stack([-hx, hx, hx, -hx], 1), torch.stack([-hy, -hy, hy, hy], 1)
    c, s = torch.cos(b[:, 6])[:, None], torch.sin(b[:, 6])[:, None]
    return torch.stack([px * c - py * s + b[:, 0:1], px * s + py * c + b[:, 1:2]], -1)


def _cross2(u, v):
    return u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]


def _strictly_inside(pts, b):
    d = pts - b[:, None, 0:2]
    c, s = torch.cos(b[:, 6])[:, None], torch.sin(b[:, 6])[:, None]
    lx, ly = d[..., 0] * c + d[..., 1] * s, -d[..., 0] * s + d[..., 1] * c
    return (lx.abs() < b[:, None, 3] / 2) & (ly.abs() < b[:, None, 4] / 2)


def boxes_iou3d_lidar(boxes_a, boxes_b):
    """pcdet's boxes_iou3d_gpu (VR/pcdet/ops/iou3d_nms/iou3d_nms_utils.py:48-80) for boxes (x, y, z, dx, dy, dz, heading) in the
    LiDAR convention, composed from torch ops in float64 on the boxes' device: [N, 7], [M, 7] -> [N, M] float32.  The footprint
    overlap is the polygon of the proper edge crossings and of the corners of one box strictly inside the other, ordered about
    its centroid.  (ops.boxes_bev_pairwise is the float32 kernel with a containment margin of 1e-2 m, which moves the IoU of
    a pedestrian-sized box by up to 1e-2: good for NMS, no baseline for a sampler whose lists are compared index by index.)"""
    a, b = boxes_a[:, :7].double(), boxes_b[:, :7].double()
    n, m = a.shape[0], b.shape[0]
    A, Bc = _footprint(a)[:, None].expand(n, m, 4, 2).reshape(-1, 4, 2), _footprint(b)[None].expand(n, m, 4, 2).reshape(-1, 4, 2)
    ab, bb = a[:, None].expand(n, m, 7).reshape(-1, 7), b[None].expand(n, m, 7).reshape(-1, 7)
    p, r = A[:, :, None, :], (torch.roll(A, -1, 1) - A)[:, :, None, :]
    q, s = Bc[:, None, :, :], (torch.roll(Bc, -1, 1) - Bc)[:, None, :, :]
    rxs = _cross2(r, s)
    safe = torch.where(rxs == 0, torch.ones_like(rxs), rxs)
    t, u = _cross2(q - p, s) / safe, _cross2(q - p, r) / safe
    hit = (rxs != 0) & (t > 0) & (t < 1) & (u > 0) & (u < 1)
    pts = torch.cat([(p + t[..., None] * r).reshape(-1, 16, 2), Bc, A], 1)
    ok = torch.cat([hit.reshape(-1, 16), _strictly_inside(Bc, ab), _strictly_inside(A, bb)], 1)
    cnt = ok.sum(1)
    ctr = (pts * ok[..., None]).sum(1) / cnt.clamp(min=1)[:, None]
    rel = pts - ctr[:, None, :]
    ang = torch.where(ok, torch.atan2(rel[..., 1], rel[..., 0]), torch.full_like(rel[..., 0], float("inf")))
    order = torch.sort(ang, dim=1, stable=True)[1]
    rel = torch.gather(rel, 1, order[..., None].expand(-1, -1, 2))
    good = torch.gather(ok, 1, order)
    rel = torch.where(good[..., None], rel, rel[:, 0:1, :])          # the unused slots repeat the first vertex: no area
    nxt = torch.roll(rel, -1, 1)
    area = 0.5 * (rel[..., 0] * nxt[..., 1] - nxt[..., 0] * rel[..., 1]).sum(1).abs()
    bev = torch.where(cnt >= 3, area, torch.zeros_like(area)).view(n, m)
    h = torch.clamp(torch.min((a[:, 2] + a[:, 5] / 2)[:, None], (b[:, 2] + b[:, 5] / 2)[None]) -
                    torch.max((a[:, 2] - a[:, 5] / 2)[:, None], (b[:, 2] - b[:, 5] / 2)[None]), min=0)
    o3 = bev * h
    vol_a, vol_b = (a[:, 3] * a[:, 4] * a[:, 5])[:, None], (b[:, 3] * b[:, 4] * b[:, 5])[None]
    return (o3 / torch.clamp(vol_a + vol_b - o3, min=1e-6)).float()


def composed_roi_targets(rois, roi_scores, roi_labels, gt_boxes, u_fg, u_slot, cfg):
    """ops.roi_targets in the reference's formulation (proposal_target_layer.py, roi_head_template.py:104-134): a Python loop
    over frames, nonzero() compactions and counts read back to the host; the three host random sources are the draws."""
    B, R = rois.shape[:2]
    M = int(_need(cfg, "ROI_PER_IMAGE"))
    score = _need(cfg, "CLS_SCORE_TYPE")
    if score not in ops.ROI_SCORE_TYPES:
        raise NotImplementedError("ProposalTargetLayer: CLS_SCORE_TYPE %r is not supported (%s)" % (score, ", ".join(sorted(ops.ROI_SCORE_TYPES))))
    if rois.shape[-1] != BOX_CODE_SIZE:
        raise NotImplementedError("ProposalTargetLayer: box codes wider than 7 are not supported (got %d)" % rois.shape[-1])
    reg_fg, cls_fg, cls_bg, lo = [float(_need(cfg, k)) for k in ("REG_FG_THRESH", "CLS_FG_THRESH", "CLS_BG_THRESH", "CLS_BG_THRESH_LO")]
    fg_per_image = int(np.round(float(_need(cfg, "FG_RATIO")) * M))
    inds, asg_all, iou_all = [], [], []
    counts = torch.zeros((B, 3), dtype=torch.int32)
    for b in range(B):
        cur_gt = gt_boxes[b]
        k = cur_gt.shape[0] - 1
        while k > 0 and cur_gt[k].sum() == 0:
            k -= 1
        cur_gt = cur_gt[:k + 1]
        iou = boxes_iou3d_lidar(rois[b], cur_gt[:, 0:7])
        if _get(cfg, "SAMPLE_ROI_BY_EACH_CLASS", False):
            same = cur_gt[None, :, 7].long() == roi_labels[b][:, None]
            best, asg = torch.where(same, iou, torch.full_like(iou, -1.0)).max(dim=1)
            none = best < 0
            best, asg = torch.where(none, torch.zeros_like(best), best), torch.where(none, torch.zeros_like(asg), asg)
        else:
            best, asg = iou.max(dim=1)
        fg = (best >= min(reg_fg, cls_fg)).nonzero().view(-1)
        easy = (best < lo).nonzero().view(-1)
        hard = ((best < reg_fg) & (best >= lo)).nonzero().view(-1)
        counts[b, 0], counts[b, 1], counts[b, 2] = fg.numel(), hard.numel(), easy.numel()
        u = u_slot[b].double()
        pick = lambda lst, lo_s, hi_s: lst[torch.floor(u[lo_s:hi_s] * lst.numel()).long()]

        def background(F_):
            if hard.numel() > 0 and easy.numel() > 0:
                n_hard = min(int((M - F_) * float(_need(cfg, "HARD_BG_RATIO"))), hard.numel())
                return torch.cat([pick(hard, F_, F_ + n_hard), pick(easy, F_ + n_hard, M)])
            return pick(hard if hard.numel() > 0 else easy, F_, M)

        if fg.numel() > 0 and hard.numel() + easy.numel() > 0:
            F_ = min(fg_per_image, fg.numel())
            order = torch.sort(u_fg[b, :fg.numel()], stable=True)[1]
            sel = torch.cat([fg[order[:F_]], background(F_)])
        elif fg.numel() > 0:
            sel = pick(fg, 0, M)
        elif hard.numel() + easy.numel() > 0:
            sel = background(0)
        else:
            raise NotImplementedError("ProposalTargetLayer: frame %d has neither foreground nor background RoIs (NaN overlaps)" % b)
        inds.append(sel)
        asg_all.append(asg)
        iou_all.append(best)
    inds = torch.stack(inds)
    bi = torch.arange(B, device=rois.device)[:, None]
    s_rois, s_iou = rois[bi, inds], torch.stack(iou_all)[bi, inds]
    src = gt_boxes[bi, torch.stack(asg_all)[bi, inds]]
    if score == "cls":
        labels = (s_iou > cls_fg).float()
        labels[(s_iou > cls_bg) & (s_iou < cls_fg)] = -1
    else:
        fg_mask, bg_mask = s_iou > cls_fg, s_iou < cls_bg
        interval = (fg_mask == 0) & (bg_mask == 0)
        labels = (fg_mask > 0).float()
        labels[interval] = (s_iou[interval] - cls_bg) / (cls_fg - cls_bg)
    # canonical transformation
    gt_of_rois = src.clone()
    roi_ry = s_rois[:, :, 6] % (2 * np.pi)
    gt_of_rois[:, :, 0:3] = gt_of_rois[:, :, 0:3] - s_rois[:, :, 0:3]
    gt_of_rois[:, :, 6] = gt_of_rois[:, :, 6] - roi_ry
    gt_of_rois = rotate_points_along_z(gt_of_rois.view(-1, 1, gt_of_rois.shape[-1]), -roi_ry.view(-1)).view(B, -1, gt_of_rois.shape[-1])
    heading = gt_of_rois[:, :, 6] % (2 * np.pi)
    opposite = (heading > np.pi * 0.5) & (heading < np.pi * 1.5)
    heading[opposite] = (heading[opposite] + np.pi) % (2 * np.pi)
    flag = heading > np.pi
    heading[flag] = heading[flag] - np.pi * 2
    gt_of_rois[:, :, 6] = torch.clamp(heading, min=-np.pi / 2, max=np.pi / 2)
    return {"rois": s_rois, "roi_labels": roi_labels[bi, inds], "roi_scores": roi_scores[bi, inds], "gt_iou_of_rois": s_iou,
            "roi_inds": inds.to(torch.int32), "gt_of_rois_src": src, "gt_of_rois": gt_of_rois,
            "reg_valid_mask": (s_iou > reg_fg).to(torch.int32), "rcnn_cls_labels": labels, "counts": counts.to(rois.device)}


def boxes_to_corners_3d(boxes3d):
    """VR/pcdet/utils/box_utils.py:boxes_to_corners_3d: [N, 7] -> [N, 8, 3]"""
    template = boxes3d.new_tensor(([1, 1, -1], [1, -1, -1], [-1, -1, -1], [-1, 1, -1], [1, 1, 1], [1, -1, 1], [-1, -1, 1], [-1, 1, 1])) / 2
    corners3d = boxes3d[:, None, 3:6].repeat(1, 8, 1) * template[None, :, :]
    corners3d = rotate_points_along_z(corners3d.view(-1, 8, 3), boxes3d[:, 6]).view(-1, 8, 3)
    return corners3d + boxes3d[:, None, 0:3]


def composed_rcnn_losses(rcnn_cls, rcnn_reg, targets, spec):
    """ops.rcnn_loss in the reference's formulation (roi_head_template.py:136-218, utils/loss_utils.py:75-136, 209-232) in torch,
    on any device: -> [3] = rcnn_loss_cls, rcnn_loss_reg, rcnn_loss_corner."""
    if rcnn_cls.dim() != 2 or rcnn_cls.shape[1] != 1:
        raise NotImplementedError("rcnn_loss: rcnn_cls must be [N, 1] (BinaryCrossEntropy on one logit)")
    if rcnn_reg.shape[-1] != BOX_CODE_SIZE:
        raise NotImplementedError("rcnn_loss: box codes wider than 7 are not supported (got %d)" % rcnn_reg.shape[-1])
    n = rcnn_cls.shape[0]
    labels = targets["rcnn_cls_labels"].reshape(-1).float()
    # (binary_cross_entropy refuses the -1 of the ignored rows; they are masked out below, as in the reference)
    batch_loss_cls = F.binary_cross_entropy(torch.sigmoid(rcnn_cls.reshape(-1)), labels.clamp(0, 1), reduction="none")
    cls_valid_mask = (labels >= 0).float()
    loss_cls = (batch_loss_cls * cls_valid_mask).sum() / torch.clamp(cls_valid_mask.sum(), min=1.0) * spec.cls_weight
    fg_mask = targets["reg_valid_mask"].reshape(-1) > 0
    fg_sum = fg_mask.long().sum().item()
    roi_boxes3d = targets["rois"].reshape(n, BOX_CODE_SIZE)
    gt_ct = targets["gt_of_rois"].reshape(n, -1)[:, 0:BOX_CODE_SIZE]
    gt_src = targets["gt_of_rois_src"].reshape(n, -1)[:, 0:BOX_CODE_SIZE]
    rois_anchor = roi_boxes3d.clone().detach()
    rois_anchor[:, 0:3] = 0
    rois_anchor[:, 6] = 0
    dxa, dya, dza = [torch.clamp_min(rois_anchor[:, k], 1e-5) for k in (3, 4, 5)]
    dxg, dyg, dzg = [torch.clamp_min(gt_ct[:, k], 1e-5) for k in (3, 4, 5)]
    diagonal = torch.sqrt(dxa ** 2 + dya ** 2)
    reg_targets = torch.stack([gt_ct[:, 0] / diagonal, gt_ct[:, 1] / diagonal, gt_ct[:, 2] / dza, torch.log(dxg / dxa), torch.log(dyg / dya),
                               torch.log(dzg / dza), gt_ct[:, 6]], dim=-1)
    reg_targets = torch.where(torch.isnan(reg_targets), rcnn_reg.detach(), reg_targets)
    diff = (rcnn_reg - reg_targets) * rcnn_reg.new_tensor(spec.code_weights)[None]
    mag = diff.abs()
    loss = torch.where(mag < spec.beta, 0.5 * mag ** 2 / spec.beta, mag - 0.5 * spec.beta) if spec.beta >= 1e-5 else mag
    loss_reg = (loss * fg_mask[:, None].float()).sum() / max(fg_sum, 1) * spec.reg_weight
    loss_corner = loss_reg.new_zeros(())
    if spec.corner_loss and fg_sum > 0:
        fg_rcnn_reg, fg_rois = rcnn_reg[fg_mask], roi_boxes3d[fg_mask]
        batch_anchors = fg_rois.clone().detach()
        batch_anchors[:, 0:3] = 0
        rcnn_boxes3d = residual_decode(fg_rcnn_reg, batch_anchors)
        rcnn_boxes3d = rotate_points_along_z(rcnn_boxes3d.unsqueeze(dim=1), fg_rois[:, 6]).squeeze(dim=1)
        rcnn_boxes3d = torch.cat([rcnn_boxes3d[:, 0:3] + fg_rois[:, 0:3], rcnn_boxes3d[:, 3:]], dim=-1)
        gt = gt_src[fg_mask]
        pred_corners = boxes_to_corners_3d(rcnn_boxes3d)
        gt_flip = torch.cat([gt[:, 0:6], gt[:, 6:7] + np.pi], dim=-1)
        corner_dist = torch.min(torch.norm(pred_corners - boxes_to_corners_3d(gt), dim=2),
                                torch.norm(pred_corners - boxes_to_corners_3d(gt_flip), dim=2))
        corner_loss = torch.where(corner_dist < 1.0, 0.5 * corner_dist ** 2, corner_dist - 0.5)
        loss_corner = corner_loss.mean(dim=1).mean() * spec.corner_weight
    return torch.stack([loss_cls, loss_reg, loss_corner])


class ProposalTargetLayer(nn.Module):
    """VR/pcdet/models/roi_heads/target_assigner/proposal_target_layer.py with the reference's config keys.  The sampling is a
    function of two arrays of uniform draws: u_fg [B, R] orders the foreground RoIs, u_slot [B, M] picks
    the element of a list for a slot.  `forward` makes them with torch.rand on the RoIs' device from `generator` (an optional
    torch.Generator on that device) unless the caller passes them."""

    def __init__(self, roi_sampler_cfg, generator=None):
        super().__init__()
        self.roi_sampler_cfg = roi_sampler_cfg
        self.generator = generator
        score = _need(roi_sampler_cfg, "CLS_SCORE_TYPE")
        if score not in ops.ROI_SCORE_TYPES:
            raise NotImplementedError("ProposalTargetLayer: CLS_SCORE_TYPE %r is not supported (%s)"
                                      % (score, ", ".join(sorted(ops.ROI_SCORE_TYPES))))

    def draws(self, batch_size, num_rois, device):
        m = int(_need(self.roi_sampler_cfg, "ROI_PER_IMAGE"))
        u_fg = torch.rand((batch_size, num_rois), generator=self.generator, device=device, dtype=torch.float32)
        u_slot = torch.rand((batch_size, m), generator=self.generator, device=device, dtype=torch.float32)
        return u_fg, u_slot

    @torch.no_grad()
    def forward(self, batch_dict, u_fg=None, u_slot=None):
        """batch_dict: rois [B, R, 7], roi_scores [B, R], roi_labels [B, R], gt_boxes [B, G, 8] -> the targets dict of
        RoIHeadTemplate.assign_targets (gt_of_rois already canonical, gt_of_rois_src the assigned rows), on the device."""
        rois, gt_boxes = batch_dict["rois"], batch_dict["gt_boxes"]
        if rois.dim() != 3 or rois.shape[-1] != BOX_CODE_SIZE or gt_boxes.shape[-1] != BOX_CODE_SIZE + 1:
            raise NotImplementedError("ProposalTargetLayer: box codes wider than 7 are not supported (rois %s, gt_boxes %s)"
                                      % (tuple(rois.shape), tuple(gt_boxes.shape)))
        B, R = rois.shape[:2]
        if R > ops.ROI_MAX_ROIS or int(_need(self.roi_sampler_cfg, "ROI_PER_IMAGE")) > ops.ROI_MAX_SAMPLES or gt_boxes.shape[1] > ops.ROI_MAX_GT:
            raise NotImplementedError("ProposalTargetLayer: %d RoIs, ROI_PER_IMAGE = %d or %d ground-truth rows exceed the caps %d / %d / %d"
                                      % (R, int(_need(self.roi_sampler_cfg, "ROI_PER_IMAGE")), gt_boxes.shape[1], ops.ROI_MAX_ROIS,
                                         ops.ROI_MAX_SAMPLES, ops.ROI_MAX_GT))
        if (u_fg is None) != (u_slot is None):
            raise ValueError("ProposalTargetLayer: pass both u_fg and u_slot, or neither")
        if u_fg is None:
            u_fg, u_slot = self.draws(B, R, rois.device)
        rois, gt_boxes = rois.float().contiguous(), gt_boxes.float().contiguous()
        scores, labels = batch_dict["roi_scores"].float().contiguous(), batch_dict["roi_labels"].long().contiguous()
        if roi_loss_fused():
            return ops.roi_targets(rois, scores, labels, gt_boxes, u_fg.contiguous(), u_slot.contiguous(), self.roi_sampler_cfg)
        return composed_roi_targets(rois, scores, labels, gt_boxes, u_fg, u_slot, self.roi_sampler_cfg)


class RoIHeadTemplate(nn.Module):
    """What the RoI heads of this tree share (VR/pcdet/models/roi_heads/roi_head_template.py): the grid points of a RoI, the
    proposal layer, the decoding of the refinement outputs, the proposal targets and the RCNN losses.  A head supplies
    `roi_grid_pool(batch_dict)` and `rcnn_outputs(batch_dict) -> (rcnn_cls [N, num_class], rcnn_reg [N, 7 * num_class])`."""

    # ---- grid points
    @staticmethod
    def get_dense_grid_points(rois, batch_size_rcnn, grid_size):
        faked_features = rois.new_ones((grid_size, grid_size, grid_size))
        dense_idx = faked_features.nonzero()                                   # [g^3, 3] (x_idx, y_idx, z_idx)
        dense_idx = dense_idx.repeat(batch_size_rcnn, 1, 1).float()
        local_roi_size = rois.view(batch_size_rcnn, -1)[:, 3:6]
        return (dense_idx + 0.5) / grid_size * local_roi_size.unsqueeze(dim=1) - (local_roi_size.unsqueeze(dim=1) / 2)

    def get_global_grid_points_of_roi(self, rois, grid_size):
        rois = rois.view(-1, rois.shape[-1])
        batch_size_rcnn = rois.shape[0]
        local_roi_grid_points = self.get_dense_grid_points(rois, batch_size_rcnn, grid_size)
        global_roi_grid_points = rotate_points_along_z(local_roi_grid_points.clone(), rois[:, 6]).squeeze(dim=1)
        global_roi_grid_points = global_roi_grid_points + rois[:, 0:3].clone().unsqueeze(dim=1)
        return global_roi_grid_points, local_roi_grid_points

    # ---- proposals and decoding
    @staticmethod
    def check_nms_config(nms_config, what):
        """The limits of both modes, each refused by name (never a wrong result)."""
        if _get(nms_config, "MULTI_CLASSES_NMS", False):
            raise NotImplementedError("%s: MULTI_CLASSES_NMS is not supported" % what)
        if _get(nms_config, "NMS_TYPE", "nms_gpu") != "nms_gpu":
            raise NotImplementedError("%s: NMS_TYPE %s is not supported (nms_gpu only)" % (what, _get(nms_config, "NMS_TYPE")))
        pre = int(_need(nms_config, "NMS_PRE_MAXSIZE"))
        if pre > ops.TAIL_MAX_CANDIDATES:
            raise NotImplementedError("%s: NMS_PRE_MAXSIZE = %d exceeds %d, the cap of the top-k select and the NMS "
                                      "(the TRAIN value of the shipped configs is not supported)" % (what, pre, ops.TAIL_MAX_CANDIDATES))
        return pre, int(_need(nms_config, "NMS_POST_MAXSIZE")), float(_need(nms_config, "NMS_THRESH"))

    @torch.no_grad()
    def proposal_layer(self, batch_dict, nms_config):
        """roi_head_template.py:45-102: rois [B, POST, 7], roi_scores [B, POST] (raw logits), roi_labels [B, POST] (1-based;
        unused slots hold zeros and label 1, as the reference leaves them)."""
        if batch_dict.get("rois", None) is not None:
            return batch_dict
        pre, post, thresh = self.check_nms_config(nms_config, "%s.proposal_layer" % type(self).__name__)
        batch_size = batch_dict["batch_size"]
        if "dense_cls_rows" in batch_dict:                                    # AnchorHeadSingle, fused mode
            meta = batch_dict["dense_anchor_tables"]
            tables = meta["tables"]
            x_shifts, y_shifts = tables.on(batch_dict["dense_cls_rows"].device)
            rois, roi_scores, roi_labels, num = ops.anchor_proposals(
                batch_dict["dense_cls_rows"], batch_dict["dense_box_rows"], batch_dict["dense_dir_rows"], x_shifts, y_shifts,
                batch_size, meta["H"], meta["W"], meta["num_class"], tables.anchor_set, tables.table.tolist(), thresh, pre, post,
                dir_offset=meta["dir_offset"], dir_limit_offset=meta["dir_limit_offset"])
            batch_dict["roi_counts"] = num
            has_class_labels = meta["num_class"] > 1
        else:                                                                  # the reference's per-frame loop
            if batch_dict.get("batch_index", None) is not None:
                raise NotImplementedError("%s.proposal_layer: stacked predictions (batch_index) are not supported" % type(self).__name__)
            batch_box_preds, batch_cls_preds = batch_dict["batch_box_preds"], batch_dict["batch_cls_preds"]
            rois = batch_box_preds.new_zeros((batch_size, post, batch_box_preds.shape[-1]))
            roi_scores = batch_box_preds.new_zeros((batch_size, post))
            roi_labels = batch_box_preds.new_zeros((batch_size, post), dtype=torch.long)
            for index in range(batch_size):
                box_preds = batch_box_preds[index]
                cur_roi_scores, cur_roi_labels = torch.max(batch_cls_preds[index], dim=1)
                selected = class_agnostic_nms(cur_roi_scores, box_preds, pre, post, thresh)
                rois[index, :len(selected), :] = box_preds[selected]
                roi_scores[index, :len(selected)] = cur_roi_scores[selected]
                roi_labels[index, :len(selected)] = cur_roi_labels[selected]
            roi_labels = roi_labels + 1
            has_class_labels = batch_cls_preds.shape[-1] > 1
        batch_dict["rois"] = rois
        batch_dict["roi_scores"] = roi_scores
        batch_dict["roi_labels"] = roi_labels
        batch_dict["has_class_labels"] = has_class_labels
        return batch_dict

    def generate_predicted_boxes(self, batch_size, rois, cls_preds, box_preds):
        """roi_head_template.py:233-261 in torch: decode against the RoI with its centre zeroed, rotate about z by the RoI
        heading, add the RoI centre."""
        batch_cls_preds = cls_preds.view(batch_size, -1, cls_preds.shape[-1])
        batch_box_preds = box_preds.view(batch_size, -1, BOX_CODE_SIZE)
        roi_ry = rois[:, :, 6].reshape(-1)
        roi_xyz = rois[:, :, 0:3].reshape(-1, 3)
        local_rois = rois.clone().detach()
        local_rois[:, :, 0:3] = 0
        batch_box_preds = residual_decode(batch_box_preds, local_rois).view(-1, BOX_CODE_SIZE)
        batch_box_preds = rotate_points_along_z(batch_box_preds.unsqueeze(dim=1), roi_ry).squeeze(dim=1)
        batch_box_preds[:, 0:3] += roi_xyz
        return batch_cls_preds, batch_box_preds.view(batch_size, -1, BOX_CODE_SIZE)

    # ---- training
    def _training_setup(self):
        """the target layer and the loss configuration, made on first use; every limit is refused by name"""
        if getattr(self, "loss_spec", None) is not None:
            return
        loss_cfg = _need(self.model_cfg, "LOSS_CONFIG")
        if _get(loss_cfg, "CLS_LOSS", "BinaryCrossEntropy") != "BinaryCrossEntropy":
            raise NotImplementedError("%s: CLS_LOSS %s is not supported (BinaryCrossEntropy only)" % (type(self).__name__, _get(loss_cfg, "CLS_LOSS")))
        if _get(loss_cfg, "REG_LOSS", "smooth-l1") != "smooth-l1":
            raise NotImplementedError("%s: REG_LOSS %s is not supported (smooth-l1 only)" % (type(self).__name__, _get(loss_cfg, "REG_LOSS")))
        if self.num_class != 1:
            raise NotImplementedError("%s: the RCNN losses need CLASS_AGNOSTIC (one logit and one box per RoI)" % type(self).__name__)
        w = _need(loss_cfg, "LOSS_WEIGHTS")
        spec = ops.RcnnLossSpec(_need(w, "rcnn_cls_weight"), _need(w, "rcnn_reg_weight"), _get(w, "rcnn_corner_weight", 0.0),
                                list(_need(w, "code_weights")), corner_loss=bool(_get(loss_cfg, "CORNER_LOSS_REGULARIZATION", False)))
        if getattr(self, "proposal_target_layer", None) is None:
            self.proposal_target_layer = ProposalTargetLayer(_need(self.model_cfg, "TARGET_CONFIG"))
        self.loss_spec = spec

    def assign_targets(self, batch_dict, u_fg=None, u_slot=None):
        """roi_head_template.py:104-134: batch_dict with rois, roi_scores, roi_labels, gt_boxes -> the targets dict
        (ProposalTargetLayer.forward; the draws are made by the layer unless given)."""
        self._training_setup()
        return self.proposal_target_layer(batch_dict, u_fg=u_fg, u_slot=u_slot)

    def forward_train(self, batch_dict, u_fg=None, u_slot=None):
        """The reference's training-mode forward: RoIs as `forward` takes them (given, or made by proposal_layer from
        NMS_CONFIG['TRAIN'] inside the candidate cap), sampled; batch_dict['rois'] / ['roi_labels'] replaced by the sampled
        ones; pooling and the FC layers; `forward_ret_dict` keeps the targets with rcnn_cls and rcnn_reg for get_loss."""
        self._training_setup()
        if "rois" not in batch_dict:
            nms_cfg = _get(self.model_cfg, "NMS_CONFIG")
            if nms_cfg is None or ("dense_cls_rows" not in batch_dict and "batch_box_preds" not in batch_dict):
                raise KeyError("%s.forward_train needs batch_dict['rois'] [B, num_rois, 7], or a dense head's outputs "
                               "(AnchorHeadSingle) and the config's NMS_CONFIG to make them from" % type(self).__name__)
            self.proposal_layer(batch_dict, _need(nms_cfg, "TRAIN"))
        rois = batch_dict["rois"]
        if rois.shape[-1] != BOX_CODE_SIZE:
            raise NotImplementedError("%s.forward_train: box codes wider than 7 are not supported (rois %s)" % (type(self).__name__, tuple(rois.shape)))
        if "gt_boxes" not in batch_dict:
            raise KeyError("%s.forward_train needs batch_dict['gt_boxes'] [B, G, 8]" % type(self).__name__)
        if batch_dict.get("roi_scores", None) is None:
            batch_dict["roi_scores"] = rois.new_zeros(rois.shape[:2])
        if batch_dict.get("roi_labels", None) is None:
            batch_dict["roi_labels"] = torch.ones(rois.shape[:2], dtype=torch.long, device=rois.device)
        targets_dict = self.assign_targets(batch_dict, u_fg=u_fg, u_slot=u_slot)
        batch_dict["rois"] = targets_dict["rois"]
        batch_dict["roi_labels"] = targets_dict["roi_labels"]
        targets_dict["rcnn_cls"], targets_dict["rcnn_reg"] = self.rcnn_outputs(batch_dict)
        batch_dict["rcnn_cls"], batch_dict["rcnn_reg"] = targets_dict["rcnn_cls"], targets_dict["rcnn_reg"]
        self.forward_ret_dict = targets_dict
        return batch_dict

    def get_loss(self, tb_dict=None):
        """roi_head_template.py:220-231 -> (rcnn_loss, tb_dict) with rcnn_loss_cls, rcnn_loss_reg, rcnn_loss_corner and
        rcnn_loss; the tb_dict values are detached device tensors (nothing is read back)."""
        self._training_setup()
        tb_dict = {} if tb_dict is None else tb_dict
        r = self.forward_ret_dict
        if roi_loss_fused():
            losses = ops.rcnn_loss(r["rcnn_cls"], r["rcnn_reg"], r, self.loss_spec)
        else:
            losses = composed_rcnn_losses(r["rcnn_cls"], r["rcnn_reg"], r, self.loss_spec)
        rcnn_loss = losses[0] + losses[1] + losses[2]
        tb_dict.update(rcnn_loss_cls=losses[0].detach(), rcnn_loss_reg=losses[1].detach(), rcnn_loss_corner=losses[2].detach(),
                       rcnn_loss=rcnn_loss.detach())
        return rcnn_loss, tb_dict

    @torch.no_grad()
    def predict(self, batch_dict):
        """The eval outputs of the reference's forward: batch_cls_preds [B, N, 1 or C], batch_box_preds [B, N, 7],
        cls_preds_normalized=False.  In the fused mode, with the detector's POST_PROCESSING config in `post_process_cfg`, the
        decode AND the final selection are one call (ops.roi_decode_select); its results wait in batch_dict['final_selection']
        for vr_detector.post_processing."""
        rois, rcnn_cls, rcnn_reg = batch_dict["rois"], batch_dict["rcnn_cls"], batch_dict["rcnn_reg"]
        if rois.shape[-1] != BOX_CODE_SIZE:
            return batch_dict                                                   # RoIs with extra columns: pooled, not decoded
        batch_size = batch_dict["batch_size"]
        cfg = getattr(self, "post_process_cfg", None)
        if tail_fused() and cfg is not None and rcnn_cls.is_cuda:
            from .vr_detector import final_selection
            batch_box_preds = final_selection(batch_dict, cfg)
            batch_cls_preds = rcnn_cls.view(batch_size, -1, rcnn_cls.shape[-1])
        else:
            batch_cls_preds, batch_box_preds = self.generate_predicted_boxes(batch_size, rois, rcnn_cls, rcnn_reg)
        batch_dict["batch_cls_preds"] = batch_cls_preds
        batch_dict["batch_box_preds"] = batch_box_preds
        batch_dict["cls_preds_normalized"] = False
        return batch_dict


@ROI_HEADS.register_module
class VoxelRCNNHead(RoIHeadTemplate):
    def __init__(self, backbone_channels, model_cfg, point_cloud_range, voxel_size, num_class=1, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_class = 1 if _get(model_cfg, "CLASS_AGNOSTIC", True) else num_class
        self.pool_cfg = _need(model_cfg, "ROI_GRID_POOL")
        layer_cfg = _need(self.pool_cfg, "POOL_LAYERS")
        self.point_cloud_range = [float(v) for v in point_cloud_range]
        self.voxel_size = [float(v) for v in voxel_size]
        self.features_source = list(_need(self.pool_cfg, "FEATURES_SOURCE"))
        self.grid_size = int(_need(self.pool_cfg, "GRID_SIZE"))

        c_out = 0
        self.roi_grid_pool_layers = nn.ModuleList()
        for src_name in self.features_source:
            cfg = _need(layer_cfg, src_name)
            mlps = [[backbone_channels[src_name]] + list(m) for m in _need(cfg, "MLPS")]      # (the config stays as it was)
            self.roi_grid_pool_layers.append(NeighborVoxelSAModuleMSG(
                query_ranges=_need(cfg, "QUERY_RANGES"), nsamples=_need(cfg, "NSAMPLE"), radii=_need(cfg, "POOL_RADIUS"),
                mlps=mlps, pool_method=_need(cfg, "POOL_METHOD")))
            c_out += sum(m[-1] for m in mlps)

        dp = float(_get(model_cfg, "DP_RATIO", 0))
        pre_channel = self.grid_size ** 3 * c_out
        self.shared_fc_layer, pre_channel = _fc_stack(pre_channel, list(_need(model_cfg, "SHARED_FC")), dp, inplace=True)
        self.cls_fc_layers, cls_channel = _fc_stack(pre_channel, list(_need(model_cfg, "CLS_FC")), dp)
        self.cls_pred_layer = nn.Linear(cls_channel, self.num_class, bias=True)
        self.reg_fc_layers, reg_channel = _fc_stack(pre_channel, list(_need(model_cfg, "REG_FC")), dp)
        self.reg_pred_layer = nn.Linear(reg_channel, BOX_CODE_SIZE * self.num_class, bias=True)
        self.init_weights()

    def init_weights(self):
        for module_list in [self.shared_fc_layer, self.cls_fc_layers, self.reg_fc_layers]:
            for m in module_list.modules():
                if isinstance(m, nn.Linear):
                    nn.init.xavier_normal_(m.weight)
                    if m.bias is not None:
                        nn.init.constant_(m.bias, 0)
        nn.init.normal_(self.cls_pred_layer.weight, 0, 0.01)
        nn.init.constant_(self.cls_pred_layer.bias, 0)
        nn.init.normal_(self.reg_pred_layer.weight, mean=0, std=0.001)
        nn.init.constant_(self.reg_pred_layer.bias, 0)

    # ---- pooling
    def roi_grid_pool(self, batch_dict):
        """rois [B, num_rois, 7 + C]; multi_scale_3d_features / _strides of the backbone -> [B * num_rois, g^3, C_out]."""
        rois = batch_dict["rois"]
        batch_size = batch_dict["batch_size"]
        with_vf_transform = batch_dict.get("with_voxel_feature_transform", False)
        g = self.grid_size
        roi_grid_xyz, _ = self.get_global_grid_points_of_roi(rois, grid_size=g)
        roi_grid_xyz = roi_grid_xyz.view(batch_size, -1, 3)
        pcr, vs = self.point_cloud_range, self.voxel_size
        roi_grid_coords = torch.cat([(roi_grid_xyz[:, :, 0:1] - pcr[0]) // vs[0], (roi_grid_xyz[:, :, 1:2] - pcr[1]) // vs[1],
                                     (roi_grid_xyz[:, :, 2:3] - pcr[2]) // vs[2]], dim=-1)
        per_frame = roi_grid_coords.shape[1]
        batch_idx = torch.arange(batch_size, device=rois.device, dtype=rois.dtype).view(-1, 1, 1).expand(-1, per_frame, 1)
        roi_grid_batch_cnt = torch.full((batch_size,), per_frame, dtype=torch.int32, device=rois.device)
        new_xyz = roi_grid_xyz.contiguous().view(-1, 3)

        pooled_features_list = []
        for k, src_name in enumerate(self.features_source):
            cur_stride = batch_dict["multi_scale_3d_strides"][src_name]
            key = "multi_scale_3d_features_post" if with_vf_transform else "multi_scale_3d_features"
            cur_sp_tensors = batch_dict[key][src_name]
            cur_coords = cur_sp_tensors.indices
            cur_voxel_xyz = get_voxel_centers(cur_coords[:, 1:4], cur_stride, vs, pcr)
            frames = torch.arange(batch_size, device=cur_coords.device, dtype=cur_coords.dtype)
            cur_voxel_xyz_batch_cnt = (cur_coords[:, 0:1] == frames[None]).sum(0, dtype=torch.int32)
            directory = cur_sp_tensors.directory()                             # the one the level's convolutions built
            cur_roi_grid_coords = torch.cat([batch_idx, roi_grid_coords // cur_stride], dim=-1).int()
            pooled_features = self.roi_grid_pool_layers[k](
                xyz=cur_voxel_xyz.contiguous(), xyz_batch_cnt=cur_voxel_xyz_batch_cnt, new_xyz=new_xyz,
                new_xyz_batch_cnt=roi_grid_batch_cnt, new_coords=cur_roi_grid_coords.contiguous().view(-1, 4),
                features=cur_sp_tensors.features.contiguous(), voxel2point_indices=directory)
            pooled_features_list.append(pooled_features.reshape(-1, g ** 3, pooled_features.shape[-1]))
        return torch.cat(pooled_features_list, dim=-1)

    def rcnn_outputs(self, batch_dict):
        pooled_features = self.roi_grid_pool(batch_dict)
        pooled_features = pooled_features.reshape(pooled_features.size(0), -1)
        shared_features = self.shared_fc_layer(pooled_features)
        return self.cls_pred_layer(self.cls_fc_layers(shared_features)), self.reg_pred_layer(self.reg_fc_layers(shared_features))

    def forward(self, batch_dict):
        if "rois" not in batch_dict:
            nms_cfg = _get(self.model_cfg, "NMS_CONFIG")
            if nms_cfg is None or ("dense_cls_rows" not in batch_dict and "batch_box_preds" not in batch_dict):
                raise KeyError("VoxelRCNNHead.forward needs batch_dict['rois'] [B, num_rois, 7 + C], or a dense head's outputs "
                               "(AnchorHeadSingle) and the config's NMS_CONFIG to make them from")
            self.proposal_layer(batch_dict, _need(nms_cfg, "TRAIN" if self.training else "TEST"))
        batch_dict["rcnn_cls"], batch_dict["rcnn_reg"] = self.rcnn_outputs(batch_dict)
        if not self.training:
            self.predict(batch_dict)
        return batch_dict


@ROI_HEADS.register_module
class PVRCNNHead(RoIHeadTemplate):
    """VR/pcdet/models/roi_heads/pvrcnn_head.py: the RoI head of the PV-RCNN + 3D-DF tree.  The grid points of every RoI pool
    the keypoints of VoxelSetAbstraction (dualfusion/pfe.py) through one StackSAModuleMSG -- one fused kernel per scale in
    eval mode (dualfusion/pointnet2_stack.py) -- and the reference's Conv1d layers refine them.  The proposal layer, the
    decoding, `forward_train` and `get_loss` are RoIHeadTemplate's, shared with VoxelRCNNHead (and with its limits: the
    9000-candidate TRAIN proposals stay refused).  `point_cls_scores` is what PointHeadSimple (dualfusion/dense_heads.py) writes
    in front of this head in the PVRCNN detector; a caller that runs the head alone supplies it."""

    def __init__(self, input_channels, model_cfg, num_class=1, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_class = 1 if _get(model_cfg, "CLASS_AGNOSTIC", True) else num_class
        self.pool_cfg = _need(model_cfg, "ROI_GRID_POOL")
        self.grid_size = int(_need(self.pool_cfg, "GRID_SIZE"))
        self.roi_grid_pool_layer, num_c_out = build_local_aggregation_module(input_channels=input_channels, config=self.pool_cfg)

        dp = float(_get(model_cfg, "DP_RATIO", 0))
        pre_channel = self.grid_size ** 3 * num_c_out
        shared_fc_list = []
        widths = list(_need(model_cfg, "SHARED_FC"))
        for k, width in enumerate(widths):
            shared_fc_list.extend([nn.Conv1d(pre_channel, width, kernel_size=1, bias=False), nn.BatchNorm1d(width), nn.ReLU()])
            pre_channel = width
            if k != len(widths) - 1 and dp > 0:
                shared_fc_list.append(nn.Dropout(dp))
        self.shared_fc_layer = nn.Sequential(*shared_fc_list)
        self.cls_layers = self.make_fc_layers(pre_channel, self.num_class, list(_need(model_cfg, "CLS_FC")), dp)
        self.reg_layers = self.make_fc_layers(pre_channel, BOX_CODE_SIZE * self.num_class, list(_need(model_cfg, "REG_FC")), dp)
        self.init_weights()

    @staticmethod
    def make_fc_layers(input_channels, output_channels, fc_list, dp_ratio):
        """roi_head_template.py:29-43 (the dropout follows the first layer whenever DP_RATIO >= 0)"""
        fc_layers = []
        pre_channel = input_channels
        for k, width in enumerate(fc_list):
            fc_layers.extend([nn.Conv1d(pre_channel, width, kernel_size=1, bias=False), nn.BatchNorm1d(width), nn.ReLU()])
            pre_channel = width
            if dp_ratio >= 0 and k == 0:
                fc_layers.append(nn.Dropout(dp_ratio))
        fc_layers.append(nn.Conv1d(pre_channel, output_channels, kernel_size=1, bias=True))
        return nn.Sequential(*fc_layers)

    def init_weights(self):
        """pvrcnn_head.py:44-62 with weight_init='xavier' (every Conv2d / Conv1d of the head, the pooling layer's included)"""
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Conv1d)):
                nn.init.xavier_normal_(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
        nn.init.normal_(self.reg_layers[-1].weight, mean=0, std=0.001)

    def roi_grid_pool(self, batch_dict):
        """rois [B, num_rois, 7 + C], point_coords [P, 4] (b, x, y, z) stacked frame after frame, point_features [P, C],
        point_cls_scores [P] -> [B * num_rois, g^3, C_out]."""
        if "point_cls_scores" not in batch_dict:
            raise KeyError("PVRCNNHead.roi_grid_pool needs batch_dict['point_cls_scores'] [P] (the keypoint scores "
                           "PointHeadSimple writes)")
        batch_size = batch_dict["batch_size"]
        rois = batch_dict["rois"]
        point_coords = batch_dict["point_coords"]
        point_features = batch_dict["point_features"] * batch_dict["point_cls_scores"].view(-1, 1)
        g = self.grid_size
        global_roi_grid_points, _ = self.get_global_grid_points_of_roi(rois, grid_size=g)
        global_roi_grid_points = global_roi_grid_points.view(batch_size, -1, 3)
        xyz = point_coords[:, 1:4]
        xyz_batch_cnt = frame_counts(point_coords[:, 0], batch_size)
        new_xyz = global_roi_grid_points.reshape(-1, 3)
        new_xyz_batch_cnt = torch.full((batch_size,), global_roi_grid_points.shape[1], dtype=torch.int32, device=xyz.device)
        _, pooled_features = self.roi_grid_pool_layer(xyz=xyz.contiguous(), xyz_batch_cnt=xyz_batch_cnt, new_xyz=new_xyz,
                                                      new_xyz_batch_cnt=new_xyz_batch_cnt, features=point_features.contiguous())
        return pooled_features.view(-1, g ** 3, pooled_features.shape[-1])

    def rcnn_outputs(self, batch_dict):
        pooled_features = self.roi_grid_pool(batch_dict)                       # [B * N, g^3, C]
        batch_size_rcnn = pooled_features.shape[0]
        pooled_features = pooled_features.permute(0, 2, 1).contiguous().view(batch_size_rcnn, -1, 1)
        shared_features = self.shared_fc_layer(pooled_features)
        rcnn_cls = self.cls_layers(shared_features).transpose(1, 2).contiguous().squeeze(dim=1)
        rcnn_reg = self.reg_layers(shared_features).transpose(1, 2).contiguous().squeeze(dim=1)
        return rcnn_cls, rcnn_reg

    def forward(self, batch_dict):
        if self.training:
            return self.forward_train(batch_dict)
        if "rois" not in batch_dict:
            nms_cfg = _get(self.model_cfg, "NMS_CONFIG")
            if nms_cfg is None or ("dense_cls_rows" not in batch_dict and "batch_box_preds" not in batch_dict):
                raise KeyError("PVRCNNHead.forward needs batch_dict['rois'] [B, num_rois, 7 + C], or a dense head's outputs "
                               "(AnchorHeadSingle) and the config's NMS_CONFIG to make them from")
            self.proposal_layer(batch_dict, _need(nms_cfg, "TEST"))
        batch_dict["rcnn_cls"], batch_dict["rcnn_reg"] = self.rcnn_outputs(batch_dict)
        self.predict(batch_dict)
        return batch_dict


def class_agnostic_nms(box_scores, box_preds, pre_max, post_max, thresh, score_thresh=None):
    """VR/pcdet/models/model_utils/model_nms_utils.py:6-25 on iou3d_nms.nms_gpu -> indices into box_scores."""
    if score_thresh is not None:
        scores_mask = box_scores >= score_thresh
        box_scores, box_preds = box_scores[scores_mask], box_preds[scores_mask]
    selected = box_scores.new_zeros((0,), dtype=torch.long)
    if box_scores.shape[0] > 0:
        order = torch.sort(box_scores, descending=True, stable=True)[1][:min(pre_max, box_scores.shape[0])]   # ties: lower index
        keep_idx, _ = iou3d_nms.nms_gpu(box_preds[order][:, 0:7], box_scores[order], thresh)
        selected = order[keep_idx[:post_max]]
    if score_thresh is not None:
        selected = scores_mask.nonzero().view(-1)[selected]
    return selected
