"""AnchorHeadSingle (VR/pcdet/models/dense_heads/anchor_head_single.py over anchor_head_template.py) for inference, plus the
two plain-torch modules in front of it: HeightCompression and BaseBEVBackbone (VR/pcdet/models/backbones_2d/).  The
reference's constructor signatures, config keys and parameter names, so its checkpoints load.

In eval the head has two modes, chosen per call by DF3D_VR_TAIL_FUSED (default 1):
  fused     the three 1x1 convolutions run as ONE convolution into channels-last pixel rows; the rows and the anchor TABLES go
            into batch_dict (`dense_cls_rows`, `dense_box_rows`, `dense_dir_rows`, `dense_anchor_tables`) and no anchor is
            decoded here: VoxelRCNNHead.proposal_layer decodes the NMS_PRE_MAXSIZE selected ones (csrc/proposals.hip);
  composed  `batch_cls_preds`, `batch_box_preds`, `cls_preds_normalized=False` as the reference's generate_predicted_boxes
            makes them (every anchor decoded in torch).
Target assignment and the losses are not here: forward in training mode raises NotImplementedError."""
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

    def forward(self, data_dict):
        if self.training:
            raise NotImplementedError("AnchorHeadSingle: target assignment and the anchor losses are not implemented; "
                                      "this head runs in eval mode only")
        x = data_dict["spatial_features_2d"]
        B, _, H, W = x.shape
        if (H, W) != (self.tables.H, self.tables.W):
            raise ValueError("AnchorHeadSingle: the map is %d x %d, the anchors were built for %d x %d" % (H, W, self.tables.H, self.tables.W))
        cls_rows, box_rows, dir_rows = self.head_rows(x)
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
