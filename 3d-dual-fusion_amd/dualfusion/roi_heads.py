"""VoxelRCNNHead (VR/pcdet/models/roi_heads/voxelrcnn_head.py over roi_head_template.py) for inference: the proposal layer,
RoI grid pooling over the backbone's sparse levels, the refinement layers and the decoding of their outputs.  The
reference's constructor signature, config keys and parameter names, so its checkpoints load.  There is no target
assignment and no loss here.

`forward` reads `batch_dict['rois']` where the caller supplies them; otherwise `proposal_layer` makes them from the dense
head's outputs and NMS_CONFIG['TEST'] -- from the head maps and anchor tables of AnchorHeadSingle's fused mode in one call
with no host round trip (ops.anchor_proposals, csrc/proposals.hip), or from `batch_cls_preds` /
`batch_box_preds` with the reference's per-frame loop on iou3d_nms.nms_gpu (composed mode, DF3D_VR_TAIL_FUSED=0).  It stores
`rcnn_cls` / `rcnn_reg` and, in eval, `batch_cls_preds`, `batch_box_preds` and `cls_preds_normalized=False`.

`roi_grid_pool` never builds the reference's dense voxel-to-point tensor (`generate_voxel2pinds`: B * Z * Y * X int32 per
level and step): every source level is looked up through its occupancy directory, the one its sparse tensor already
carries where a convolution built it."""
import torch
import torch.nn as nn

from . import iou3d_nms, ops
from .dense_heads import residual_decode, tail_fused
from .pointnet2_stack import NeighborVoxelSAModuleMSG
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
    rot = torch.stack((cosa, sina, zeros, -sina, cosa, zeros, zeros, zeros, ones), dim=1).view(-1, 3, 3).float()
    points_rot = torch.matmul(points[:, :, 0:3], rot)
    return torch.cat((points_rot, points[:, :, 3:]), dim=-1)


def get_voxel_centers(voxel_coords, downsample_times, voxel_size, point_cloud_range):
    """VR/pcdet/utils/common_utils.py:get_voxel_centers: voxel_coords [N, 3] (z, y, x) -> centres [N, 3] (x, y, z)."""
    centers = voxel_coords[:, [2, 1, 0]].float()
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


@ROI_HEADS.register_module
class VoxelRCNNHead(nn.Module):
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
        pre, post, thresh = self.check_nms_config(nms_config, "VoxelRCNNHead.proposal_layer")
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
                raise NotImplementedError("VoxelRCNNHead.proposal_layer: stacked predictions (batch_index) are not supported")
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

    def forward(self, batch_dict):
        if "rois" not in batch_dict:
            nms_cfg = _get(self.model_cfg, "NMS_CONFIG")
            if nms_cfg is None or ("dense_cls_rows" not in batch_dict and "batch_box_preds" not in batch_dict):
                raise KeyError("VoxelRCNNHead.forward needs batch_dict['rois'] [B, num_rois, 7 + C], or a dense head's outputs "
                               "(AnchorHeadSingle) and the config's NMS_CONFIG to make them from")
            self.proposal_layer(batch_dict, _need(nms_cfg, "TRAIN" if self.training else "TEST"))
        pooled_features = self.roi_grid_pool(batch_dict)
        pooled_features = pooled_features.reshape(pooled_features.size(0), -1)
        shared_features = self.shared_fc_layer(pooled_features)
        batch_dict["rcnn_cls"] = self.cls_pred_layer(self.cls_fc_layers(shared_features))
        batch_dict["rcnn_reg"] = self.reg_pred_layer(self.reg_fc_layers(shared_features))
        if not self.training:
            self.predict(batch_dict)
        return batch_dict

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
