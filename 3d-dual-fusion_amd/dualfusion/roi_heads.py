"""VoxelRCNNHead (VR/pcdet/models/roi_heads/voxelrcnn_head.py): RoI grid pooling over the backbone's sparse levels and
the refinement layers on GIVEN RoIs.  The reference's constructor signature, config keys and parameter names, so its
checkpoints load.  There is no proposal layer, target assignment, loss or box decoding here: `forward` reads
`batch_dict['rois']` and stores `rcnn_cls` / `rcnn_reg`.

`roi_grid_pool` never builds the reference's dense voxel-to-point tensor (`generate_voxel2pinds`: B * Z * Y * X int32 per
level and step): every source level is looked up through its occupancy directory, the one its sparse tensor already
carries where a convolution built it."""
import torch
import torch.nn as nn

from . import ops
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

    def forward(self, batch_dict):
        if "rois" not in batch_dict:
            raise KeyError("VoxelRCNNHead.forward needs batch_dict['rois'] [B, num_rois, 7 + C]: this head has no "
                           "proposal layer, the RoIs come from the caller")
        pooled_features = self.roi_grid_pool(batch_dict)
        pooled_features = pooled_features.reshape(pooled_features.size(0), -1)
        shared_features = self.shared_fc_layer(pooled_features)
        batch_dict["rcnn_cls"] = self.cls_pred_layer(self.cls_fc_layers(shared_features))
        batch_dict["rcnn_reg"] = self.reg_pred_layer(self.reg_fc_layers(shared_features))
        return batch_dict
