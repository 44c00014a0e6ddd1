"""Voxelisation layer and mean voxel feature encoders with the reference's class names.

`Voxelization` = TF/mmdet3d/ops/voxel/voxelize.py:61-113 (hard voxelisation; `max_voxels` is a
(train, test) pair).  `VoxelGenerator` = CP/det3d/core/input/voxel_generator.py:5-30 (numba
semantics at the cap).  VFEs: `VoxelFeatureExtractorV3` (CP/.../voxel_encoder.py:8-24),
`HardSimpleVFE` (TF/.../voxel_encoder.py:13-44), `MeanVFE` (VR/.../mean_vfe.py:6-29).
The HIP kernel fuses the mean into the voxeliser; `voxelize_mean()` exposes that fused form and
skips the padded [M, T, C] tensor entirely.  Dynamic voxelisation (no caps, no dropped points):
`DynamicScatter` / `dynamic_scatter` (TF/mmdet3d/ops/voxel/scatter_points.py), `DynamicSimpleVFE`,
`DynamicVFE` (TF/.../voxel_encoder.py:47-283) on csrc/dynscatter.hip."""
import torch
from torch import nn

from . import ops as _ops
from .registry import READERS, VOXEL_ENCODERS


class _Voxelization(object):
    @staticmethod
    def apply(points, voxel_size, coors_range, max_points=35, max_voxels=20000):
        """voxelize.py:13-58.  max_points == -1 or max_voxels == -1 selects dynamic voxelisation
        (per-point (z, y, x) coordinates, -1 outside the grid)."""
        if max_points == -1 or max_voxels == -1:
            return _ops.dynamic_voxelize(points.contiguous().float(), voxel_size, coors_range)
        voxels, coors, num, _ = _ops.hard_voxelize(points.contiguous().float(), voxel_size, coors_range, max_points,
                                                   max_voxels, break_at_cap=True, want_voxels=True, want_mean=False)
        return voxels, coors, num


voxelization = _Voxelization.apply


class Voxelization(nn.Module):
    def __init__(self, voxel_size, point_cloud_range, max_num_points, max_voxels=20000):
        super(Voxelization, self).__init__()
        self.voxel_size = voxel_size
        self.point_cloud_range = point_cloud_range
        self.max_num_points = max_num_points
        if isinstance(max_voxels, tuple) or isinstance(max_voxels, list):
            self.max_voxels = tuple(max_voxels)
        else:
            self.max_voxels = (max_voxels, max_voxels)
        pcr = torch.tensor(point_cloud_range, dtype=torch.float32)
        vs = torch.tensor(voxel_size, dtype=torch.float32)
        grid_size = torch.round((pcr[3:] - pcr[:3]) / vs).long()
        input_feat_shape = grid_size[:2]
        self.grid_size = grid_size
        self.pcd_shape = [*input_feat_shape, 1][::-1]

    def _cap(self):
        return self.max_voxels[0] if self.training else self.max_voxels[1]

    def forward(self, input):
        return voxelization(input, self.voxel_size, self.point_cloud_range, self.max_num_points, self._cap())

    def voxelize_mean(self, points, break_at_cap=True, batch_index=None, while_waiting=None):
        """fused voxelise + mean VFE: (mean [M,C], coors [M,3] (z,y,x) -- or [M,4] (b,z,y,x) when `batch_index`
        is given --, num [M])."""
        _, coors, num, mean = _ops.hard_voxelize(points.contiguous().float(), self.voxel_size, self.point_cloud_range,
                                                 self.max_num_points, self._cap(), break_at_cap=break_at_cap,
                                                 want_voxels=False, want_mean=True, batch_index=batch_index,
                                                 while_waiting=while_waiting)
        return mean, coors, num

    def __repr__(self):
        return "%s(voxel_size=%s, point_cloud_range=%s, max_num_points=%s, max_voxels=%s)" % (
            self.__class__.__name__, self.voxel_size, self.point_cloud_range, self.max_num_points, self.max_voxels)


dynamic_scatter = _ops.dynamic_scatter


class DynamicScatter(nn.Module):
    """TF/mmdet3d/ops/voxel/scatter_points.py:53-107: reduces the points that share a voxel coordinate to one row, 'mean'
    when `average_points` else 'max'; returns (voxel_feats [M, C], voxel_coors [M, ndim]), voxels in ascending
    coordinate order.

    With 4-column (b, z, y, x) coordinates the reference loops over the samples in Python (one reduction and one host
    read each) and concatenates; here the batch index is simply the most significant key column of ONE native call,
    which gives the same rows in the same order for batch-sorted input.  The one divergence: the reference takes the
    batch size from the LAST row (`coors[-1, 0] + 1`) and silently drops samples beyond it; every non-negative batch id
    is kept here."""

    def __init__(self, voxel_size, point_cloud_range, average_points: bool):
        super(DynamicScatter, self).__init__()
        self.voxel_size = voxel_size
        self.point_cloud_range = point_cloud_range
        self.average_points = average_points

    def forward_single(self, points, coors):
        reduce = 'mean' if self.average_points else 'max'
        if not isinstance(coors, _ops.DynamicScatterPlan):
            coors = coors.contiguous()
        return dynamic_scatter(points.contiguous(), coors, reduce)

    def forward(self, points, coors):
        """points [N, C], coors [N, 3] (z, y, x) or [N, 4] (b, z, y, x) int32 -- or a `dynamic_scatter_plan` of them."""
        return self.forward_single(points, coors)

    def __repr__(self):
        tmpstr = self.__class__.__name__ + '('
        tmpstr += 'voxel_size=' + str(self.voxel_size)
        tmpstr += ', point_cloud_range=' + str(self.point_cloud_range)
        tmpstr += ', average_points=' + str(self.average_points)
        tmpstr += ')'
        return tmpstr


class VoxelGenerator(object):
    """CP/det3d/core/input/voxel_generator.py:5-30 on the GPU (numba `continue` semantics at the cap)."""

    def __init__(self, voxel_size, point_cloud_range, max_num_points, max_voxels=20000):
        self._voxel_size = voxel_size
        self._point_cloud_range = point_cloud_range
        self._max_num_points = max_num_points
        self._max_voxels = max_voxels

    def generate(self, points, max_voxels=-1):
        mv = self._max_voxels if max_voxels == -1 else max_voxels
        voxels, coors, num, _ = _ops.hard_voxelize(points.contiguous().float(), self._voxel_size,
                                                   self._point_cloud_range, self._max_num_points, mv,
                                                   break_at_cap=False, want_voxels=True, want_mean=False)
        return voxels, coors, num


@READERS.register_module
class VoxelFeatureExtractorV3(nn.Module):
    def __init__(self, num_input_features=4, norm_cfg=None, name="VoxelFeatureExtractorV3"):
        super(VoxelFeatureExtractorV3, self).__init__()
        self.name = name
        self.num_input_features = num_input_features

    def forward(self, features, num_voxels, coors=None):
        assert self.num_input_features == features.shape[-1]
        points_mean = features[:, :, :self.num_input_features].sum(dim=1, keepdim=False) / \
            num_voxels.type_as(features).view(-1, 1)
        return points_mean.contiguous()


@VOXEL_ENCODERS.register_module()
class HardSimpleVFE(nn.Module):
    def __init__(self, num_features=4):
        super(HardSimpleVFE, self).__init__()
        self.num_features = num_features
        self.fp16_enabled = False

    def forward(self, features, num_points, coors):
        points_mean = features[:, :, :self.num_features].sum(dim=1, keepdim=False) / \
            num_points.type_as(features).view(-1, 1)
        return points_mean.contiguous()


class MeanVFE(nn.Module):
    """VR/pcdet/models/backbones_3d/vfe/mean_vfe.py:6-29 (batch_dict in / out, count clamped >= 1)."""

    def __init__(self, model_cfg=None, num_point_features=4, **kwargs):
        super(MeanVFE, self).__init__()
        self.model_cfg = model_cfg
        self.num_point_features = num_point_features

    def get_output_feature_dim(self):
        return self.num_point_features

    def forward(self, batch_dict, **kwargs):
        voxel_features, voxel_num_points = batch_dict['voxels'], batch_dict['voxel_num_points']
        points_mean = voxel_features[:, :, :].sum(dim=1, keepdim=False)
        normalizer = torch.clamp_min(voxel_num_points.view(-1, 1), min=1.0).type_as(voxel_features)
        batch_dict['voxel_features'] = (points_mean / normalizer).contiguous()
        return batch_dict


@VOXEL_ENCODERS.register_module()
class DynamicSimpleVFE(nn.Module):
    """TF/mmdet3d/models/voxel_encoders/voxel_encoder.py:47-83: the mean of the points of every voxel, for dynamic
    voxelisation (`Voxelization(max_num_points=-1)` coordinates); no gradient, like the reference."""

    def __init__(self, voxel_size=(0.2, 0.2, 4), point_cloud_range=(0, -40, -3, 70.4, 40, 1)):
        super(DynamicSimpleVFE, self).__init__()
        self.scatter = DynamicScatter(voxel_size, point_cloud_range, True)
        self.fp16_enabled = False

    @torch.no_grad()
    def forward(self, features, coors):
        features, features_coors = self.scatter(features, coors)
        return features, features_coors


@VOXEL_ENCODERS.register_module()
class DynamicVFE(nn.Module):
    """TF/mmdet3d/models/voxel_encoders/voxel_encoder.py:86-283: point-wise Linear + BatchNorm + ReLU layers, each followed
    by a max / mean scatter into voxels whose result is gathered back to the points and concatenated for the next layer;
    optional decorations: offset to the voxel's point mean, offset to the voxel centre, distance to the origin.

    ONE `dynamic_scatter_plan` per forward serves the cluster mean, every layer's scatter and every gather back to the
    points (the reference sorts the coordinates again in each scatter and maps voxels to points through a dense
    B * Z * Y * X int64 canvas).  Points outside the grid (negative coordinates) get zero rows from the gather.  The
    reference counts three input channels for `with_distance` but appends one column, so it cannot run with that key;
    one channel is counted here."""

    def __init__(self, in_channels=4, feat_channels=[], with_distance=False, with_cluster_center=False,
                 with_voxel_center=False, voxel_size=(0.2, 0.2, 4), point_cloud_range=(0, -40, -3, 70.4, 40, 1),
                 norm_cfg=dict(type='BN1d', eps=1e-3, momentum=0.01), mode='max', fusion_layer=None,
                 return_point_feats=False):
        super(DynamicVFE, self).__init__()
        from .backbones import build_norm_layer
        assert mode in ['avg', 'max']
        assert len(feat_channels) > 0
        if fusion_layer is not None:
            raise NotImplementedError("DynamicVFE fusion_layer (PointFusion) is not part of the 3D-Dual-Fusion configs")
        if with_cluster_center:
            in_channels += 3
        if with_voxel_center:
            in_channels += 3
        if with_distance:
            in_channels += 1
        self.in_channels = in_channels
        self._with_distance = with_distance
        self._with_cluster_center = with_cluster_center
        self._with_voxel_center = with_voxel_center
        self.return_point_feats = return_point_feats
        self.fp16_enabled = False
        self.vx = voxel_size[0]
        self.vy = voxel_size[1]
        self.vz = voxel_size[2]
        self.x_offset = self.vx / 2 + point_cloud_range[0]
        self.y_offset = self.vy / 2 + point_cloud_range[1]
        self.z_offset = self.vz / 2 + point_cloud_range[2]
        self.point_cloud_range = point_cloud_range
        self.scatter = DynamicScatter(voxel_size, point_cloud_range, True)
        feat_channels = [self.in_channels] + list(feat_channels)
        vfe_layers = []
        for i in range(len(feat_channels) - 1):
            in_filters = feat_channels[i]
            out_filters = feat_channels[i + 1]
            if i > 0:
                in_filters *= 2
            _, norm_layer = build_norm_layer(norm_cfg, out_filters)
            vfe_layers.append(nn.Sequential(nn.Linear(in_filters, out_filters, bias=False), norm_layer,
                                            nn.ReLU(inplace=True)))
        self.vfe_layers = nn.ModuleList(vfe_layers)
        self.num_vfe = len(vfe_layers)
        self.vfe_scatter = DynamicScatter(voxel_size, point_cloud_range, (mode != 'max'))
        self.cluster_scatter = DynamicScatter(voxel_size, point_cloud_range, average_points=True)
        self.fusion_layer = None

    def forward(self, features, coors, points=None, img_feats=None, img_metas=None):
        """features [N, C] points, coors [N, 4] int32 (b, z, y, x) -> (voxel_feats [M, feat_channels[-1]], voxel_coors
        [M, 4]), or the point features of the last layer with `return_point_feats`."""
        plan = coors if isinstance(coors, _ops.DynamicScatterPlan) else _ops.dynamic_scatter_plan(coors.contiguous())
        coors = plan.coors
        features_ls = [features]
        if self._with_cluster_center:
            voxel_mean, _ = self.cluster_scatter(features[:, :3], plan)
            f_cluster = features[:, :3] - _ops.voxel_to_point(voxel_mean, plan)
            features_ls.append(f_cluster)
        if self._with_voxel_center:
            f_center = features.new_zeros(size=(features.size(0), 3))
            f_center[:, 0] = features[:, 0] - (coors[:, 3].type_as(features) * self.vx + self.x_offset)
            f_center[:, 1] = features[:, 1] - (coors[:, 2].type_as(features) * self.vy + self.y_offset)
            f_center[:, 2] = features[:, 2] - (coors[:, 1].type_as(features) * self.vz + self.z_offset)
            features_ls.append(f_center)
        if self._with_distance:
            features_ls.append(torch.norm(features[:, :3], 2, 1, keepdim=True))
        features = torch.cat(features_ls, dim=-1)
        for i, vfe in enumerate(self.vfe_layers):
            # (the library's fp32 product at every size: the split-operand row kernels behind ops.linear_rows are range-limited
            # and raw point features -- metres, intensities -- are not scaled for them)
            point_feats = _ops.batch_norm_rows(vfe[1], vfe[0](features), relu=True)
            voxel_feats, voxel_coors = self.vfe_scatter(point_feats, plan)
            if i != len(self.vfe_layers) - 1:
                features = torch.cat([point_feats, _ops.voxel_to_point(voxel_feats, plan)], dim=1)
        if self.return_point_feats:
            return point_feats
        return voxel_feats, voxel_coors
