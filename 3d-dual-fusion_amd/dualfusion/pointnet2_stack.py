"""The voxel-query part of pcdet's `pointnet2_stack` under the reference's names and signatures
(VR/pcdet/ops/pointnet2/pointnet2_stack/voxel_query_utils.py, pointnet2_utils.py:GroupingOperation,
voxel_pool_modules.py:NeighborVoxelSAModuleMSG), on csrc/roipool.hip.

Wherever the reference takes its dense `voxel2point_indices` [B, Z, Y, X] tensor, an `ops.GridDirectory` over the same
voxels is accepted too (row i of the indices it was built from = row i of `xyz`); the directory is the product path.
`NeighborVoxelSAModuleMSG` runs one fused kernel per scale in eval mode without autograd (query, gather, position term,
ReLU and pool; nothing of size M * C * nsample is stored) and the reference's formulation on the query and grouping ops
otherwise (the composed path: it trains); `DF3D_ROI_POOL_FUSED=0` keeps the composed path everywhere."""
import os
from typing import List

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops


class VoxelQuery(torch.autograd.Function):
    @staticmethod
    def forward(ctx, max_range, radius: float, nsample: int, xyz: torch.Tensor, new_xyz: torch.Tensor,
                new_coords: torch.Tensor, point_indices):
        """max_range (z, y, x); xyz [N1 + N2 .., 3]; new_xyz [M1 + M2 .., 3]; new_coords int32 [M, 4] (batch, z, y, x);
        point_indices: dense int32 [B, Z, Y, X] or a GridDirectory.  Returns idx int32 [M, nsample] of global rows with
        the rows of empty balls set to 0, and empty_ball_mask bool [M]."""
        idx = ops.voxel_query(max_range, radius, nsample, xyz, new_xyz, new_coords, point_indices)
        empty_ball_mask = idx[:, 0] == -1
        idx.masked_fill_(empty_ball_mask[:, None], 0)
        ctx.mark_non_differentiable(idx, empty_ball_mask)
        return idx, empty_ball_mask

    @staticmethod
    def backward(ctx, a=None, b=None):
        return None, None, None, None, None, None, None


voxel_query = VoxelQuery.apply


# `GroupingOperation.apply(features, features_batch_cnt, idx, idx_batch_cnt)`: features float32 [N1 + N2 .., C], idx int32
# [M1 + M2 .., nsample] local to its frame, counts int32 [B], all contiguous -> [M, C, nsample]; the backward is the ordered,
# atomic-free sum of ops.group_points_stack_backward
GroupingOperation = ops._GroupPointsStack


def grouping_operation(features, features_batch_cnt, idx, idx_batch_cnt):
    """`GroupingOperation.apply` of the reference, with its counts converted to int32 where a caller holds them wider."""
    return ops.group_points_stack(features.contiguous(), features_batch_cnt.int().contiguous(), idx.contiguous(),
                                  idx_batch_cnt.int().contiguous())


def _local_indices(idx, empty_ball_mask, xyz_batch_cnt, new_xyz_batch_cnt):
    """Global rows -> rows local to their frame.  The reference does this through `.view(batch_size, -1, nsample)`, which
    needs the same number of centres in every frame; the counts serve any split and agree wherever that is defined."""
    cnt = xyz_batch_cnt.long()
    starts = torch.cumsum(cnt, 0) - cnt
    ends = torch.cumsum(new_xyz_batch_cnt.long(), 0)
    frame = torch.bucketize(torch.arange(idx.shape[0], device=idx.device), ends, right=True)
    frame = frame.clamp_(max=cnt.shape[0] - 1)
    local = idx - starts[frame].to(torch.int32)[:, None]
    return local.masked_fill_(empty_ball_mask[:, None], 0)


class VoxelQueryAndGrouping(nn.Module):
    def __init__(self, max_range, radius: float, nsample: int):
        super().__init__()
        self.max_range, self.radius, self.nsample = max_range, radius, nsample

    def forward(self, new_coords: torch.Tensor, xyz: torch.Tensor, xyz_batch_cnt: torch.Tensor, new_xyz: torch.Tensor,
                new_xyz_batch_cnt: torch.Tensor, features: torch.Tensor, voxel2point_indices):
        """Returns grouped_features [M, C, nsample], grouped_xyz [M, 3, nsample], empty_ball_mask [M]."""
        idx, empty_ball_mask = voxel_query(self.max_range, self.radius, self.nsample, xyz, new_xyz, new_coords,
                                           voxel2point_indices)
        idx = _local_indices(idx, empty_ball_mask, xyz_batch_cnt, new_xyz_batch_cnt)
        grouped_xyz = grouping_operation(xyz, xyz_batch_cnt, idx, new_xyz_batch_cnt)
        grouped_features = grouping_operation(features, xyz_batch_cnt, idx, new_xyz_batch_cnt)
        return grouped_features, grouped_xyz, empty_ball_mask


def _bn_fold(bn):
    scale = bn.weight * torch.rsqrt(bn.running_var + bn.eps)
    return scale, bn.bias - bn.running_mean * scale


def fused_enabled():
    return os.environ.get("DF3D_ROI_POOL_FUSED", "1") != "0"


class NeighborVoxelSAModuleMSG(nn.Module):
    def __init__(self, *, query_ranges: List[List[int]], radii: List[float], nsamples: List[int], mlps: List[List[int]],
                 use_xyz: bool = True, pool_method="max_pool"):
        super().__init__()
        assert len(query_ranges) == len(nsamples) == len(mlps)
        self.groupers = nn.ModuleList()
        self.mlps_in = nn.ModuleList()
        self.mlps_pos = nn.ModuleList()
        self.mlps_out = nn.ModuleList()
        for i in range(len(query_ranges)):
            self.groupers.append(VoxelQueryAndGrouping(query_ranges[i], radii[i], nsamples[i]))
            mlp_spec = mlps[i]
            self.mlps_in.append(nn.Sequential(nn.Conv1d(mlp_spec[0], mlp_spec[1], kernel_size=1, bias=False),
                                              nn.BatchNorm1d(mlp_spec[1])))
            self.mlps_pos.append(nn.Sequential(nn.Conv2d(3, mlp_spec[1], kernel_size=1, bias=False),
                                               nn.BatchNorm2d(mlp_spec[1])))
            self.mlps_out.append(nn.Sequential(nn.Conv1d(mlp_spec[1], mlp_spec[2], kernel_size=1, bias=False),
                                               nn.BatchNorm1d(mlp_spec[2]), nn.ReLU()))
        self.relu = nn.ReLU()
        self.pool_method = pool_method
        self.init_weights()

    def init_weights(self):
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Conv1d)):
                nn.init.kaiming_normal_(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            if isinstance(m, (nn.BatchNorm2d, nn.BatchNorm1d)):
                nn.init.constant_(m.weight, 1.0)
                nn.init.constant_(m.bias, 0)

    def takes_fused(self, k, voxel2point_indices):
        """The fused kernel serves scale k of this call (eval mode, no autograd, a directory, a served shape)."""
        g = self.groupers[k]
        bns = (self.mlps_in[k][1], self.mlps_pos[k][1], self.mlps_out[k][1])
        return (not self.training and not torch.is_grad_enabled() and fused_enabled()
                and all(bn.running_var is not None for bn in bns)
                and ops.voxel_pool_fused_supported(self.mlps_in[k][0].out_channels, g.nsample, g.max_range, self.pool_method,
                                                   voxel2point_indices))

    def _fused(self, k, xyz, new_xyz, new_coords, features, grid):
        conv, bn = self.mlps_in[k]
        scale, shift = _bn_fold(bn)
        rows_in = F.linear(features, conv.weight[:, :, 0] * scale[:, None], shift)
        conv, bn = self.mlps_pos[k]
        scale, shift = _bn_fold(bn)
        w_pos = torch.cat([conv.weight[:, :, 0, 0] * scale[:, None], shift[:, None]], 1).contiguous()
        g = self.groupers[k]
        pooled = ops.voxel_pool_fused(rows_in.contiguous(), xyz, grid, new_xyz, new_coords, g.max_range, g.radius, g.nsample,
                                      w_pos, self.pool_method)
        conv, bn = self.mlps_out[k][0], self.mlps_out[k][1]
        scale, shift = _bn_fold(bn)
        return F.relu(F.linear(pooled, conv.weight[:, :, 0] * scale[:, None], shift))

    def _composed(self, k, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, new_coords, features, voxel2point_indices):
        # every layer of the module is a per-row layer: a linear over channels-last rows and the row BatchNorm kernels
        # (ops.batch_norm_rows: batch statistics in train mode, bnrows.hip), no [1, C, N] / [1, C, M, nsample] round trips
        features_in = ops.batch_norm_rows(self.mlps_in[k][1], F.linear(features, self.mlps_in[k][0].weight[:, :, 0]))
        grouped_features, grouped_xyz, empty_ball_mask = self.groupers[k](
            new_coords, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features_in, voxel2point_indices)
        keep = (~empty_ball_mask)[:, None, None].to(grouped_features.dtype)
        # empty balls: features and relative coordinates are zeroed BEFORE the position branch (voxel_pool_modules.py:99-105)
        grouped_features = (grouped_features * keep).permute(0, 2, 1)                              # [M, nsample, C]
        rel = ((grouped_xyz - new_xyz.unsqueeze(-1)) * keep).permute(0, 2, 1).reshape(-1, 3)       # [M * nsample, 3]
        # mlps_pos' 1 x 1 Conv2d + BatchNorm2d see every (m, s) entry as one row of three channels
        pos = ops.batch_norm_rows(self.mlps_pos[k][1], F.linear(rel, self.mlps_pos[k][0].weight[:, :, 0, 0]))
        new_features = self.relu(grouped_features + pos.view(grouped_features.shape))
        if self.pool_method == "max_pool":
            pooled = new_features.max(dim=1)[0]
        elif self.pool_method == "avg_pool":
            pooled = new_features.mean(dim=1)
        else:
            raise NotImplementedError
        return ops.batch_norm_rows(self.mlps_out[k][1], F.linear(pooled, self.mlps_out[k][0].weight[:, :, 0]), relu=True)

    def forward(self, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, new_coords, features, voxel2point_indices):
        """xyz [N1 + N2 .., 3] with counts [B]; new_xyz [M1 + M2 .., 3] with counts [B]; new_coords int32 [M, 4] in the
        reference's (batch, x, y, z) order; features [N, C]; voxel2point_indices: dense [B, Z, Y, X] or a GridDirectory.
        Returns [M, sum_k mlps[k][-1]]."""
        new_coords = new_coords[:, [0, 3, 2, 1]].contiguous()
        xyz, new_xyz, features = xyz.contiguous(), new_xyz.contiguous(), features.contiguous()
        new_features_list = []
        for k in range(len(self.groupers)):
            if self.takes_fused(k, voxel2point_indices):
                new_features_list.append(self._fused(k, xyz, new_xyz, new_coords, features, voxel2point_indices))
            else:
                new_features_list.append(self._composed(k, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, new_coords,
                                                        features, voxel2point_indices))
        return torch.cat(new_features_list, dim=1)


# ---------------------------------------------------------------------------------------------------------------------------
# The ball-query part (pointnet2_utils.py:8-155, pointnet2_modules.py:10-112) on csrc/stackpool.hip: the point side of
# PV-RCNN (VoxelSetAbstraction in dualfusion/pfe.py, PVRCNNHead.roi_grid_pool).  `StackSAModuleMSG` runs one fused kernel per
# scale in eval mode without autograd (ball query, gather, both MLP layers, max; nothing of size M * C * nsample is stored)
# and the reference's formulation on the query and grouping ops otherwise (the composed path: it trains, and it serves
# avg_pool, MLPs of another depth and channel counts the kernel does not); `DF3D_STACK_SA_FUSED=0` keeps the composed path
# everywhere.  `stack_farthest_point_sample` is the reference's stacked FPS (one launch for all segments).  Not provided:
# `VectorPoolAggregationModuleMSG` (refused by name), three_nn / interpolate.
def ball_query_stack(radius, nsample, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt):
    """`BallQuery.apply` of the reference: idx int32 [M, nsample] local to the frame with the rows of empty balls set to 0,
    and empty_ball_mask bool [M].  The counts stay on the device."""
    with torch.no_grad():
        idx = ops.ball_query_stack(radius, nsample, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt)
        empty_ball_mask = idx[:, 0] == -1
        idx.masked_fill_(empty_ball_mask[:, None], 0)
    return idx, empty_ball_mask


ball_query = ball_query_stack


class QueryAndGroup(nn.Module):
    def __init__(self, radius: float, nsample: int, use_xyz: bool = True):
        super().__init__()
        self.radius, self.nsample, self.use_xyz = radius, nsample, use_xyz

    def forward(self, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features=None):
        """Returns new_features [M, (3 +) C, nsample] (relative xyz first) and idx [M, nsample]; the entries of an empty ball
        are zero.  The counts are not summed on the host (the reference's two asserts cost a device-to-host read each)."""
        idx, empty_ball_mask = ball_query_stack(self.radius, self.nsample, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt)
        keep = (~empty_ball_mask)[:, None, None].to(xyz.dtype)
        grouped_xyz = (grouping_operation(xyz, xyz_batch_cnt, idx, new_xyz_batch_cnt) - new_xyz.unsqueeze(-1)) * keep
        if features is not None:
            grouped_features = grouping_operation(features, xyz_batch_cnt, idx, new_xyz_batch_cnt) * keep
            new_features = torch.cat([grouped_xyz, grouped_features], dim=1) if self.use_xyz else grouped_features
        else:
            assert self.use_xyz, "Cannot have not features and not use xyz as a feature!"
            new_features = grouped_xyz
        return new_features, idx


def stack_farthest_point_sample(xyz, xyz_batch_cnt, npoint):
    """`StackFarthestPointSampling.apply` of the reference (pointnet2_utils.py:187-221): xyz [N1 + N2 .., 3], xyz_batch_cnt
    [B], npoint an int, a list or a tensor [B] -> int32 [sum(npoint)] of global rows, all segments in one launch.  Not
    differentiable.  With a tensor `npoint` its sum is read back once, as the reference reads it."""
    with torch.no_grad():
        return ops.stack_furthest_point_sample(xyz.contiguous(), xyz_batch_cnt.int().contiguous(),
                                               npoint.int().contiguous() if isinstance(npoint, torch.Tensor) else npoint)


def frame_counts(batch_idx, batch_size):
    """int32 [B]: rows per frame, counted on the device without a read-back"""
    ones = torch.ones(batch_idx.shape[0], dtype=torch.int32, device=batch_idx.device)
    return torch.zeros(batch_size, dtype=torch.int32, device=batch_idx.device).index_add_(0, batch_idx.long(), ones)


def stack_sa_fused_enabled():
    return os.environ.get("DF3D_STACK_SA_FUSED", "1") != "0"


class StackSAModuleMSG(nn.Module):
    def __init__(self, *, radii: List[float], nsamples: List[int], mlps: List[List[int]], use_xyz: bool = True,
                 pool_method="max_pool"):
        super().__init__()
        assert len(radii) == len(nsamples) == len(mlps)
        self.groupers = nn.ModuleList()
        self.mlps = nn.ModuleList()
        for i in range(len(radii)):
            self.groupers.append(QueryAndGroup(radii[i], nsamples[i], use_xyz=use_xyz))
            mlp_spec = list(mlps[i])                         # (the reference adds the 3 to its caller's list)
            if use_xyz:
                mlp_spec[0] += 3
            shared_mlps = []
            for k in range(len(mlp_spec) - 1):
                shared_mlps.extend([nn.Conv2d(mlp_spec[k], mlp_spec[k + 1], kernel_size=1, bias=False),
                                    nn.BatchNorm2d(mlp_spec[k + 1]), nn.ReLU()])
            self.mlps.append(nn.Sequential(*shared_mlps))
        self.use_xyz = use_xyz
        self.pool_method = pool_method
        self.init_weights()

    def init_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            if isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1.0)
                nn.init.constant_(m.bias, 0)

    def takes_fused(self, k, xyz):
        """The fused kernel serves scale k of this call (eval mode, no autograd, on the device, a served shape)."""
        mlp = self.mlps[k]
        if self.training or torch.is_grad_enabled() or not xyz.is_cuda or not stack_sa_fused_enabled() or len(mlp) != 6:
            return False
        return (self.use_xyz and mlp[1].running_var is not None and mlp[4].running_var is not None
                and ops.stack_sa_fused_supported(mlp[0].out_channels, mlp[3].out_channels, self.groupers[k].nsample,
                                                 self.pool_method))

    def fused_operands(self, k, features):
        """The operands of ops.stack_sa_fused for scale k, BatchNorms folded: rows_in [N, C1] = the features through the first
        layer's feature columns (one GEMM over the N source rows instead of over M * nsample; None for a source without
        features), w_pos [C1, 4] = (its xyz columns | shift), w2 [C2, C1], b2 [C2]."""
        conv, bn = self.mlps[k][0], self.mlps[k][1]
        scale, shift = _bn_fold(bn)
        w1 = conv.weight[:, :, 0, 0] * scale[:, None]                                      # [C1, 3 + C_in]
        w_pos = torch.cat([w1[:, :3], shift[:, None]], 1).contiguous()
        rows_in = F.linear(features, w1[:, 3:]).contiguous() if features is not None and w1.shape[1] > 3 else None
        conv, bn = self.mlps[k][3], self.mlps[k][4]
        scale, shift = _bn_fold(bn)
        return rows_in, w_pos, (conv.weight[:, :, 0, 0] * scale[:, None]).contiguous(), shift.contiguous()

    def _fused(self, k, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features):
        g = self.groupers[k]
        rows_in, w_pos, w2, b2 = self.fused_operands(k, features)
        return ops.stack_sa_fused(rows_in, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, g.radius, g.nsample, w_pos, w2, b2)

    def _composed(self, k, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features):
        grouped, _ = self.groupers[k](xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features)  # [M, C, nsample]
        M, C, nsample = grouped.shape
        # the 1 x 1 Conv2d + BatchNorm2d layers see every (m, s) entry as one row: linears over channels-last rows and the row
        # BatchNorm kernels (ops.batch_norm_rows: batch statistics in train mode), no [1, C, M, nsample] round trips
        rows = grouped.permute(0, 2, 1).reshape(M * nsample, C)
        mlp = self.mlps[k]
        for i in range(0, len(mlp), 3):
            rows = ops.batch_norm_rows(mlp[i + 1], F.linear(rows, mlp[i].weight[:, :, 0, 0]), relu=True)
        rows = rows.view(M, nsample, rows.shape[1])
        if self.pool_method == "max_pool":
            return rows.max(dim=1)[0]
        if self.pool_method == "avg_pool":
            return rows.mean(dim=1)
        raise NotImplementedError

    def forward(self, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features=None, empty_voxel_set_zeros=True):
        """xyz [N1 + N2 .., 3] with counts [B]; new_xyz [M1 + M2 .., 3] with counts [B]; features [N, C] or None.
        Returns new_xyz and new_features [M, sum_k mlps[k][-1]]."""
        xyz, new_xyz = xyz.contiguous(), new_xyz.contiguous()
        xyz_batch_cnt, new_xyz_batch_cnt = xyz_batch_cnt.int().contiguous(), new_xyz_batch_cnt.int().contiguous()
        features = features.contiguous() if features is not None else None
        new_features_list = []
        for k in range(len(self.groupers)):
            if self.takes_fused(k, xyz):
                new_features_list.append(self._fused(k, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features))
            else:
                new_features_list.append(self._composed(k, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features))
        return new_xyz, torch.cat(new_features_list, dim=1)


def _cfg_get(config, key, default=None):
    if hasattr(config, "get"):
        return config.get(key, default)
    return getattr(config, key, default)


def build_local_aggregation_module(input_channels, config):
    """pointnet2_modules.py:10-27; `config` (a dict or an EasyDict) is not edited (the reference prepends to its MLPS)."""
    name = _cfg_get(config, "NAME", "StackSAModuleMSG")
    if name == "StackSAModuleMSG":
        mlps = [[input_channels] + list(m) for m in _cfg_get(config, "MLPS")]
        layer = StackSAModuleMSG(radii=list(_cfg_get(config, "POOL_RADIUS")), nsamples=list(_cfg_get(config, "NSAMPLE")),
                                 mlps=mlps, use_xyz=True, pool_method="max_pool")
        return layer, sum(m[-1] for m in mlps)
    if name == "VectorPoolAggregationModuleMSG":
        raise NotImplementedError("VectorPoolAggregationModuleMSG (the vector-pool aggregation of PV-RCNN++) is not provided: "
                                  "StackSAModuleMSG is the aggregation of every shipped PV-RCNN + 3D-DF config")
    raise NotImplementedError("local aggregation module %r" % (name,))
