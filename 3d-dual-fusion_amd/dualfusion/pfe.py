"""VoxelSetAbstraction (VR/pcdet/models/backbones_3d/pfe/voxel_set_abstraction.py:124-411), the point feature encoder of
the PV-RCNN + 3D-DF tree: keypoints by furthest point sampling, their features gathered from the BEV map (bilinear), the raw
points and the sparse levels x_conv1..4 (StackSAModuleMSG over voxel centres), and the fusion layer.  The reference's
constructor signature, config keys, parameter names and batch_dict keys.

Device path: the BEV sample is one launch for all frames (ops.bev_interpolate, NCHW read in place, ordered backward), every
set-abstraction scale is one fused kernel in eval mode (dualfusion/pointnet2_stack.py), and the per-frame counts of every
source are one device count per tensor (an integer index_add_: torch.bincount reads its maximum back), not the reference's
per-frame `.sum()` loops.  The keypoints of all frames come from one launch of the stacked FPS kernel
(ops.stack_furthest_point_sample, mode "frames": frames differ in point count, and the counts stay on the device), so
`forward` makes NO device-to-host copy; DF3D_VSA_STACK_FPS=0 keeps the per-frame ops.furthest_point_sample calls, which read
the frames' point counts back once.  `sector_fps` is the reference's function of that name on the same kernel.

Sources are read as the reference reads them: rows stacked frame after frame (ascending batch index), which is how pcdet's
collate and the sparse convolutions of this package leave them.

Not provided, refused by name: SAMPLE_METHOD SPC (sectorized proposal-centric sampling), FILTER_NEIGHBOR_WITH_ROI and the
vector-pool aggregation.  The keypoint scores PVRCNNHead reads (`point_cls_scores`) come from PointHeadSimple
(dualfusion/dense_heads.py); the PVRCNN detector (dualfusion/vr_detector.py) strings the modules together."""
import math
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .pointnet2_stack import build_local_aggregation_module, frame_counts
from .registry import PFE
from .roi_heads import _get, get_voxel_centers


def _need(cfg, key):
    v = _get(cfg, key)
    if v is None:
        raise KeyError("VoxelSetAbstraction: the config has no %s" % key)
    return v


def pad_keypoint_indices(non_empty, num_keypoints):
    """voxel_set_abstraction.py:258-261: a frame with fewer points than keypoints repeats its sampled order"""
    times = int(num_keypoints / non_empty.shape[0]) + 1
    return non_empty.repeat(times)[:num_keypoints]


def stack_fps_enabled():
    return os.environ.get("DF3D_VSA_STACK_FPS", "1") != "0"


def sector_fps(points, num_sampled_points, num_sectors):
    """voxel_set_abstraction.py:78-121, the second half of SPC keypoint sampling: points [N, 3] are split into
    `num_sectors` sectors by azimuth, sector s with n_s points gives min(n_s, ceil(n_s / N * num_sampled_points)) picks, and
    all sectors are sampled by ONE stacked launch -> sampled points [N_out, 3], sector after sector.

    The sector of a point as the reference computes it (atan2 + pi, divide, floor, clamp to [0, num_sectors]; a point that
    lands on `num_sectors` belongs to no sector there either), a stable sort by sector, the per-sector counts by index_add_
    and the pick counts in float64, all on the device; empty sectors are segments without rows and without picks.  One
    device-to-host read, of the output length (the reference makes one per sector).  If no sector has a point the
    reference samples the whole cloud as one segment; so does this."""
    sector_size = math.pi * 2 / num_sectors
    point_angles = torch.atan2(points[:, 1], points[:, 0]) + math.pi
    sector_idx = (point_angles / sector_size).floor().clamp(min=0, max=num_sectors).long()
    order = torch.argsort(sector_idx, stable=True)
    xyz = points[order].contiguous()
    ones = torch.ones(points.shape[0], dtype=torch.int32, device=points.device)
    cnt = torch.zeros(num_sectors + 1, dtype=torch.int32, device=points.device).index_add_(0, sector_idx, ones)[:num_sectors]
    ratio = cnt.double() / points.shape[0]
    num = torch.minimum(cnt, torch.ceil(ratio * num_sampled_points).int()).contiguous()
    idx = ops.stack_furthest_point_sample(xyz, cnt.contiguous(), num, mode="stack")
    if idx.shape[0] == 0:
        xyz = points.contiguous()
        idx = ops.stack_furthest_point_sample(xyz, ops.device_constant([points.shape[0]], torch.int32, points.device),
                                              int(num_sampled_points), mode="stack")
    return xyz[idx.long()]


@PFE.register_module
class VoxelSetAbstraction(nn.Module):
    def __init__(self, model_cfg, voxel_size, point_cloud_range, num_bev_features=None, num_rawpoint_features=None, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.voxel_size = [float(v) for v in voxel_size]
        self.point_cloud_range = [float(v) for v in point_cloud_range]
        self.point_source = _need(model_cfg, "POINT_SOURCE")
        if self.point_source not in ("raw_points", "voxel_centers"):
            raise NotImplementedError("VoxelSetAbstraction: POINT_SOURCE %r (raw_points or voxel_centers)" % (self.point_source,))
        method = _need(model_cfg, "SAMPLE_METHOD")
        if method == "SPC":
            raise NotImplementedError("VoxelSetAbstraction: SAMPLE_METHOD SPC (sectorized proposal-centric sampling) is not "
                                      "provided; FPS is the method of every shipped PV-RCNN + 3D-DF config")
        if method != "FPS":
            raise NotImplementedError("VoxelSetAbstraction: SAMPLE_METHOD %r" % (method,))
        self.num_keypoints = int(_need(model_cfg, "NUM_KEYPOINTS"))
        self.features_source = list(_need(model_cfg, "FEATURES_SOURCE"))
        SA_cfg = _need(model_cfg, "SA_LAYER")

        self.SA_layers = nn.ModuleList()
        self.SA_layer_names = []
        self.downsample_times_map = {}
        c_in = 0
        for src_name in self.features_source:
            if src_name in ("bev", "raw_points"):
                continue
            cfg = SA_cfg[src_name]
            self._refuse_roi_filter(cfg, src_name)
            self.downsample_times_map[src_name] = _need(cfg, "DOWNSAMPLE_FACTOR")
            input_channels = _get(cfg, "INPUT_CHANNELS", None)
            if input_channels is None:
                first = _need(cfg, "MLPS")[0]
                input_channels = first[0] if isinstance(first, (list, tuple)) else first
            cur_layer, cur_num_c_out = build_local_aggregation_module(input_channels=input_channels, config=cfg)
            self.SA_layers.append(cur_layer)
            self.SA_layer_names.append(src_name)
            c_in += cur_num_c_out
        if "bev" in self.features_source:
            c_in += num_bev_features
        if "raw_points" in self.features_source:
            self._refuse_roi_filter(SA_cfg["raw_points"], "raw_points")
            self.SA_rawpoints, cur_num_c_out = build_local_aggregation_module(input_channels=num_rawpoint_features - 3,
                                                                              config=SA_cfg["raw_points"])
            c_in += cur_num_c_out
        out = int(_need(model_cfg, "NUM_OUTPUT_FEATURES"))
        self.vsa_point_feature_fusion = nn.Sequential(nn.Linear(c_in, out, bias=False), nn.BatchNorm1d(out), nn.ReLU())
        self.num_point_features = out
        self.num_point_features_before_fusion = c_in

    @staticmethod
    def _refuse_roi_filter(cfg, src_name):
        if _get(cfg, "FILTER_NEIGHBOR_WITH_ROI", False):
            raise NotImplementedError("VoxelSetAbstraction: FILTER_NEIGHBOR_WITH_ROI (SA_LAYER.%s) is not provided" % src_name)

    def interpolate_from_bev_features(self, keypoints, bev_features, batch_size, bev_stride):
        """keypoints [M, 4] (b, x, y, z), bev_features [B, C, H, W] -> [M, C], all frames in one launch"""
        return ops.bev_interpolate(keypoints.contiguous(), bev_features.contiguous(), self.point_cloud_range, self.voxel_size,
                                   bev_stride)

    def get_sampled_points(self, batch_dict):
        """-> keypoints [B * NUM_KEYPOINTS, 4] (b, x, y, z).

        Stacked path (the default; read per call): the frames' rows in frame order, their counts on the device, ONE
        `frames`-mode launch of ops.stack_furthest_point_sample with NUM_KEYPOINTS picks for every frame, one gather.  No
        device-to-host copy.  It therefore cannot raise on an empty frame: that frame's keypoint rows come out as NaN
        (its indices are -1).

        DF3D_VSA_STACK_FPS=0: one ops.furthest_point_sample call per frame, sized by the frames' point counts, which are
        read back (the one device-to-host copy of `forward` on that path); an empty frame raises ValueError."""
        batch_size = batch_dict["batch_size"]
        if self.point_source == "raw_points":
            src_points = batch_dict["points"][:, 1:4]
            batch_indices = batch_dict["points"][:, 0].long()
        else:
            src_points = get_voxel_centers(batch_dict["voxel_coords"][:, 1:4], 1, self.voxel_size, self.point_cloud_range)
            batch_indices = batch_dict["voxel_coords"][:, 0].long()
        # the frames' rows in their order, frame after frame (what the reference's boolean masks select), without a
        # compaction per frame
        order = torch.argsort(batch_indices, stable=True)
        src_points = src_points[order].contiguous()
        K = self.num_keypoints
        if stack_fps_enabled():
            num = torch.full((batch_size,), K, dtype=torch.int32, device=src_points.device)
            idx = ops.stack_furthest_point_sample(src_points, frame_counts(batch_indices, batch_size), num,
                                                  total=batch_size * K, mode="frames")
            keypoints = src_points[idx.clamp(min=0).long()]
            keypoints = torch.where((idx < 0)[:, None], keypoints.new_full((), float("nan")), keypoints)
            batch_idx = torch.arange(batch_size, device=keypoints.device).view(-1, 1).repeat(1, K).view(-1, 1)
            return torch.cat((batch_idx.float(), keypoints), dim=1)
        counts = frame_counts(batch_indices, batch_size).tolist()
        keypoints_list, start = [], 0
        for bs_idx in range(batch_size):
            n = counts[bs_idx]
            if n == 0:
                raise ValueError("VoxelSetAbstraction: frame %d has no points to sample keypoints from" % bs_idx)
            sampled_points = src_points[start:start + n]
            start += n
            # the first min(n, K) picks of a K-pick FPS: the reference overwrites the rest (voxel_set_abstraction.py:258-261)
            cur_pt_idxs = ops.furthest_point_sample(sampled_points.unsqueeze(0), min(n, K))[0].long()
            if n < K:
                cur_pt_idxs = pad_keypoint_indices(cur_pt_idxs, K)
            keypoints_list.append(sampled_points[cur_pt_idxs])
        keypoints = torch.cat(keypoints_list, dim=0)
        batch_idx = torch.arange(batch_size, device=keypoints.device).view(-1, 1).repeat(1, K).view(-1, 1)
        return torch.cat((batch_idx.float(), keypoints), dim=1)

    @staticmethod
    def aggregate_keypoint_features_from_one_source(batch_size, aggregate_func, xyz, xyz_features, xyz_bs_idxs, new_xyz,
                                                    new_xyz_batch_cnt):
        xyz_batch_cnt = frame_counts(xyz_bs_idxs, batch_size)
        _, pooled_features = aggregate_func(
            xyz=xyz.contiguous(), xyz_batch_cnt=xyz_batch_cnt, new_xyz=new_xyz, new_xyz_batch_cnt=new_xyz_batch_cnt,
            features=xyz_features.contiguous() if xyz_features is not None else None)
        return pooled_features

    def forward(self, batch_dict):
        """batch_dict: batch_size, points [N, 1 + 3 + C] (b, x, y, z, ..) and / or voxel_coords, spatial_features [B, C, H, W]
        with spatial_features_stride, multi_scale_3d_features {x_conv*: SparseConvTensor} -> point_features_before_fusion
        [B * K, C_in], point_features [B * K, NUM_OUTPUT_FEATURES], point_coords [B * K, 4]."""
        keypoints = self.get_sampled_points(batch_dict)
        batch_size = batch_dict["batch_size"]
        point_features_list = []
        if "bev" in self.features_source:
            point_features_list.append(self.interpolate_from_bev_features(
                keypoints, batch_dict["spatial_features"], batch_size, bev_stride=batch_dict["spatial_features_stride"]))
        new_xyz = keypoints[:, 1:4].contiguous()
        new_xyz_batch_cnt = torch.full((batch_size,), self.num_keypoints, dtype=torch.int32, device=new_xyz.device)
        if "raw_points" in self.features_source:
            raw_points = batch_dict["points"]
            point_features_list.append(self.aggregate_keypoint_features_from_one_source(
                batch_size=batch_size, aggregate_func=self.SA_rawpoints, xyz=raw_points[:, 1:4],
                xyz_features=raw_points[:, 4:] if raw_points.shape[1] > 4 else None, xyz_bs_idxs=raw_points[:, 0],
                new_xyz=new_xyz, new_xyz_batch_cnt=new_xyz_batch_cnt))
        for k, src_name in enumerate(self.SA_layer_names):
            cur = batch_dict["multi_scale_3d_features"][src_name]
            cur_coords = cur.indices
            xyz = get_voxel_centers(cur_coords[:, 1:4], self.downsample_times_map[src_name], self.voxel_size,
                                    self.point_cloud_range)
            point_features_list.append(self.aggregate_keypoint_features_from_one_source(
                batch_size=batch_size, aggregate_func=self.SA_layers[k], xyz=xyz, xyz_features=cur.features,
                xyz_bs_idxs=cur_coords[:, 0], new_xyz=new_xyz, new_xyz_batch_cnt=new_xyz_batch_cnt))
        point_features = torch.cat(point_features_list, dim=-1)
        batch_dict["point_features_before_fusion"] = point_features
        fc, bn = self.vsa_point_feature_fusion[0], self.vsa_point_feature_fusion[1]
        batch_dict["point_features"] = ops.batch_norm_rows(bn, F.linear(point_features, fc.weight), relu=True)
        batch_dict["point_coords"] = keypoints
        return batch_dict
