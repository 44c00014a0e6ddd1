"""TransFusion-tree camera fusion layer `ACTR` (registry FUSION_LAYERS; reference
TF/mmdet3d/models/fusion_layers/point_fusion.py:315-643).

The reference projects voxel centres with per-sample nuScenes-devkit DB lookups on the CPU
(lidar -> ego -> global -> ego_cam -> cam, :551-643) and cannot run without the dataset on disk
(SURVEY.md Appendix C item 12).  This layer takes the equivalent per-camera 4x4 `lidar2cam` and 3x3
`cam_intrinsic` (or a 4x4 `lidar2img`) from `img_metas` and does everything on the device, batched:
  visibility   depth > 1, 1 < u < W_ori-1, 1 < v < H_ori-1 on the ORIGINAL image (:612-617)
  image coords u,v * scale_factor - crop_offset [flip]; normalised by the padded input shape (:519-540)
  assignment   a voxel seen by several cameras goes to the LAST one; unseen voxels stay with camera 0
               at (0, 0) and still form queries (:544-547, Appendix C item 6)
  per-query image feature = level-0 map at (pixel // 4) (:375-378)
  write-back   pts_feats + enh (fusion_method 'sum'), one contribution per voxel (:482-491)
"""
import os

import torch
from torch import nn

from .actr import build as build_actr
from .registry import FUSION_LAYERS


@FUSION_LAYERS.register_module(name="ACTR")
class ACTRFusionLayer(nn.Module):
    def __init__(self, pfat_cfg, init_cfg=None, lt_cfg=None, coord_type='LIDAR', activate_out=False,
                 data_version='v1.0-trainval', data_root='./data/nuscenes', model_name='ACTR', num_cams=6):
        super().__init__()
        self.fusion_method = pfat_cfg['fusion_method']
        if self.fusion_method not in ('sum', 'replace', 'concat'):
            raise NotImplementedError("fusion_method %r" % self.fusion_method)
        self.actr = build_actr(pfat_cfg, lt_cfg=lt_cfg, model_name=model_name)
        self.coord_type = coord_type
        self.activate_out = activate_out
        self.num_cams = num_cams

    # ------------------------------------------------------------------ geometry
    @staticmethod
    def _calib(img_metas, dev):
        import numpy as np
        from . import ops as _ops
        # cached by value (ops.device_constant): a per-call host -> device copy drains the stream first
        l2c = _ops.device_constant(np.stack([np.asarray(m['lidar2cam'], np.float32) for m in img_metas]), torch.float32, dev)  # [B,6,4,4]
        K = _ops.device_constant(np.stack([np.asarray(m['cam_intrinsic'], np.float32) for m in img_metas]), torch.float32, dev)  # [B,6,3,3]
        return l2c, K

    @staticmethod
    def _undo_3d_augmentation(xyz, b, img_metas):
        """The points the cameras saw: the 3-D augmentations recorded in `img_meta` are undone in reverse order before
        the projection, `apply_3d_transformation(points, 'LIDAR', img_meta, reverse=True)` of the reference
        (TF/mmdet3d/models/fusion_layers/coord_transform.py:6-94 over core/points/base_points.py:77-141,199-205,
        lidar_points.py:28-33): 'T' subtracts pcd_trans, 'S' multiplies by 1 / pcd_scale_factor, 'R' multiplies the
        row vectors by the inverse of pcd_rotation, 'HF' / 'VF' negate y / x when the sample was flipped."""
        if not any(m.get('transformation_3d_flow') for m in img_metas):
            return xyz
        xyz = xyz.clone()
        for i, m in enumerate(img_metas):
            flow = list(m.get('transformation_3d_flow', []))
            if not flow:
                continue
            sel = (b == i).nonzero(as_tuple=True)[0]
            x = xyz[sel]
            rot = torch.as_tensor(m['pcd_rotation'], dtype=x.dtype, device=x.device) if 'pcd_rotation' in m \
                else torch.eye(3, dtype=x.dtype, device=x.device)
            trans = torch.as_tensor(m['pcd_trans'], dtype=x.dtype, device=x.device) if 'pcd_trans' in m \
                else torch.zeros(3, dtype=x.dtype, device=x.device)
            scale = m.get('pcd_scale_factor', 1.)
            for op in flow[::-1]:
                if op == 'T':
                    x = x + (-trans)
                elif op == 'S':
                    x = x * (1.0 / scale)
                elif op == 'R':
                    x = x @ rot.inverse()
                elif op == 'HF':
                    if m.get('pcd_horizontal_flip', False):
                        x = x * x.new_tensor([1.0, -1.0, 1.0])
                elif op == 'VF':
                    if m.get('pcd_vertical_flip', False):
                        x = x * x.new_tensor([-1.0, 1.0, 1.0])
                else:
                    raise ValueError("This 3D data transformation op (%s) is not supported" % op)
            xyz[sel] = x
        return xyz

    def project(self, pts, img_metas):
        """pts [N,4] (b,x,y,z) batch-sorted -> cam_id [N] int64, coor_norm [N,2], coor_pix [N,2] (input-image px)."""
        dev = pts.device
        l2c, K = self._calib(img_metas, dev)
        b = pts[:, 0].long()
        xyz = self._undo_3d_augmentation(pts[:, 1:4], b, img_metas)
        xyz1 = torch.cat([xyz, torch.ones_like(pts[:, :1])], 1)                      # [N,4]
        # broadcast multiply-sum instead of einsum: einsum lowers to a batched GEMM over N*6 tiny 3x4 matrices
        # (9 ms at nuScenes size); this is two element-wise passes
        cam = (l2c[b][:, :, :3, :] * xyz1[:, None, None, :]).sum(-1)                 # [N,6,3]
        depth = cam[..., 2]
        uvw = (K[b] * cam[:, :, None, :]).sum(-1)
        u = uvw[..., 0] / uvw[..., 2]
        v = uvw[..., 1] / uvw[..., 2]
        from . import ops as _ops
        const = lambda v, dt=torch.float32: _ops.device_constant(v, dt, dev)         # noqa: E731  (cached by value)
        ori = const([[m['ori_shape'][0], m['ori_shape'][1]] for m in img_metas])
        H = ori[b, 0][:, None]
        W = ori[b, 1][:, None]
        vis = (depth > 1.0) & (u > 1) & (u < W - 1) & (v > 1) & (v < H - 1)
        sf = const([[float(v) for v in list(m.get('scale_factor', [1.0, 1.0]))[:2]] for m in img_metas])
        off = const([[float(v) for v in list(m.get('img_crop_offset', [0.0, 0.0]))[:2]]
                     if not isinstance(m.get('img_crop_offset', 0), (int, float))
                     else [float(m.get('img_crop_offset', 0))] * 2 for m in img_metas])
        x = u * sf[b, 0][:, None] - off[b, 0][:, None]
        y = v * sf[b, 1][:, None] - off[b, 1][:, None]
        flip = const([bool(m.get('flip', False)) for m in img_metas], torch.bool)
        iw = const([float(m['img_shape'][1]) for m in img_metas])
        x = torch.where(flip[b][:, None], iw[b][:, None] - x, x)
        pad = const([[float(m['input_shape'][0]), float(m['input_shape'][1])] for m in img_metas])
        # last visible camera wins; none -> camera 0 at (0,0)
        ncam = vis.shape[1]
        order = torch.arange(1, ncam + 1, device=dev)[None, :] * vis.long()
        last = order.max(1)[0]                                                        # 0 = unseen
        cam_id = (last - 1).clamp(min=0)
        seen = last > 0
        gx = torch.gather(x, 1, cam_id[:, None])[:, 0]
        gy = torch.gather(y, 1, cam_id[:, None])[:, 0]
        pix = torch.stack([torch.where(seen, gx, torch.zeros_like(gx)), torch.where(seen, gy, torch.zeros_like(gy))], 1)
        norm = torch.stack([pix[:, 0] / pad[b, 1], pix[:, 1] / pad[b, 0]], 1)
        return cam_id, norm, pix

    def assemble(self, img_feats, pts, pts_feats, cam_id, norm, pix, batch_size):
        """split_param (:342-382) without the Python double loop: per (b, cam) zero-padded query sets."""
        dev = pts.device
        N6 = batch_size * self.num_cams
        b = pts[:, 0].long()
        seg = b * self.num_cams + cam_id                                              # [N] image index
        counts = torch.bincount(seg, minlength=N6)
        max_pts = int(counts.max().item()) if seg.numel() else 0                      # host sync (the reference's too)
        # slot = rank of the row among rows of the same segment, in row order
        order = torch.argsort(seg, stable=True)
        starts = torch.cumsum(counts, 0) - counts
        slot = torch.empty_like(seg)
        slot[order] = torch.arange(seg.numel(), device=dev) - starts[seg[order]]
        C = pts_feats.shape[1]
        IC = img_feats[0].shape[1]
        v_feat = pts_feats.new_zeros((N6, max_pts, C))
        v_i_feat = pts_feats.new_zeros((N6, max_pts, IC))
        grid = pts_feats.new_zeros((N6, max_pts, 2))
        qpts = pts_feats.new_zeros((N6, max_pts, 3))
        v_feat[seg, slot] = pts_feats
        grid[seg, slot] = norm
        qpts[seg, slot] = pts[:, 1:4]                    # the reference keeps the AUGMENTED points as lidar_grid (pts_b, :441)
        ic = (pix.to(torch.long) // 4)
        v_i_feat[seg, slot] = img_feats[0][seg, :, ic[:, 1], ic[:, 0]]
        return v_feat, v_i_feat, grid, qpts, seg, slot

    def _forward_native(self, img_feats, pts, pts_feats, cam_id, norm, pix, batch_size):
        """split_param / agg_param on the kernels of the CenterPoint adapter (csrc/fusion.hip) instead of advanced
        indexing: every voxel belongs to exactly one (sample, camera) list, so the per-camera visibility mask is
        one-hot; slots by df3d_query_slots, query tensors (LiDAR rows, image features at pixel // 4 gathered from the
        channel-first maps, points, depth position embedding) by df3d_assemble_queries2 with only the padding rows
        cleared, the additive write-back by df3d_fusion_writeback.  One host round trip (the longest list), as the
        reference has."""
        import ctypes
        from . import _lib
        from . import ops as _ops
        lib = _lib.load()
        P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)   # noqa: E731
        dev = pts.device
        n, C = pts_feats.shape
        ncam = self.num_cams
        f0 = img_feats[0].contiguous()
        NI, Ci, H, W = f0.shape
        cams = torch.arange(ncam, device=dev, dtype=cam_id.dtype)
        mask = (cam_id[None, :] == cams[:, None]).to(torch.uint8).contiguous()                 # [ncam, n] one-hot
        ic = (pix.to(torch.long) // 4).to(torch.int32)
        grid = ic[None].expand(ncam, n, 2).contiguous()
        ind = torch.zeros((n, 4), dtype=torch.int32, device=dev)
        ind[:, 0] = pts[:, 0].to(torch.int32)
        pinv = pts[:, 1:4].contiguous()
        pos = torch.empty((ncam, n), dtype=torch.int32, device=dev)
        counts = torch.empty((batch_size * ncam,), dtype=torch.int32, device=dev)
        lib.df3d_query_slots(P(mask), P(ind), n, batch_size, ncam, P(pos), P(counts), _ops._stream())
        max_ne = int(counts.max().item()) if n > 0 else 0                                      # the one host sync
        N6 = batch_size * ncam
        v_feat = torch.empty((N6, max_ne, C), dtype=torch.float32, device=dev)
        v_i_feat = torch.empty((N6, max_ne, Ci), dtype=torch.float32, device=dev)
        qgrid = torch.empty((N6, max_ne, 2), dtype=torch.float32, device=dev)
        qpts = torch.empty((N6, max_ne, 3), dtype=torch.float32, device=dev)
        depth_pos = self.actr.pos_encode_method == "depth" and C % 2 == 0
        qpos = torch.empty((N6, max_ne, C), dtype=torch.float32, device=dev) if depth_pos else None
        lib.df3d_assemble_queries2(P(pts_feats), P(pinv), P(ind), P(grid), P(mask), P(pos), P(f0), None, None, n, C,
                                   Ci, batch_size, ncam, H, W, max_ne, P(v_feat), P(v_i_feat), P(qgrid), P(qpts),
                                   P(qpos), P(counts), _ops._stream())
        # the reference's query coordinates are the un-truncated image coordinates over the padded input shape
        # (coor_2d, :538-546), not pixel centres of the feature map: overwrite the kernel's integer-grid values
        seg = pts[:, 0].long() * ncam + cam_id
        slot = pos[cam_id, torch.arange(n, device=dev)].long()
        qgrid[seg, slot] = norm
        enh = self._actr(v_feat, qgrid, [f0], qpts, v_i_feat, q_pos=qpos).contiguous()
        out = torch.empty_like(pts_feats)
        lib.df3d_fusion_writeback(P(pts_feats), P(enh), P(ind), P(mask), P(pos), n, C, ncam, max_ne, P(out),
                                  _ops._stream())
        return out

    def _forward_autograd(self, img_feats, pts, pts_feats, cam_id, norm, pix, batch_size):
        """Training formulation of `_forward_native` (the per-rank body of BASELINE configs[3]): the integer work -- one-hot
        (sample, camera) lists, query slots (df3d_query_slots), the image-feature / point gathers of the assembly kernel --
        runs on the same native kernels without gradients (none of it depends on a learnable value); the floating-point
        stages are differentiable: the LiDAR rows enter their slots by index_put (gradient = a gather), ACTR runs its
        module path (input projection as chunked batched products, GroupNorm, dual-query layers with the deformable
        sampling and its backward on csrc/msda.hip), the additive write-back reads every voxel's one slot.  Same values as
        `_forward_native` up to summation order."""
        import ctypes
        from . import _lib
        from . import ops as _ops
        lib = _lib.load()
        P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)   # noqa: E731
        dev = pts.device
        n, C = pts_feats.shape
        ncam = self.num_cams
        f0 = img_feats[0].contiguous()
        NI, Ci, H, W = f0.shape
        N6 = batch_size * ncam
        with torch.no_grad():
            cams = torch.arange(ncam, device=dev, dtype=cam_id.dtype)
            mask = (cam_id[None, :] == cams[:, None]).to(torch.uint8).contiguous()
            ic = (pix.to(torch.long) // 4).to(torch.int32)
            grid = ic[None].expand(ncam, n, 2).contiguous()
            ind = torch.zeros((n, 4), dtype=torch.int32, device=dev)
            ind[:, 0] = pts[:, 0].to(torch.int32)
            pinv = pts[:, 1:4].contiguous()
            pos = torch.empty((ncam, n), dtype=torch.int32, device=dev)
            counts = torch.empty((N6,), dtype=torch.int32, device=dev)
            lib.df3d_query_slots(P(mask), P(ind), n, batch_size, ncam, P(pos), P(counts), _ops._stream())
            max_ne = int(counts.max().item()) if n > 0 else 0                                  # the one host sync
            rows_nograd = pts_feats.detach().contiguous()
            v_feat0 = torch.empty((N6, max_ne, C), dtype=torch.float32, device=dev)
            v_i_feat = torch.empty((N6, max_ne, Ci), dtype=torch.float32, device=dev)
            qgrid = torch.empty((N6, max_ne, 2), dtype=torch.float32, device=dev)
            qpts = torch.empty((N6, max_ne, 3), dtype=torch.float32, device=dev)
            lib.df3d_assemble_queries2(P(rows_nograd), P(pinv), P(ind), P(grid), P(mask), P(pos), P(f0), None, None,
                                       n, C, Ci, batch_size, ncam, H, W, max_ne, P(v_feat0), P(v_i_feat), P(qgrid),
                                       P(qpts), None, P(counts), _ops._stream())
            seg = pts[:, 0].long() * ncam + cam_id
            slot = pos[cam_id, torch.arange(n, device=dev)].long()
            qgrid[seg, slot] = norm                    # the un-truncated image coordinates (see _forward_native)
        # the LiDAR rows with their gradient path: zeros + index_put (every (seg, slot) pair is distinct)
        v_feat = torch.zeros_like(v_feat0).index_put((seg, slot), pts_feats)
        enh = self._actr(v_feat, qgrid, [f0], qpts, v_i_feat)
        return pts_feats + enh[seg, slot]

    def _actr(self, v_feat, grid, img_feats, qpts, v_i_feat, q_pos=None):
        """ACTR on the assembled queries.  Inference with the 3D-DF configuration (one 256-channel level, two dual-query
        layers) takes the fold-through path of the CenterPoint adapter: the input projection runs on the matrix cores
        straight from the channel-first camera maps (csrc/imgproj.hip) and GroupNorm + both value projections are
        one folded GEMM -- no [B*6, 256, H, W] permute / copy, no normalised image map (the module composition made
        five 550 MB copies per step at bs = 4)."""
        from . import ops as _ops
        f0 = img_feats[0]
        actr = self.actr
        if (len(img_feats) == 1 and f0.is_cuda and f0.dtype == torch.float32 and f0.is_contiguous() and actr.can_fold()
                and len(actr.transformer.encoder.layers) == 2 and f0.shape[1] == 256
                and _ops.imgproj_supported(actr.input_proj[0][0].weight.shape[0], 256, actr.input_proj[0][1].num_channels)
                and os.environ.get("DF3D_IMGPROJ", "1") == "1"):
            NI, Ci, H, W = f0.shape
            w = actr.input_proj[0][0].weight
            packed = _ops.derived(self.__dict__, "_wpack", (w,), lambda: _ops.imgproj_pack(w[:, :, 0, 0].contiguous()))
            pkey = (f0.data_ptr(), NI, Ci * H * W)
            if getattr(self, "_ptrs", None) is None or self._ptrs[0] != pkey:
                base, step = f0.data_ptr(), Ci * H * W * 4
                self._ptrs = (pkey, torch.tensor([base + i * step for i in range(NI)], dtype=torch.int64, device=f0.device))
            u, _ = _ops.imgproj_split(self._ptrs[1], NI, Ci, H * W, packed)
            return actr.forward_folded(v_feat, grid, u, None, (H, W), v_i_feat, qpts, q_pos=q_pos)
        return actr(v_feat=v_feat, grid=grid, i_feats=img_feats, lidar_grid=qpts, v_i_feat=v_i_feat)

    def forward(self, img_feats, pts, pts_feats, img_metas, imgs=None):
        """pts: [N,4] (b,x,y,z) tensor from SparseEncoderFusion.coor2pts (or the reference's list of
        per-sample [n_b,3] tensors); pts_feats [N,C].  Returns fused [N,C]."""
        if isinstance(pts, (list, tuple)):
            pts = torch.cat([torch.cat([p.new_full((p.shape[0], 1), i), p[:, :3]], 1) for i, p in enumerate(pts)])
        batch_size = len(img_metas)
        img_feats = list(img_feats[:self.actr.num_backbone_outs])
        # the image coordinates index the level-0 map at stride 4 (point_fusion.py:366): a map of another stride
        # would be read out of bounds
        fh, fw = img_feats[0].shape[-2:]
        ih, iw = img_metas[0]['input_shape'][:2]
        if fh * 4 < ih or fw * 4 < iw:
            raise ValueError("ACTRFusionLayer expects the stride-4 camera feature map: input %dx%d needs at least "
                             "%dx%d, got %dx%d" % (ih, iw, -(-ih // 4), -(-iw // 4), fh, fw))
        cam_id, norm, pix = self.project(pts, img_metas)
        if (pts_feats.is_cuda and pts_feats.dtype == torch.float32 and self.fusion_method == 'sum' and not self.activate_out
                and not torch.is_grad_enabled() and len(img_feats) == 1 and img_feats[0].dtype == torch.float32
                and os.environ.get("DF3D_TF_NATIVE_ASSEMBLE", "1") == "1"):
            return self._forward_native(img_feats, pts, pts_feats.contiguous(), cam_id, norm, pix, batch_size)
        if (pts_feats.is_cuda and pts_feats.dtype == torch.float32 and self.fusion_method == 'sum' and not self.activate_out
                and torch.is_grad_enabled() and len(img_feats) == 1 and img_feats[0].dtype == torch.float32
                and not img_feats[0].requires_grad and os.environ.get("DF3D_TF_NATIVE_ASSEMBLE", "1") == "1"):
            return self._forward_autograd(img_feats, pts, pts_feats.contiguous(), cam_id, norm, pix, batch_size)
        v_feat, v_i_feat, grid, qpts, seg, slot = self.assemble(img_feats, pts, pts_feats, cam_id, norm, pix, batch_size)
        enh = self._actr(v_feat, grid, img_feats, qpts, v_i_feat)
        enh_cat = enh[seg, slot]
        if self.fusion_method == 'replace':
            out = enh_cat
        elif self.fusion_method == 'concat':
            out = torch.cat((pts_feats, enh_cat), dim=1)
        else:
            out = pts_feats + enh_cat
        return torch.relu(out) if self.activate_out else out
