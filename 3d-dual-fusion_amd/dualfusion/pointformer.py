"""3-D local self-attention over the LiDAR queries (ACTRv2): `LocalTransformer`
(reference: CP/det3d/models/model_utils/pointformer.py:250-380; pre-norm encoder layer :10-44;
helpers CP/det3d/ops/furthest_point_sample/points_sampler.py:34-115,
CP/det3d/ops/group_points/group_points.py:11-131).

Pipeline: D-FPS of npoint centres -> ball query (radius, nsample) -> group features and ABSOLUTE
xyz -> position-encoding MLP (1x1 conv + BN2d + ReLU, 1x1 conv) -> `num_layers` pre-norm MHA
encoder layers over each group (sequence = nsample, batch = B*npoint) -> scatter the transformed
group features back to the points.  Index ops are the HIP kernels of csrc/pointops.hip.  Inference runs
the fused layer kernels (csrc/ltlayer.hip) or the row kernels; under grad the module takes the same row
layout from differentiable pieces (`_forward_train_rows`: row kernels with their own backward, the
attention inside a group through df3d_group_attention / _backward); configurations those do not serve
keep the torch composition of the layer.  Parameter names follow the reference (`pe.0.conv`, `pe.0.bn`,
`pe.1.conv`, `chunk.layers.j.{self_attn,linear1,linear2,norm1,norm2}`), SURVEY.md Appendix B.
"""
import copy
import os

import threading
import weakref

import torch
import torch.nn.functional as F
from torch import nn

from . import ops as _ops


_GEO = threading.local()          # last LocalTransformer geometry of this host thread (see LocalTransformer._geometry)


class ConvModule(nn.Module):
    """The two mmcv.cnn.ConvModule configurations LocalTransformer uses (pointformer.py:287-290):
    conv(bias = no norm) [-> BN2d] [-> ReLU], sub-module names `conv` / `bn` / `activate`."""

    def __init__(self, in_channels, out_channels, kernel_size, norm_cfg=None, act_cfg=dict(type='ReLU')):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size, bias=norm_cfg is None)
        self.with_norm = norm_cfg is not None
        self.with_activation = act_cfg is not None
        if self.with_norm:
            self.bn = nn.BatchNorm2d(out_channels)
        if self.with_activation:
            self.activate = nn.ReLU(inplace=True)

    def forward(self, x):
        x = self.conv(x)
        if self.with_norm:
            x = self.bn(x)
        if self.with_activation:
            x = self.activate(x)
        return x


class TransformerEncoderLayerPreNorm(nn.Module):
    """pointformer.py:10-44: x = LN1(x); x = x + MHA(x); x = LN2(x); x = x + FFN(x)."""

    def __init__(self, d_model, nhead, dim_feedforward=2048, dropout=0.1, activation="relu"):
        super().__init__()
        self.self_attn = nn.MultiheadAttention(d_model, nhead, dropout=dropout)
        self.linear1 = nn.Linear(d_model, dim_feedforward)
        self.dropout = nn.Dropout(dropout, inplace=True)
        self.linear2 = nn.Linear(dim_feedforward, d_model)
        self.norm1 = nn.LayerNorm(d_model)
        self.norm2 = nn.LayerNorm(d_model)
        self.dropout1 = nn.Dropout(dropout, inplace=True)
        self.dropout2 = nn.Dropout(dropout, inplace=True)
        self.activation = nn.ReLU(inplace=True)

    def _rows_fit(self, src, src_mask, src_key_padding_mask):
        """The whole layer on row kernels: 64 channels, heads of 16, FFN 128, no masks (the ACTRv2 configuration)."""
        a = self.self_attn
        return (src_mask is None and src_key_padding_mask is None and _ops.CONV_PRECISION == "split" and src.dim() == 3
                and src.shape[-1] == 64 and a.embed_dim == 64 and a.head_dim == 16 and a._qkv_same_embed_dim
                and a.in_proj_bias is not None and _ops.ffn_supported(64, self.linear1.out_features)
                and src.shape[0] * a.num_heads <= 1024
                and src.shape[0] <= 64)

    def _fused_fit(self, src):
        """The whole layer as ONE kernel (csrc/ltlayer.hip): groups of 32 tokens, 4 heads of 16, feed-forward 128."""
        a = self.self_attn
        return (src.shape[0] == 32 and a.num_heads == 4 and self.linear1.out_features == 128 and src.is_contiguous()
                and self.linear1.bias is not None and self.linear2.bias is not None and a.out_proj.bias is not None
                and os.environ.get("DF3D_LT_FUSED", "1") == "1")

    def _packed_fused(self):
        a = self.self_attn
        ts = (a.in_proj_weight, a.in_proj_bias, a.out_proj.weight, a.out_proj.bias, self.linear1.weight, self.linear1.bias,
              self.linear2.weight, self.linear2.bias, self.norm1.weight, self.norm1.bias, self.norm2.weight, self.norm2.bias)
        return _ops.derived(self.__dict__, "_lt_packed", ts, lambda: tuple(_ops.lt_layer_pack(*ts)))

    def _forward_fused(self, src):
        pk, vc = self._packed_fused()
        return _ops.lt_layer(src, pk, vc, self.self_attn.num_heads, self.linear1.out_features, self.norm1.eps, self.norm2.eps)

    def _forward_rows(self, src):
        """LN1 -> in-projection (three 64-column banks of one grouped launch of the split-precision conv kernel over an
        identity table) -> `group_attention` -> out-projection -> LN2(x + .) -> FFN + residual (the fused feed-forward kernel,
        hidden activation in registers): fp32-grade products (bf16 hi + lo operands), no library GEMM (hipBLASLt
        runs these [524 k, 64] x [64, 64..192] fp32 products at ~20 TFLOP/s: 8 ms per Voxel-RCNN step) and no flash kernel
        on sequences of 32."""
        L, G, C = src.shape
        R = L * G
        a = self.self_attn
        ident = _ops.identity_table(R, src.device)
        x1, s1 = _ops.add_layernorm(src.reshape(R, C).contiguous(), None, self.norm1.weight, self.norm1.bias, self.norm1.eps,
                                    want_split=True)
        qkv, _ = _ops.conv_rows_split(s1, C, 0, _ops.packed_linear(a.in_proj_weight, 64), 64, 3, ident, R,
                                      a.in_proj_bias.detach())
        so = _ops.group_attention(qkv, L, G, a.num_heads, split_only=True)
        att, _ = _ops.sparse_conv_split(so, _ops.packed_linear(a.out_proj.weight), ident, R, C, C,
                                        bias=a.out_proj.bias.detach(), emit_split=False)
        x3 = _ops.add_layernorm(x1, att, self.norm2.weight, self.norm2.bias, self.norm2.eps)
        # FFN + residual: the fused feed-forward kernel (csrc/ffn.hip, 64-wide rows): the hidden activation stays in registers
        w1, w2 = self.linear1.weight, self.linear2.weight
        packed = _ops.derived(self.__dict__, "_ffn_packed", (w1, w2),
                              lambda: _ops.ffn_pack(w1.detach().contiguous(), w2.detach().contiguous()))
        out = _ops.ffn_fused(x3, packed, self.linear1.bias.detach(), self.linear2.bias.detach(), self.linear1.out_features,
                             residual=x3)
        return out.view(L, G, C)

    def forward(self, src, src_mask=None, src_key_padding_mask=None):
        if (src.is_cuda and src.dtype == torch.float32 and not self.training and not torch.is_grad_enabled()
                and self._rows_fit(src, src_mask, src_key_padding_mask)):
            if self._fused_fit(src):
                return self._forward_fused(src)
            return self._forward_rows(src)
        if (src.is_cuda and src.dtype == torch.float32 and not self.training and not torch.is_grad_enabled()
                and src.shape[-1] % 4 == 0):
            # the row kernel of csrc/actr.hip (one wave per row, residual add fused): torch's LayerNorm runs at
            # ~0.5 TB/s on these [32 * B * npoint, 64] rows (9 ms per step in the Voxel-RCNN tree)
            src = _ops.add_layernorm(src.contiguous(), None, self.norm1.weight, self.norm1.bias, self.norm1.eps)
            src2, _ = self.self_attn(src, src, src, attn_mask=src_mask, key_padding_mask=src_key_padding_mask,
                                     need_weights=False)
            src = _ops.add_layernorm(src, src2.contiguous(), self.norm2.weight, self.norm2.bias, self.norm2.eps)
            src2 = self.linear2(self.activation(self.linear1(src)))
            return src + src2
        if self._train_rows_fit(src, src_mask, src_key_padding_mask):
            return self._forward_train_rows(src)
        return self._forward_torch(src, src_mask, src_key_padding_mask)

    def _train_rows_fit(self, src, src_mask, src_key_padding_mask):
        """Under grad, the layer on the row kernels with backward kernels: fp32 GPU rows, heads of 16 channels, no masks, no
        active dropout (LocalTransformer builds drop = 0.0).  Follows from the module and the tensor alone."""
        a = self.self_attn
        drops = a.dropout + self.dropout.p + self.dropout1.p + self.dropout2.p
        return (torch.is_grad_enabled() and src.is_cuda and src.dtype == torch.float32 and src.dim() == 3
                and not torch.is_autocast_enabled() and src_mask is None and src_key_padding_mask is None
                and (drops == 0 or not self.training) and a.head_dim == 16 and a._qkv_same_embed_dim and not a.batch_first
                and a.in_proj_bias is not None and a.bias_k is None and not a.add_zero_attn and src.shape[-1] == a.embed_dim
                and src.shape[-1] <= 1024 and src.shape[1] > 0
                and _ops.group_attention_backward_supported(src.shape[0], a.num_heads))

    def _forward_train_rows(self, src):
        """The layer under grad on [tokens * groups, C] rows, every step a kernel pair with its own backward: LN1
        (`layernorm_rows`) -> in-projection (`linear_rows_autograd`: chunked weight gradient) -> `group_attention` (backward
        recomputes the probabilities) -> out-projection -> LN2(x + .) (`dropout_add_layernorm`) -> linear1 -> ReLU in place
        (`relu_dropout_`) -> linear2 -> + residual.  Both residuals start from the NORMALISED tensor (the reference's pre-norm
        form, pointformer.py:34-43)."""
        L, G, C = src.shape
        a = self.self_attn
        x1 = _ops.layernorm_rows(src.reshape(L * G, C), self.norm1)
        qkv = _ops.linear_rows_autograd(x1, a.in_proj_weight, a.in_proj_bias)
        att = _ops.group_attention(qkv, L, G, a.num_heads)
        att = _ops.linear_rows_autograd(att, a.out_proj.weight, a.out_proj.bias)
        x3 = _ops.dropout_add_layernorm(x1, att, self.norm2, self.dropout1)
        h = _ops.linear_rows_autograd(x3, self.linear1.weight, self.linear1.bias)
        if h.requires_grad and h._base is None and _ops.relu_dropout_supported(h):
            h = _ops.relu_dropout_(h, 0.0)
        else:
            h = torch.relu(h)
        return (x3 + _ops.linear_rows_autograd(h, self.linear2.weight, self.linear2.bias)).view(L, G, C)

    def _forward_torch(self, src, src_mask=None, src_key_padding_mask=None):
        """The layer as the torch composition of its modules (any configuration: masks, dropout, heads of any size, CPU)."""
        src = self.norm1(src)
        src2, _ = self.self_attn(src, src, src, attn_mask=src_mask, key_padding_mask=src_key_padding_mask,
                                 need_weights=False)
        src = src + self.dropout1(src2)
        src = self.norm2(src)
        src2 = self.linear2(self.dropout(self.activation(self.linear1(src))))
        return src + self.dropout2(src2)


class _EncoderStack(nn.Module):
    """Holds `layers` like nn.TransformerEncoder (same state_dict keys `chunk.layers.j.*`) without
    its fast-path machinery, which does not accept custom layers."""

    def __init__(self, layer, num_layers):
        super().__init__()
        self.layers = nn.ModuleList([copy.deepcopy(layer) for _ in range(num_layers)])
        self.num_layers = num_layers

    def forward(self, x):
        for l in self.layers:
            x = l(x)
        return x


class LocalTransformer(nn.Module):
    def __init__(self, npoint, radius, nsample, dim_feature, dim_out, nhead=4, num_layers=2,
                 norm_cfg=dict(type="BN2d"), ratio=1, drop=0.0, prenorm=True, attn_feat_agg_method="unique",
                 feat_agg_method="replace"):
        super().__init__()
        if ratio != 1 or not prenorm:
            raise NotImplementedError("only the pre-norm, ratio=1 configuration used by ACTRv2 is implemented")
        self.npoint, self.nsample, self.radius = npoint, nsample, radius
        self.nc_in, self.nc_out = dim_feature, dim_out
        self.pe = nn.Sequential(ConvModule(3, self.nc_in // 2, 1, norm_cfg=norm_cfg),
                                ConvModule(self.nc_in // 2, self.nc_in, 1, act_cfg=None, norm_cfg=None))
        self.chunk = _EncoderStack(TransformerEncoderLayerPreNorm(d_model=self.nc_in, dim_feedforward=2 * self.nc_in,
                                                                  dropout=drop, nhead=nhead), num_layers)
        self.attn_feat_agg_method = attn_feat_agg_method
        self.feat_agg_method = feat_agg_method

    @staticmethod
    def _winner(idx_flat, n_points):
        """Per point id the flat group position whose feature is kept by the reference's
        `unique_idx` (pointformer.py:320-328): scatter_ of flipped (inverse, perm) pairs keeps, for a
        sequential scatter, the LOWEST flat position of each id.  -1 where a point is in no group."""
        B, L = idx_flat.shape
        pos = torch.arange(L, device=idx_flat.device, dtype=torch.int64).expand(B, L)
        win = torch.full((B, n_points), L, dtype=torch.int64, device=idx_flat.device)
        win.scatter_reduce_(1, idx_flat.long(), pos, reduce="amin", include_self=True)
        return torch.where(win == L, torch.full_like(win, -1), win)

    def scatter(self, attn_features, feats, idxs):
        """attn_features [B,C,N] updated IN PLACE at the grouped point ids (pointformer.py:315-347)."""
        B, C, np_, ns = feats.shape
        N = attn_features.shape[2]
        idx_f = idxs.reshape(B, -1)
        feat_f = feats.reshape(B, C, -1)
        if self.attn_feat_agg_method == "unique":
            win = self._winner(idx_f, N)                                    # [B,N]
            has = win >= 0
            picked = torch.gather(feat_f, 2, win.clamp(min=0)[:, None, :].expand(B, C, N))
            attn_features.copy_(torch.where(has[:, None, :], picked, attn_features))
        elif self.attn_feat_agg_method == "sum":
            summed = torch.zeros_like(attn_features).scatter_add_(2, idx_f.long()[:, None, :].expand(B, C, -1), feat_f)
            cnt = torch.zeros((B, N), device=feats.device).scatter_add_(1, idx_f.long(),
                                                                        torch.ones_like(idx_f, dtype=torch.float32))
            attn_features.copy_(torch.where(cnt[:, None, :] > 0, (attn_features + summed) / cnt.clamp(min=1)[:, None, :],
                                            attn_features))
        else:
            raise NotImplementedError(self.attn_feat_agg_method)

    def _geometry(self, xyz_in):
        """FPS centres, ball-query neighbourhoods and grouped coordinates.  They depend on the point coordinates and on
        (npoint, radius, nsample) only, and the ACTRv2 encoder hands the SAME coordinate tensor to the LocalTransformer
        of every layer (actr_transformer.py:482-486): the result of the first layer is reused by the others (the
        reference recomputes it -- 2048 serial FPS iterations -- once per layer)."""
        key = (self.npoint, float(self.radius), self.nsample, xyz_in._version, tuple(xyz_in.shape))
        # a few entries: the geometry of the NEXT batch may be prepared (VoxelBackBone8xFusion.prefetch) before this batch's
        # layers ask for theirs
        entries = getattr(_GEO, "entries", None)
        if entries is None:
            entries = _GEO.entries = []
        if not torch.is_grad_enabled():
            for hit in entries:
                if hit[0]() is xyz_in and hit[1] == key:
                    return hit[2], hit[3]
        xyz = xyz_in.contiguous()
        fps_idx = _ops.furthest_point_sample(xyz, self.npoint)                          # [B,np]
        xyz_t = xyz.transpose(1, 2).contiguous()
        new_xyz = _ops.gather_points(xyz_t, fps_idx).transpose(1, 2).contiguous()       # [B,np,3]
        group_idx = _ops.ball_query(0.0, self.radius, self.nsample, xyz, new_xyz)       # [B,np,ns]
        group_xyz = _ops.group_points(xyz_t, group_idx)                                 # [B,3,np,ns] (absolute)
        if not torch.is_grad_enabled():
            entries[:] = [e for e in entries if e[0]() is not None][-3:]
            entries.append((weakref.ref(xyz_in), key, group_idx, group_xyz))
        return group_idx, group_xyz

    def _row_plan(self, xyz_in, group_idx, group_xyz):
        """Index tensors of the row-layout path, functions of the geometry alone (cached with it): gather rows of the
        grouped points in [ns, B*np] order, the grouped coordinates as rows, and for every point the row of the
        'unique' winner (lowest flat group position, pointformer.py:320-328) or -1."""
        rows = getattr(_GEO, "rows", None)
        if rows is None:
            rows = _GEO.rows = []
        for hit in rows:
            if hit[0] is group_idx:
                return hit[1]
        B, np_, ns = group_idx.shape
        N = xyz_in.shape[1]
        base = (torch.arange(B, device=group_idx.device, dtype=torch.int64) * N)[:, None, None]
        sel = (group_idx.long() + base).permute(2, 0, 1).reshape(-1)                    # [ns*B*np] rows of [B*N, C]
        gx = group_xyz.permute(3, 0, 2, 1).reshape(ns * B * np_, 3).contiguous()        # [ns*B*np, 3]
        win = self._winner(group_idx.reshape(B, -1), N)                                 # [B,N] flat (p, s) position
        has = win >= 0
        w = win.clamp(min=0)
        p_w, s_w = w // ns, w % ns
        src = s_w * (B * np_) + torch.arange(B, device=w.device)[:, None] * np_ + p_w   # row of y [ns*B*np, C]
        # the inverse map for the fused last layer: token row -> the point row it wins (or -1)
        # (no boolean-mask indexing: its size is a device -> host round trip, and this runs on the side stream behind the
        # 4.7 ms of furthest point sampling -- the host would sit there instead of queueing the backbone)
        R = ns * B * np_
        dst = torch.full((R + 1,), -1, dtype=torch.int64, device=w.device)
        dst.scatter_(0, torch.where(has.reshape(-1), src.reshape(-1), torch.full_like(src.reshape(-1), R)),
                     torch.arange(B * N, device=w.device))
        dst = dst[:R]
        plan = (sel, gx, src.reshape(-1), has.reshape(-1, 1), dst)
        del rows[:-3]
        rows.append((group_idx, plan))
        return plan

    def _pe_rows(self, gx):
        """self.pe (two 1x1 ConvModules, the first with BatchNorm2d + ReLU) on coordinate rows [R, 3] -> [R, C]."""
        c0, c1 = self.pe[0], self.pe[1]
        w0, b0 = c0.conv.weight[:, :, 0, 0], c0.conv.bias
        if c0.with_norm:
            inv = torch.rsqrt(c0.bn.running_var + c0.bn.eps) * c0.bn.weight
            w0 = w0 * inv[:, None]
            b0 = c0.bn.bias - c0.bn.running_mean * inv + (b0 * inv if b0 is not None else 0)
        h = F.linear(gx, w0, b0)
        if c0.with_activation:
            h = torch.relu_(h)
        return F.linear(h, c1.conv.weight[:, :, 0, 0], c1.conv.bias)

    def _pe_gather(self, flat, sel, gx):
        """flat[sel] + pe(gx): one kernel when the positional MLP has the usual form (BN folded + ReLU, then linear)."""
        c0, c1 = self.pe[0], self.pe[1]
        C = flat.shape[1]
        if not (c0.with_activation and c1.conv.bias is not None and C % 4 == 0 and 256 % (C // 4) == 0 and C <= 256):
            return flat.index_select(0, sel) + self._pe_rows(gx)
        w0, b0 = c0.conv.weight[:, :, 0, 0], c0.conv.bias
        if c0.with_norm:
            inv = torch.rsqrt(c0.bn.running_var + c0.bn.eps) * c0.bn.weight
            w0 = w0 * inv[:, None]
            b0 = c0.bn.bias - c0.bn.running_mean * inv + (b0 * inv if b0 is not None else 0)
        elif b0 is None:
            b0 = w0.new_zeros(w0.shape[0])
        return _ops.pe_gather_add(flat, sel, gx, w0.contiguous(), b0.contiguous(),
                                  c1.conv.weight[:, :, 0, 0].contiguous(), c1.conv.bias.contiguous())

    def _fused_chunk(self, flat, ns, groups):
        """(layers, first layer's fragments + positional MLP, its vector) when the chunk runs as fused launches, else None."""
        layers = list(self.chunk.layers)
        c0, c1 = self.pe[0], self.pe[1]
        probe = flat.new_empty((ns, 1, flat.shape[1]))
        if (len(layers) < 2 or flat.shape[1] != 64 or not flat.is_contiguous() or os.environ.get("DF3D_LT_GATHER", "1") != "1"
                or not all(l._rows_fit(probe, None, None) and l._fused_fit(probe) for l in layers)
                or not (c0.with_activation and c1.conv.bias is not None and c0.conv.out_channels == 32 and c0.conv.in_channels == 3)):
            return None
        ts = [c0.conv.weight, c0.conv.bias, c1.conv.weight, c1.conv.bias] + ([c0.bn.weight, c0.bn.bias, c0.bn.running_mean,
                                                                              c0.bn.running_var] if c0.with_norm else [])
        pk, vc = layers[0]._packed_fused()

        def build():
            # (the BatchNorm fold lives inside the miss branch: ahead of the key check it was six tiny launches per module and
            # step -- ~0.1 ms of the Voxel-RCNN step for values that only change with the parameters)
            w0, b0 = c0.conv.weight[:, :, 0, 0], c0.conv.bias
            if c0.with_norm:
                inv = torch.rsqrt(c0.bn.running_var + c0.bn.eps) * c0.bn.weight
                w0 = w0 * inv[:, None]
                b0 = c0.bn.bias - c0.bn.running_mean * inv + (b0 * inv if b0 is not None else 0)
            elif b0 is None:
                b0 = w0.new_zeros(w0.shape[0])
            return tuple(_ops.lt_layer_pack_pe(pk, vc, w0, b0, c1.conv.weight[:, :, 0, 0], c1.conv.bias))
        return (layers,) + _ops.derived(self.__dict__, "_pe_packed", [pk, vc] + ts, build)

    def _forward_rows(self, xyz, rows):
        """Inference path without a single transpose: `rows` [B,N,C] is the caller's query tensor (updated in place,
        'replace' semantics); grouped features are row gathers, the positional MLP runs on coordinate rows, the
        encoder sees [ns, B*np, C] directly and the winners are gathered back by row."""
        B, N, C = rows.shape
        group_idx, group_xyz = self._geometry(xyz)
        sel, gx, src, has, dst = self._row_plan(xyz, group_idx, group_xyz)
        ns, np_ = group_idx.shape[2], group_idx.shape[1]
        flat = rows.reshape(B * N, C)
        fused = self._fused_chunk(flat, ns, B * np_)
        if fused is not None:
            # the whole module as len(layers) launches: gather + positional MLP in the first layer's load, the 'unique' /
            # 'replace' write-back in the last layer's store (in place: the first launch has read `flat` before the last writes)
            layers, packed_pe, vec_pe = fused
            y = _ops.lt_layer_gather(flat, sel, gx, B * np_, packed_pe, vec_pe, layers[0].norm1.eps, layers[0].norm2.eps)
            for l in layers[1:-1]:
                y = l._forward_fused(y)
            pk, vc = layers[-1]._packed_fused()
            _ops.lt_layer_scatter(y, pk, vc, layers[-1].norm1.eps, layers[-1].norm2.eps, dst, flat)
            return rows
        x = self._pe_gather(flat, sel, gx)
        y = self.chunk(x.view(ns, B * np_, C)).reshape(ns * B * np_, C)
        flat.copy_(torch.where(has, y.index_select(0, src), flat))
        return rows

    def _pe_rows_train(self, gx):
        """self.pe on coordinate rows [R, 3] -> [R, C] under grad: the two 1x1 convolutions as row linears with the chunked
        weight gradient, BatchNorm2d over the rows (its statistics over [B, ., np, ns] are the statistics over the R rows) on
        batch statistics in train() mode (`ops.batch_norm_rows`: running statistics move as nn.BatchNorm2d moves them)."""
        c0, c1 = self.pe[0], self.pe[1]
        h = _ops.linear_rows_autograd(gx, c0.conv.weight[:, :, 0, 0], c0.conv.bias)
        if c0.with_norm:
            h = _ops.batch_norm_rows(c0.bn, h, relu=c0.with_activation)
        elif c0.with_activation:
            h = torch.relu(h)
        return _ops.linear_rows_autograd(h, c1.conv.weight[:, :, 0, 0], c1.conv.bias)

    def _forward_train_rows(self, xyz, features):
        """The row layout of `_forward_rows` from differentiable pieces: the gradient reaches `features` through the grouped
        rows (index_select by `sel`: every group a point is in) as well as through the kept rows of the points in no group
        (the `where`).  Geometry and row plan carry no gradient and are shared between the layers as at inference."""
        B, C, N = features.shape
        with torch.no_grad():
            group_idx, group_xyz = self._geometry(xyz)
            sel, gx, src, has, _ = self._row_plan(xyz, group_idx, group_xyz)
        ns, np_ = group_idx.shape[2], group_idx.shape[1]
        flat = features.permute(0, 2, 1).reshape(B * N, C)         # (a view when the caller holds [B,N,C] rows)
        x = flat.index_select(0, sel) + self._pe_rows_train(gx)
        y = self.chunk(x.view(ns, B * np_, C)).reshape(ns * B * np_, C)
        out = torch.where(has, y.index_select(0, src), flat).view(B, N, C)
        features.copy_(out.permute(0, 2, 1))             # the reference mutates its input in place (:371-372)
        return out

    def forward(self, xyz, features):
        """xyz [B,N,3], features [B,C,N] (may be a permuted view: 'replace' writes through it, as the
        reference does) -> [B,N,C].

        Under grad the result is differentiable in `features` and in every parameter, through the grouped rows and through
        the kept rows.  With feat_agg_method 'replace' the result is ALSO written into the caller's `features` in place, under
        grad as without: autograd refuses that write for a view of a leaf that requires grad and -- at backward -- for a
        tensor an earlier node saved, so a training caller hands in a non-leaf nobody saved (the ACTRv2 encoder's query
        tensor is one)."""
        if (features.is_cuda and not torch.is_grad_enabled() and not self.training and features.dtype == torch.float32
                and self.attn_feat_agg_method == "unique" and self.feat_agg_method == "replace"
                and features.permute(0, 2, 1).is_contiguous() and not (self.pe[0].with_norm and self.pe[0].bn.training)
                and self.pe[1].with_norm is False and self.pe[1].with_activation is False):
            return self._forward_rows(xyz, features.permute(0, 2, 1))
        if (features.is_cuda and torch.is_grad_enabled() and features.dtype == torch.float32
                and not torch.is_autocast_enabled() and self.attn_feat_agg_method == "unique"
                and self.feat_agg_method == "replace" and self.pe[1].with_norm is False
                and self.pe[1].with_activation is False):
            return self._forward_train_rows(xyz, features)
        feats_c = features.contiguous()
        group_idx, group_xyz = self._geometry(xyz)
        group_features = _ops.group_points(feats_c, group_idx)                          # [B,C,np,ns]
        x = group_features + self.pe(group_xyz)
        B, D, np_, ns = x.shape
        x = x.permute(0, 2, 1, 3).reshape(-1, D, ns).permute(2, 0, 1)                   # [ns, B*np, D]
        y = self.chunk(x).permute(1, 2, 0).reshape(B, np_, D, ns).transpose(1, 2)       # [B,D,np,ns]
        if self.feat_agg_method == "replace":
            out = feats_c
            self.scatter(out, y, group_idx)
            if out.data_ptr() != features.data_ptr():
                features.copy_(out)          # the reference mutates its input in place (:371-372)
            features = out
        elif self.feat_agg_method == "sum":
            attn = torch.zeros_like(feats_c)
            self.scatter(attn, y, group_idx)
            features = feats_c + attn
        else:
            raise NotImplementedError(self.feat_agg_method)
        return features.permute(0, 2, 1)
