"""Detection head of the CenterPoint tree: `CenterHead` / `SepHead` with the reference's
constructor arguments and parameter names (CP/det3d/models/bbox_heads/center_head.py:66-110,165-243), and
`predict` = the reference's decode + per-sample post-processing (center_head.py:302-501) as ONE device call
(`df3d_centerhead_predict`: keys -> radix sort -> gather -> NMS bit matrix -> on-device greedy reduction -> select)
instead of ~30 launches and three host round trips per (task, sample).  `loss` (center_head.py:250-298) is the
reference's torch composition (training row)."""
import copy
import os

import torch
from torch import nn

from . import ops as _ops
from .registry import HEADS


def _clamped_sigmoid(x):
    """center_head.py:246-248."""
    return torch.clamp(x.sigmoid_(), min=1e-4, max=1 - 1e-4)


def _transpose_and_gather_feat(feat, ind):
    """CP/det3d/core/utils/center_utils.py: [B, C, H, W] -> rows at the flat pixel indices ind [B, M] -> [B, M, C]."""
    feat = feat.permute(0, 2, 3, 1).contiguous()
    feat = feat.view(feat.size(0), -1, feat.size(3))
    return feat.gather(1, ind.unsqueeze(2).expand(ind.size(0), ind.size(1), feat.size(2)))


def reg_loss(output, mask, ind, target):
    """RegLoss (CP/det3d/models/losses/centernet_loss.py:6-27) -> one value per box code."""
    pred = _transpose_and_gather_feat(output, ind)
    mask = mask.float().unsqueeze(2)
    loss = torch.nn.functional.l1_loss(pred * mask, target * mask, reduction='none')
    loss = loss / (mask.sum() + 1e-4)
    return loss.transpose(2, 0).sum(dim=2).sum(dim=1)


def fast_focal_loss(out, target, ind, mask, cat):
    """FastFocalLoss (centernet_loss.py:29-58)."""
    mask = mask.float()
    gt = torch.pow(1 - target, 4)
    neg_loss = (torch.log(1 - out) * torch.pow(out, 2) * gt).sum()
    pos_pred_pix = _transpose_and_gather_feat(out, ind)
    pos_pred = pos_pred_pix.gather(2, cat.unsqueeze(2))
    num_pos = mask.sum()
    pos_loss = (torch.log(pos_pred) * torch.pow(1 - pos_pred, 2) * mask.unsqueeze(2)).sum()
    # the reference branches on num_pos == 0 (-> -neg_loss); pos_loss is exactly 0 then, so dividing by max(num_pos, 1)
    # is the same value without reading num_pos back to the host in the middle of the step
    return -(pos_loss + neg_loss) / num_pos.clamp(min=1.0)


class _BranchConvFunction(torch.autograd.Function):
    """First convolutions of all G head branches (3x3, 64 -> 64 each, every branch reads the same shared rows) with
    autograd, on the kernels the inference path uses: forward = ONE grouped launch (two branches per 128-column
    block); input gradient = one grouped launch over the G gradient slices with the transposed filters and the
    mirrored table, then the sum over branches; filter gradient = df3d_sparse_conv_grad_filters with G * 64 output
    columns.  rows [P, 64], w [G, 9, 64, 64] (tap, cin, cout), bias [G * 64] -> [P, G * 64]."""

    @staticmethod
    def forward(ctx, rows, w, bias, nbr, nbr_mirror):
        G, K, cin, cout = w.shape
        P = rows.shape[0]
        pair = 2 if G % 2 == 0 else 1
        wd = w.detach().float()
        wp = wd.view(G // pair, pair, K, cin, cout).permute(0, 2, 3, 1, 4).reshape(G // pair, K, cin, cout * pair)
        packed = _ops.conv_pack_weights_groups(wp.contiguous())
        out, _ = _ops.conv_rows_split(_ops.split_rows(rows.contiguous()), cin, 0, packed, cout * pair, G // pair, nbr, P,
                                      bias.detach().float().contiguous() if bias is not None else None, None, None,
                                      relu=False)
        ctx.save_for_backward(rows, w, nbr, nbr_mirror)
        ctx.has_bias = bias is not None
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        rows, w, nbr, nbr_mirror = ctx.saved_tensors
        G, K, cin, cout = w.shape
        P = rows.shape[0]
        go = grad_out.contiguous().float()
        plan = _ops.conv_grad_plan(K, cin, cout, False, grouped=True)
        with _ops.precision(plan.mode):
            packed_t = _ops.conv_pack_weights_groups(w.detach().float().transpose(2, 3).contiguous())
            if plan.scaled:   # the gradient rows as fp16 pairs under their own power-of-two scale; the epilogue multiplies by 1 / s
                gs, inv_s, g_sc = _ops.split_rows_scaled(go, G * cin)
            else:             # three bf16 parts -- or, `plan.fixed_scale`, fp16 pairs at the activation scale
                gs, inv_s, g_sc = _ops.split_rows(go), None, None
            part, _ = _ops.conv_rows_split(gs, cout, cout, packed_t, cin, G, nbr_mirror, P, None, inv_s, None, relu=False)
        g_rows = part.view(P, G, cin).sum(1)
        g_w = _ops.sparse_conv_grad_filters(rows.contiguous(), go, nbr, grad_scale=g_sc)            # [K, cin, G * cout]
        g_w = g_w.view(K, cin, G, cout).permute(2, 0, 1, 3)
        g_b = go.sum(0) if ctx.has_bias else None
        return g_rows, g_w, g_b, None, None


class _HeadFinalFunction(torch.autograd.Function):
    """Final convolutions of all head branches (3x3, 64 -> 1..3 maps each) with autograd on the vector-ALU kernels of
    csrc/headconv.hip: acts [P, G * 64] fp32 rows, w4 [G, 9, 64, 4], b4 [G, 4] -> packed maps [P, width]."""

    @staticmethod
    def forward(ctx, acts, w4, b4, cols, width, B, H, W):
        acts = acts.contiguous()
        w4d, b4d = w4.detach().float().contiguous(), b4.detach().float().contiguous()
        out = _ops.head_final_conv(_ops.split_rows(acts), B, H, W, w4d, b4d, cols, width)
        ctx.save_for_backward(acts, w4d, cols)
        ctx.geom = (B, H, W)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        acts, w4d, cols = ctx.saved_tensors
        B, H, W = ctx.geom
        go = grad_out.contiguous().float()
        g_a, g_w = _ops.head_final_conv_backward(acts, go, B, H, W, w4d.shape[0], w4d, cols)
        # bias gradient: column sums of the packed maps, gathered into the [G, 4] layout (padding maps: 0)
        sums = torch.cat([go.sum(0), go.new_zeros(1)])
        c = cols.long()
        j = torch.arange(4, device=go.device)
        idx = torch.where(j[None, :] < c[:, 1:2], c[:, 0:1] + j[None, :], torch.full_like(c[:, 0:1], go.shape[1]))
        return g_a, g_w, sums[idx], None, None, None, None, None


class _PermuteGather(torch.autograd.Function):
    """out = src[idx] where every element of `src` but the last (a zero used for padding slots) appears exactly once in
    `idx`: the backward is the gather through the inverse index (`inv[i]` = position of src[i] in out), not an index_add."""

    @staticmethod
    def forward(ctx, src, idx, inv):
        ctx.save_for_backward(inv)
        return src.index_select(0, idx)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        inv, = ctx.saved_tensors
        g = grad.contiguous().index_select(0, inv)
        g[-1] = 0                                   # the padding zero is not a parameter
        return g, None, None


class SepHead(nn.Module):
    def __init__(self, in_channels, heads, head_conv=64, final_kernel=1, bn=False, init_bias=-2.19, **kwargs):
        super(SepHead, self).__init__(**kwargs)
        self.heads = heads
        for head in self.heads:
            classes, num_conv = self.heads[head]
            mods = []
            for _ in range(num_conv - 1):
                mods.append(nn.Conv2d(in_channels, head_conv, kernel_size=final_kernel, stride=1,
                                      padding=final_kernel // 2, bias=True))
                if bn:
                    mods.append(nn.BatchNorm2d(head_conv))
                mods.append(nn.ReLU())
            mods.append(nn.Conv2d(head_conv, classes, kernel_size=final_kernel, stride=1, padding=final_kernel // 2,
                                  bias=True))
            fc = nn.Sequential(*mods)
            if 'hm' in head:
                fc[-1].bias.data.fill_(init_bias)
            else:
                for m in fc.modules():
                    if isinstance(m, nn.Conv2d):
                        nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
                        if m.bias is not None:
                            nn.init.constant_(m.bias, 0)
            self.__setattr__(head, fc)

    def forward(self, x):
        return {head: self.__getattr__(head)(x) for head in self.heads}


@HEADS.register_module
class CenterHead(nn.Module):
    def __init__(self, in_channels=[128, ], tasks=[], dataset='nuscenes', weight=0.25, code_weights=[],
                 common_heads=dict(), logger=None, init_bias=-2.19, share_conv_channel=64, num_hm_conv=2,
                 dcn_head=False):
        super(CenterHead, self).__init__()
        if dcn_head:
            raise NotImplementedError("dcn_head=True (deformable-conv head) is not part of the 3D-Dual-Fusion configs")
        num_classes = [len(t["class_names"]) for t in tasks]
        self.class_names = [t["class_names"] for t in tasks]
        self.code_weights = code_weights
        self.weight = weight
        self.dataset = dataset
        self.in_channels = in_channels
        self.num_classes = num_classes
        self.box_n_dim = 9 if 'vel' in common_heads else 7
        self.use_direction_classifier = False
        self.shared_conv = nn.Sequential(nn.Conv2d(in_channels, share_conv_channel, kernel_size=3, padding=1, bias=True),
                                         nn.BatchNorm2d(share_conv_channel), nn.ReLU(inplace=True))
        self.tasks = nn.ModuleList()
        for num_cls in num_classes:
            heads = copy.deepcopy(common_heads)
            heads.update(dict(hm=(num_cls, num_hm_conv)))
            self.tasks.append(SepHead(share_conv_channel, heads, bn=True, init_bias=init_bias, final_kernel=3))

    def forward_reference(self, x):
        x = self.shared_conv(x)
        return [task(x) for task in self.tasks]

    def forward(self, x, *kwargs):
        self.__dict__.pop("_packed_train", None)          # a previous step's packed maps (and their graph) are not kept
        if ((self.training or torch.is_grad_enabled()) and x.is_cuda and x.dtype == torch.float32
                and _ops.CONV_PRECISION in ("split", "bf16") and self._row_kernels_fit(x) and self._train_rows_fit()):
            return self.forward_rows_train(x)
        if (self.training or torch.is_grad_enabled() or not x.is_cuda or x.dtype != torch.float32
                or not self._row_kernels_fit(x)):
            return self.forward_reference(x)
        if _ops.CONV_PRECISION == "fp32":
            return self.forward_rows_fp32(x)
        # the head's own convolutions stay split precision (fp32-grade) in the bf16 mode of the backbone / neck
        return self.forward_rows(x)

    # ------------------------------------------------------------------ the three conv depths as three launches
    def train(self, mode=True):
        for k in ("_row_plan", "_row_fit", "_plan_tensors"):
            self.__dict__.pop(k, None)
        return super(CenterHead, self).train(mode)

    def _state_tensors(self):
        """Every parameter and buffer of the head.  Their (dict, name) slots are collected ONCE (the module tree walk of
        `parameters()` cost ~1 ms of host time per step) and read per call: a list of the tensors themselves would go on
        watching the old buffer objects after `.double().float()` replaced them.  `train()` drops the slots."""
        slots = self.__dict__.get("_plan_tensors")
        if slots is None:
            slots = self.__dict__["_plan_tensors"] = _ops.state_slots(self)
        return _ops.slot_tensors(slots)

    def _row_kernels_fit(self, x):
        hit = self.__dict__.get("_row_fit")
        if hit is None:
            hit = self.__dict__["_row_fit"] = self._row_kernels_fit_uncached()
        return hit

    def _row_kernels_fit_uncached(self):
        sc = self.shared_conv[0]
        ok = sc.in_channels == 512 and sc.out_channels == 64 and sc.kernel_size == (3, 3)
        for task in self.tasks:
            for head in task.heads:
                fc = getattr(task, head)
                ok = ok and len(fc) == 4 and isinstance(fc[1], nn.BatchNorm2d) and fc[0].kernel_size == (3, 3) \
                    and fc[0].out_channels == 64 and fc[3].out_channels <= 32
        return ok

    def _train_rows_fit(self):
        """What `forward_rows_train` assumes on top of `_row_kernels_fit`: final convs of <= 4 maps (HF_KMAX of
        headconv.hip) with a bias, biased first convs, and ONE set of BatchNorm hyper-parameters over all branches (their 36
        BatchNorms run as one).  Anything else (e.g. a single 10-class task) trains through `forward_reference`."""
        bns = [getattr(task, head)[1] for task in self.tasks for head in task.heads]
        fcs = [getattr(task, head) for task in self.tasks for head in task.heads]
        return (all(fc[3].out_channels <= 4 and fc[3].bias is not None and fc[0].bias is not None for fc in fcs)
                and all((b.momentum, b.eps, b.training, b.affine, b.track_running_stats) ==
                        (bns[0].momentum, bns[0].eps, bns[0].training, bns[0].affine, bns[0].track_running_stats) for b in bns))

    @staticmethod
    def _filters(conv, pad_to=None):
        w = conv.weight.detach().float().permute(2, 3, 1, 0).reshape(9, conv.in_channels, conv.out_channels)
        if pad_to is not None and pad_to > conv.out_channels:
            w = torch.cat([w, w.new_zeros(9, conv.in_channels, pad_to - conv.out_channels)], 2)
        return w.contiguous()

    @staticmethod
    def _fold(bn):
        scale = bn.weight.float() * torch.rsqrt(bn.running_var.float() + bn.eps)
        return scale, bn.bias.float() - bn.running_mean.float() * scale

    def _plan(self):
        key = _ops.tensors_key(self._state_tensors()) + (_ops.split_parts(),)
        plan = self.__dict__.get("_row_plan")
        if plan is not None and plan["key"] == key:
            return plan
        sc, sbn = self.shared_conv[0], self.shared_conv[1]
        s_scale, s_shift = self._fold(sbn)
        dev = sc.weight.device
        mid_filters, mid_bias, mid_scale, mid_shift, fin_packed, fin_bias, cols, layout = [], [], [], [], [], [], [], []
        fin_w4, fin_b4 = [], []
        c0 = 0
        for t, task in enumerate(self.tasks):
            for head in task.heads:
                fc = getattr(task, head)
                mid_filters.append(self._filters(fc[0]))
                mid_bias.append(fc[0].bias.detach().float())
                a, b = self._fold(fc[1])
                mid_scale.append(a)
                mid_shift.append(b)
                k = fc[3].out_channels
                fin_packed.append(_ops.conv_pack_weights(self._filters(fc[3], 32)))
                fin_bias.append(torch.cat([fc[3].bias.detach().float(), torch.zeros(32 - k, device=dev)]))
                if k <= 4:           # [9, 64, 4] tap-major filters for the vector-ALU kernel (csrc/headconv.hip)
                    fin_w4.append(self._filters(fc[3], 4))
                    fin_b4.append(torch.cat([fc[3].bias.detach().float(), torch.zeros(4 - k, device=dev)]))
                cols.append((c0, k))
                layout.append((t, head, c0, k))
                c0 += k
        # All branches read the same 64 shared channels, so two neighbouring 64-column branches form one 128-column block
        # of one convolution 64 -> 64 * branches: half the gathers of the input rows, and the 128-column kernel
        mid_pair = 2 if len(mid_filters) % 2 == 0 else 1
        mid_packed = [_ops.conv_pack_weights(torch.cat(mid_filters[i:i + mid_pair], dim=2).contiguous())
                      for i in range(0, len(mid_filters), mid_pair)]
        plan = dict(key=key, shared=_ops.conv_pack_weights(self._filters(sc)), s_bias=sc.bias.detach().float().contiguous(),
                    s_scale=s_scale.contiguous(), s_shift=s_shift.contiguous(),
                    mid=torch.cat(mid_packed), mid_pair=mid_pair, mid_bias=torch.cat(mid_bias).contiguous(),
                    mid_scale=torch.cat(mid_scale).contiguous(), mid_shift=torch.cat(mid_shift).contiguous(),
                    fin=torch.cat(fin_packed), fin_bias=torch.cat(fin_bias).contiguous(),
                    cols=torch.tensor(cols, dtype=torch.int32, device=dev).contiguous(), layout=layout,
                    groups=len(cols), width=(c0 + 7) // 8 * 8, nbr={},
                    fin_w4=torch.stack(fin_w4).contiguous() if len(fin_w4) == len(cols) else None,
                    fin_b4=torch.stack(fin_b4).contiguous() if len(fin_b4) == len(cols) else None)
        self.__dict__["_row_plan"] = plan
        return plan

    @torch.no_grad()
    def forward_rows_fp32(self, x):
        """The exact-fp32 mode (DF3D_CONV_PRECISION=fp32) on the native kernels: the three conv depths of the head as three
        launches of the fp32 MFMA kernel (`v_mfma_f32_16x16x4_f32`, csrc/spconv.hip) over the dense 3 x 3 neighbour table:
        shared conv 512 -> 64; the first convs of all branches as ONE grouped launch (every group reads the same 64 shared
        channels; 64 -> 128 per group = two branches) into a [pixels, 64 * branches] buffer; the final convs as ONE grouped
        launch, each group reading its branch's 64 columns of that buffer in place (64 -> classes padded to 16)."""
        from .necks import _rows_of
        key = _ops.tensors_key(self._state_tensors())
        plan = self.__dict__.get("_row_plan_fp32")
        if plan is None or plan["key"] != key:
            sc, sbn = self.shared_conv[0], self.shared_conv[1]
            dev = sc.weight.device
            s_scale, s_shift = self._fold(sbn)
            branches = [(t, head, getattr(task, head)) for t, task in enumerate(self.tasks) for head in task.heads]
            nb = len(branches)
            per = int(os.environ.get("DF3D_HEAD_FP32_PAIR", "2"))          # branches per group of the first convs
            if nb % per:
                per = 1
            folds = [self._fold(fc[1]) for _, _, fc in branches]
            mid_w = torch.stack([torch.cat([self._filters(fc[0]) for _, _, fc in branches[i:i + per]], 2)
                                 for i in range(0, nb, per)]).contiguous()                     # [nb / per, 9, 64, 64 * per]
            mid_bias = torch.cat([fc[0].bias.detach().float() if fc[0].bias is not None else torch.zeros(64, device=dev)
                                  for _, _, fc in branches]).contiguous()
            kp = 16 if max(fc[3].out_channels for _, _, fc in branches) <= 16 else 32
            fin_w = torch.stack([self._filters(fc[3], kp) for _, _, fc in branches]).contiguous()  # [nb, 9, 64, kp]
            fin_b = torch.cat([torch.cat([fc[3].bias.detach().float() if fc[3].bias is not None
                                          else torch.zeros(fc[3].out_channels, device=dev),
                                          torch.zeros(kp - fc[3].out_channels, device=dev)]) for _, _, fc in branches]).contiguous()
            plan = dict(key=key, shared=self._filters(sc), s_bias=sc.bias.detach().float().contiguous() if sc.bias is not None else None,
                        s_scale=s_scale.contiguous(), s_shift=s_shift.contiguous(), branches=branches, kp=kp,
                        mid_w=mid_w, mid_bias=mid_bias, mid_scale=torch.cat([f[0] for f in folds]).contiguous(),
                        mid_shift=torch.cat([f[1] for f in folds]).contiguous(), fin_w=fin_w, fin_b=fin_b, nbr={})
            self.__dict__["_row_plan_fp32"] = plan
        B, _, H, W = x.shape
        rows, _ = _rows_of(x)
        if (B, H, W) not in plan["nbr"]:
            plan["nbr"][(B, H, W)] = _ops.conv2d_neighbors(B, H, W, 3, 3, 1, 1, False, x.device)[0]
        nbr = plan["nbr"][(B, H, W)]
        n = B * H * W
        s1 = _ops.sparse_conv_fused(rows.contiguous(), plan["shared"], nbr, n, bias=plan["s_bias"], scale=plan["s_scale"],
                                    shift=plan["s_shift"], relu=True)
        mid = _ops.sparse_conv_grouped(s1, plan["mid_w"], nbr, n, bias=plan["mid_bias"], scale=plan["mid_scale"],
                                       shift=plan["mid_shift"], relu=True, group_in=0)
        out = _ops.sparse_conv_grouped(mid, plan["fin_w"], nbr, n, bias=plan["fin_b"], group_in=64)
        rets = [dict() for _ in self.tasks]
        kp = plan["kp"]
        for i, (t, head, fc) in enumerate(plan["branches"]):
            k = fc[3].out_channels
            r = out[:, i * kp:i * kp + k]
            v = r.view(B, H, W, k).permute(0, 3, 1, 2)
            v._df3d_rows = (r, None, v._version)
            rets[t][head] = v
        return rets

    @torch.no_grad()
    def forward_rows(self, x):
        """shared 3x3 conv (512 -> 64), the 36 first convs of all heads (64 -> 36 x 64) and their 36 final convs
        (block-diagonal 64 -> classes) as three launches of the split-precision conv kernel over pixel rows; every
        head map is a column slice of one [B*H*W, 72] buffer, which `predict` reads in place."""
        from .necks import _rows_of
        plan = self._plan()
        B, _, H, W = x.shape
        rows, split = _rows_of(x)
        if (split is None or split.dtype != torch.uint8     # no hi/lo rows cached (bf16 mode of the neck caches bf16 rows)
                or split.shape[1] != _ops.split_width(rows.shape[1])):
            split = _ops.split_rows(rows.contiguous())
        if (B, H, W) not in plan["nbr"]:
            plan["nbr"][(B, H, W)] = _ops.conv2d_neighbors(B, H, W, 3, 3, 1, 1, False, x.device)[0]
        nbr = plan["nbr"][(B, H, W)]
        n = B * H * W
        G = plan["groups"]
        _, s1 = _ops.conv_rows_split(split, 512, 0, plan["shared"], 64, 1, nbr, n, plan["s_bias"], plan["s_scale"],
                                     plan["s_shift"], relu=True, want_out=False, want_split=True)
        _, s2 = _ops.conv_rows_split(s1, 64, 0, plan["mid"], 64 * plan["mid_pair"], G // plan["mid_pair"], nbr, n,
                                     plan["mid_bias"], plan["mid_scale"], plan["mid_shift"], relu=True, want_out=False,
                                     want_split=True)
        if (plan["fin_w4"] is not None and os.environ.get("DF3D_HEAD_FINAL", "valu") == "valu"
                and _ops.CONV_PRECISION != "split3"):       # (csrc/headconv.hip reads two-part rows)
            # 72 output maps of 36 branches in one launch of csrc/headconv.hip (round 3: the taps are COLUMNS of a matrix-core
            # product over each halo pixel's 64 channels, the shifted sum runs through LDS; every activation read 1.3x)
            # instead of a block-diagonal matrix-core launch padded to 32 columns per branch
            if "fin_pk" not in plan:
                plan["fin_pk"] = (_ops.head_final_pack(plan["fin_w4"])
                                  if os.environ.get("DF3D_HEADFINAL", "mfma")[:1] != "v" else None)
            out = _ops.head_final_conv(s2, B, H, W, plan["fin_w4"], plan["fin_b4"], plan["cols"], plan["width"],
                                       packed=plan["fin_pk"])
        else:
            out, _ = _ops.conv_rows_split(s2, 64, 64, plan["fin"], 32, G, nbr, n, plan["fin_bias"], None, None, relu=False,
                                          out_channels=plan["width"], out_cols=plan["cols"])
        rets = [dict() for _ in self.tasks]
        for t, head, c0, k in plan["layout"]:
            r = out[:, c0:c0 + k]
            v = r.view(B, H, W, k).permute(0, 3, 1, 2)
            v._df3d_rows = (r, None, v._version)
            rets[t][head] = v
        return rets

    # ------------------------------------------------------------------ loss-only path: heat maps densely, box codes at the object centres
    _SITE_CODES = (("reg", 2), ("height", 1), ("dim", 3), ("vel", 2), ("rot", 2))      # the loss kernel's code order

    def _sites_plan(self, plan):
        """Operands of the loss-only path, kept in (and dropped with) the row plan: the heat-map branches as a dense subset
        (first convs 64 -> 64 per task as 128-column blocks, final convs into a packed [n, width] buffer) and the regression
        branches as banks of `ops.head_regress_at`.  None when the head is not reg / height / dim / rot (/ vel) + hm."""
        if "sites" in plan:
            return plan["sites"]
        plan["sites"] = None
        names = [n for n, _ in self._SITE_CODES]
        vel = all("vel" in task.heads for task in self.tasks)
        want = {n: k for n, k in self._SITE_CODES if vel or n != "vel"}
        for task in self.tasks:
            if set(task.heads) != set(want) | {"hm"} or any(getattr(task, n)[3].out_channels != k for n, k in want.items()) \
                    or any(getattr(task, n)[0].bias is None or getattr(task, n)[3].bias is None for n in task.heads):
                return None
        dev = self.shared_conv[0].weight.device
        pad4 = lambda fc: torch.cat([fc[3].bias.detach().float(), torch.zeros(4 - fc[3].out_channels, device=dev)])
        # heat maps: the dense subset
        hms = [task.hm for task in self.tasks]
        pair = 2 if len(hms) % 2 == 0 else 1
        f1 = [self._filters(fc[0]) for fc in hms]
        folds = [self._fold(fc[1]) for fc in hms]
        cols, c0 = [], 0
        for fc in hms:
            cols.append((c0, fc[3].out_channels))
            c0 += fc[3].out_channels
        w4 = torch.stack([self._filters(fc[3], 4) for fc in hms]).contiguous()
        sites = dict(hm_mid=torch.cat([_ops.conv_pack_weights(torch.cat(f1[i:i + pair], dim=2).contiguous())
                                       for i in range(0, len(f1), pair)]), hm_pair=pair,
                     hm_bias=torch.cat([fc[0].bias.detach().float() for fc in hms]).contiguous(),
                     hm_scale=torch.cat([a for a, _ in folds]).contiguous(), hm_shift=torch.cat([b for _, b in folds]).contiguous(),
                     hm_w4=w4, hm_b4=torch.stack([pad4(fc) for fc in hms]).contiguous(),
                     hm_pk=_ops.head_final_pack(w4) if os.environ.get("DF3D_HEADFINAL", "mfma")[:1] != "v" else None,
                     hm_cols=cols, hm_cols_dev=torch.tensor(cols, dtype=torch.int32, device=dev).contiguous(),
                     hm_width=(c0 + 7) // 8 * 8, vel=vel, ncodes=10 if vel else 8)
        # regression branches: banks (task, branch) in the loss kernel's code order
        banks, rcols = [], []
        for task in self.tasks:
            c = 0
            for n in names:
                if n in want:
                    banks.append(getattr(task, n))
                    rcols.append((c, want[n]))
                    c += want[n]
        rfolds = [self._fold(fc[1]) for fc in banks]
        sites.update(w1=_ops.head_regress_pack(torch.stack([self._filters(fc[0]) for fc in banks]).contiguous()),
                     bias1=torch.stack([fc[0].bias.detach().float() for fc in banks]).contiguous(),
                     scale1=torch.stack([a for a, _ in rfolds]).contiguous(), shift1=torch.stack([b for _, b in rfolds]).contiguous(),
                     w2=torch.stack([self._filters(fc[3], 4) for fc in banks]).contiguous(),
                     b2=torch.stack([pad4(fc) for fc in banks]).contiguous(),
                     cols=torch.tensor(rcols, dtype=torch.int32, device=dev).contiguous())
        plan["sites"] = sites
        return sites

    def loss_sites_wanted(self, example):
        """The switch of the loss-only path (DF3D_HEAD_LOSS_SITES, default on; read per call) and what it needs of `example`:
        device tensors hm / ind / mask / cat / anno_box for every task."""
        if os.environ.get("DF3D_HEAD_LOSS_SITES", "1") == "0" or self.dataset not in ('waymo', 'nuscenes'):
            return False
        if not isinstance(example, dict):
            return False
        T = len(self.tasks)
        for k in ("hm", "ind", "mask", "cat", "anno_box"):
            v = example.get(k)
            if not isinstance(v, (list, tuple)) or len(v) < T or not all(torch.is_tensor(a) and a.is_cuda for a in v[:T]):
                return False
        return True

    def loss_sites_fit(self, x):
        """True in the state in which `forward(x)` would run `forward_rows` with its `head_final_conv` branch (eval, no grad,
        CUDA fp32 input, row kernels, two-part split rows) for a head whose branches the loss-only operands describe."""
        if (self.training or torch.is_grad_enabled() or not x.is_cuda or x.dtype != torch.float32 or not self._row_kernels_fit(x)
                or _ops.CONV_PRECISION in ("fp32", "split3") or os.environ.get("DF3D_HEAD_FINAL", "valu") != "valu"):
            return False
        plan = self._plan()
        if plan["fin_w4"] is None:
            return False
        sites = self._sites_plan(plan)
        return sites is not None and len(self.code_weights) == sites["ncodes"]

    @torch.no_grad()
    def forward_loss_dense(self, x):
        """Dense part of the loss-only path (fixed shapes: library launches, allocations and views only): the shared conv as
        in `forward_rows`, then ONLY the heat-map branches -- their first convs as one grouped launch, their final convs
        through `head_final_conv`.  -> (heat maps [B*H*W, width] fp32 packed, split rows of the shared conv, (B, H, W))."""
        from .necks import _rows_of
        self.__dict__.pop("_packed_train", None)
        plan = self._plan()
        sites = self._sites_plan(plan)
        B, _, H, W = x.shape
        rows, split = _rows_of(x)
        if (split is None or split.dtype != torch.uint8 or split.shape[1] != _ops.split_width(rows.shape[1])):
            split = _ops.split_rows(rows.contiguous())
        if (B, H, W) not in plan["nbr"]:
            plan["nbr"][(B, H, W)] = _ops.conv2d_neighbors(B, H, W, 3, 3, 1, 1, False, x.device)[0]
        nbr = plan["nbr"][(B, H, W)]
        n = B * H * W
        T = len(self.tasks)
        _, s1 = _ops.conv_rows_split(split, 512, 0, plan["shared"], 64, 1, nbr, n, plan["s_bias"], plan["s_scale"],
                                     plan["s_shift"], relu=True, want_out=False, want_split=True)
        _, s2 = _ops.conv_rows_split(s1, 64, 0, sites["hm_mid"], 64 * sites["hm_pair"], T // sites["hm_pair"], nbr, n,
                                     sites["hm_bias"], sites["hm_scale"], sites["hm_shift"], relu=True, want_out=False,
                                     want_split=True)
        out = _ops.head_final_conv(s2, B, H, W, sites["hm_w4"], sites["hm_b4"], sites["hm_cols_dev"], sites["hm_width"],
                                   packed=sites["hm_pk"])
        return out, s1, (B, H, W)

    @torch.no_grad()
    def loss_sites(self, example, dense):
        """Sparse part of the loss-only path: the regression branches at the object centres (ONE launch, csrc/headloss.hip)
        and the loss over the dense heat maps and those slot rows.  Same dict as `loss_device`."""
        out_hm, s1, (B, H, W) = dense
        sites = self._sites_plan(self._plan())
        T = len(self.tasks)
        pred = _ops.head_regress_at(s1, B, H, W, [example['ind'][t] for t in range(T)], [example['mask'][t] for t in range(T)],
                                    sites["w1"], sites["bias1"], sites["scale1"], sites["shift1"], sites["w2"], sites["b2"],
                                    sites["cols"])
        ncodes = sites["ncodes"]
        tasks = []
        for t, (c0, k) in enumerate(sites["hm_cols"]):
            p = pred[t]
            d = dict(hm=out_hm[:, c0:c0 + k], reg=p[:, 0:2], height=p[:, 2:3], dim=p[:, 3:6], rot=p[:, ncodes - 2:ncodes])
            if sites["vel"]:
                d['vel'] = p[:, 6:8]
            tasks.append(d)
        targets = [dict(hm=example['hm'][t], ind=example['ind'][t], mask=example['mask'][t], cat=example['cat'][t],
                        anno_box=example['anno_box'][t]) for t in range(T)]
        out = _ops.centerhead_loss(tasks, targets, B, H, W, self.code_weights, self.weight, reg_by_slot=True)
        return {'loss': out[:, 0], 'hm_loss': out[:, 1], 'loc_loss': out[:, 2], 'num_positive': out[:, 3],
                'loc_loss_elem': out[:, 4:4 + ncodes]}

    def _final_pack(self, branches, dev):
        """Index tensors that gather the [G, 9, 64, 4] / [G, 4] operands of the final-conv kernel out of the concatenated
        (flattened) conv weights / biases of the branches (last element of the concatenation = 0 for the padding maps)."""
        key = (tuple(fc[3].out_channels for _, _, fc in branches), str(dev))
        hit = self.__dict__.get("_final_pack_cache")
        if hit is not None and hit["key"] == key:
            return hit
        widx, bidx, cols, layout = [], [], [], []
        wbase = bbase = c0 = 0
        for _, _, fc in branches:
            k = fc[3].out_channels
            assert k <= 4 and fc[3].in_channels == 64 and fc[3].kernel_size == (3, 3)
            j, c, tap = torch.meshgrid(torch.arange(4), torch.arange(64), torch.arange(9), indexing="ij")
            idx = wbase + (j * 64 + c) * 9 + tap                         # weight [k, 64, 3, 3] flattened
            idx = torch.where(j < k, idx, torch.full_like(idx, -1))
            widx.append(idx.permute(2, 1, 0))                            # [tap, c, j]
            bidx.append(torch.tensor([bbase + jj if jj < k else -1 for jj in range(4)]))
            cols.append((c0, k))
            layout.append((c0, k))
            wbase += k * 64 * 9
            bbase += k
            c0 += k
        widx = torch.stack(widx)
        bidx = torch.stack(bidx)
        widx[widx < 0] = wbase                                           # the appended zero
        bidx[bidx < 0] = bbase
        def inverse(idx, n):                       # position of source element i in idx (the last source element: anywhere)
            inv = torch.zeros(n + 1, dtype=torch.long)
            flat = idx.reshape(-1)
            inv[flat] = torch.arange(flat.numel())
            return inv
        hit = dict(key=key, widx=widx.to(dev), bidx=bidx.to(dev), layout=layout, width=(c0 + 7) // 8 * 8,
                   winv=inverse(widx, wbase).to(dev), binv=inverse(bidx, bbase).to(dev),
                   cols=torch.tensor(cols, dtype=torch.int32, device=dev).contiguous())
        self.__dict__["_final_pack_cache"] = hit
        return hit

    def forward_rows_train(self, x):
        """`forward` with autograd (training rows) over channels-last pixel rows: the shared
        convolution and the first convolution of all branches run on the sparse-convolution kernels (forward, input
        gradient and filter gradient; `_BranchConvFunction` batches the 36 branches into single launches), their
        BatchNorms as ONE batch-statistics normalisation (+ ReLU) over the 36 x 64 columns (csrc/bnrows.hip); the final
        64 -> classes convolutions (1 - 3 maps each) on the vector-ALU kernels of csrc/headconv.hip (`_HeadFinalFunction`).
        Every head map is a column slice of one [B*H*W, 72] buffer."""
        from .necks import _bn_rows, _rows_of, _train_stack
        F = torch.nn.functional
        tables = self.__dict__.setdefault("_train_tables", {})
        B, _, H, W = x.shape
        rows, _ = _rows_of(x)
        sc, sbn = self.shared_conv[0], self.shared_conv[1]
        s, _, _ = _train_stack([(sc, sbn, True, 1)], rows, B, H, W, tables)
        nbr = tables[(B, H, W, 3, 3, 1, 1, False)][0]
        mkey = (B, H, W, "mirror")
        if mkey not in tables:
            tables[mkey] = nbr.flip(0).contiguous()
        branches = [(t, head, getattr(task, head)) for t, task in enumerate(self.tasks) for head in task.heads]
        G = len(branches)
        # [G, cout, cin, 3, 3] -> [G, tap, cin, cout] from ONE concatenation of the flattened filters
        w = torch.cat([fc[0].weight.reshape(-1) for _, _, fc in branches]).view(G, 64, 64, 3, 3)
        w = w.permute(0, 3, 4, 2, 1).reshape(G, 9, 64, 64)
        b = torch.cat([fc[0].bias for _, _, fc in branches])
        m = _BranchConvFunction.apply(s, w, b, nbr, tables[mkey])                       # [P, G * 64]
        # ONE batch-statistics BatchNorm + ReLU over the 36 x 64 columns (row kernels), the running statistics copied back
        bns = [fc[1] for _, _, fc in branches]
        mean = torch.cat([bn.running_mean for bn in bns])
        var = torch.cat([bn.running_var for bn in bns])
        if bns[0].training and _ops.bn_rows_supported(G * 64):
            m = _ops.BatchNormRowsFunction.apply(m, torch.cat([bn.weight for bn in bns]), torch.cat([bn.bias for bn in bns]),
                                                 mean, var, bns[0].momentum, bns[0].eps, True)
        else:
            m = torch.relu(F.batch_norm(m, mean, var, torch.cat([bn.weight for bn in bns]),
                                        torch.cat([bn.bias for bn in bns]), bns[0].training, bns[0].momentum, bns[0].eps))
        if bns[0].training:
            with torch.no_grad():
                torch._foreach_copy_([bn.running_mean for bn in bns], list(mean.split(64)))
                torch._foreach_copy_([bn.running_var for bn in bns], list(var.split(64)))
                torch._foreach_add_([bn.num_batches_tracked for bn in bns], 1)
        # final convolutions of all branches: one launch forward, two backward; the [G, 9, 64, 4] filter bank is gathered
        # from the flattened conv weights (one cat + one index: the gradient returns through the same two ops)
        pack = self._final_pack(branches, m.device)
        flat_w = torch.cat([fc[3].weight.reshape(-1) for _, _, fc in branches] + [m.new_zeros(1)])
        flat_b = torch.cat([fc[3].bias for _, _, fc in branches] + [m.new_zeros(1)])
        w4 = _PermuteGather.apply(flat_w, pack["widx"].reshape(-1), pack["winv"]).view(G, 9, 64, 4)
        b4 = _PermuteGather.apply(flat_b, pack["bidx"].reshape(-1), pack["binv"]).view(G, 4)
        out = _HeadFinalFunction.apply(m, w4, b4, pack["cols"], pack["width"], B, H, W)
        rets = [dict() for _ in self.tasks]
        maps = out.view(B, H, W, -1)
        # the packed buffer itself, for `loss_rows` (losses + their gradient in two launches)
        cols = [dict() for _ in self.tasks]
        for (t, head, fc), (c0, k) in zip(branches, pack["layout"]):
            cols[t][head] = (c0, k)
        self.__dict__["_packed_train"] = (out, cols, (B, H, W))
        for (t, head, fc), (c0, k) in zip(branches, pack["layout"]):
            v = maps[..., c0:c0 + k].permute(0, 3, 1, 2)
            rets[t][head] = v.clone() if head == 'hm' else v       # `loss` applies sigmoid_ to the heat maps in place
        return rets

    def loss_rows(self, example):
        """`loss` for the maps the last `forward_rows_train` produced, on the packed buffer: values and gradients of all
        tasks from the two launches of csrc/loss.hip (`ops.CenterHeadLossFunction`) instead of ~45 autograd ops per task.
        Same dict as `loss` (device tensors; 'loss' entries carry the graph).  None when the path does not apply."""
        stash = self.__dict__.pop("_packed_train", None)
        if stash is None or self.dataset not in ('waymo', 'nuscenes'):
            return None
        out, cols, (B, H, W) = stash
        need = ("hm", "ind", "mask", "cat", "anno_box")
        if any(k not in example for k in need) or not all(torch.is_tensor(v) and v.is_cuda for k in need for v in example[k]):
            return None
        targets = [dict(hm=example["hm"][t].float(), ind=example["ind"][t].long(), mask=example["mask"][t],
                        cat=example["cat"][t].long(), anno_box=example["anno_box"][t].float()) for t in range(len(self.tasks))]
        vals = _ops.CenterHeadLossFunction.apply(out, cols, targets, B, H, W, list(self.code_weights), float(self.weight))
        n = len(self.code_weights)
        det = vals.detach()
        return {"loss": [vals[t, 0] for t in range(len(cols))], "hm_loss": [det[t, 1] for t in range(len(cols))],
                "loc_loss": [det[t, 2] for t in range(len(cols))], "loc_loss_elem": [det[t, 4:4 + n] for t in range(len(cols))],
                "num_positive": [det[t, 3] for t in range(len(cols))]}

    def loss(self, example, preds_dicts, batch_dict=None, host_copies=True, **kwargs):
        """center_head.py:250-298: per task the CornerNet focal loss on the clamped sigmoid heat map
        (losses/centernet_loss.py:29-58) + `weight` x the code-weighted L1 loss of the gathered box regressions
        (:6-27); plain torch (autograd), the targets `hm / ind / mask / cat / anno_box` come with `example` exactly as
        the reference's assigner provides them.  Like the reference it replaces preds_dict['hm'] by its sigmoid in
        place and returns {key: [per-task values]}."""
        from collections import defaultdict
        self.__dict__.pop("_packed_train", None)          # the reference flow head(x) -> head.loss(...) never calls loss_rows
        rets = []
        for task_id, preds_dict in enumerate(preds_dicts):
            preds_dict['hm'] = _clamped_sigmoid(preds_dict['hm'])
            hm_loss = fast_focal_loss(preds_dict['hm'], example['hm'][task_id], example['ind'][task_id],
                                      example['mask'][task_id], example['cat'][task_id])
            target_box = example['anno_box'][task_id]
            if self.dataset not in ('waymo', 'nuscenes'):
                raise NotImplementedError()
            if 'vel' in preds_dict:
                preds_dict['anno_box'] = torch.cat((preds_dict['reg'], preds_dict['height'], preds_dict['dim'],
                                                    preds_dict['vel'], preds_dict['rot']), dim=1)
            else:
                preds_dict['anno_box'] = torch.cat((preds_dict['reg'], preds_dict['height'], preds_dict['dim'],
                                                    preds_dict['rot']), dim=1)
                target_box = target_box[..., [0, 1, 2, 3, 4, 5, -2, -1]]
            box_loss = reg_loss(preds_dict['anno_box'], example['mask'][task_id], example['ind'][task_id], target_box)
            loc_loss = (box_loss * box_loss.new_tensor(self.code_weights)).sum()
            loss = hm_loss + self.weight * loc_loss
            ret = {}
            if batch_dict is not None and "auxseg_loss" in batch_dict:
                auxseg_loss = sum(a[task_id] for a in batch_dict['auxseg_loss'])
                ret['auxseg_loss'] = auxseg_loss
                loss = loss + auxseg_loss
            # `host_copies=False`: the logged values stay on the device (a `.cpu()` here stalls the host until the forward
            # has drained, before it could queue the backward); `training_step` copies them after backward
            keep = (lambda v: v.detach().cpu()) if host_copies else (lambda v: v.detach())
            ret.update({'loss': loss, 'hm_loss': keep(hm_loss), 'loc_loss': loc_loss,
                        'loc_loss_elem': keep(box_loss), 'num_positive': example['mask'][task_id].float().sum()})
            rets.append(ret)
        merged = defaultdict(list)
        for ret in rets:
            for k, v in ret.items():
                merged[k].append(v)
        return merged

    @torch.no_grad()
    def loss_device(self, example, preds_dicts):
        """The same loss values as `loss` for a no-grad evaluation (validation loss, the loss scalars a data-parallel
        step reduces over the ranks), computed by ONE device call for all tasks and samples (csrc/loss.hip) with no host
        round trip; `loss` itself stays the reference's autograd composition for training.  Returns
        {'loss', 'hm_loss', 'loc_loss', 'num_positive': [T] device tensors, 'loc_loss_elem': [T, codes]} -- views
        of one [T, 14] buffer.  Unlike the reference it leaves preds_dict['hm'] untouched (no in-place sigmoid)."""
        if self.dataset not in ('waymo', 'nuscenes'):
            raise NotImplementedError()
        B, _, H, W = preds_dicts[0]['hm'].shape
        tasks = []
        for pd in preds_dicts:
            d = {k: self._rows(pd[k]) for k in ('hm', 'reg', 'height', 'dim', 'rot')}
            if 'vel' in pd:
                d['vel'] = self._rows(pd['vel'])
            tasks.append(d)
        targets = [dict(hm=example['hm'][t], ind=example['ind'][t], mask=example['mask'][t], cat=example['cat'][t],
                        anno_box=example['anno_box'][t]) for t in range(len(preds_dicts))]
        ncodes = 10 if 'vel' in preds_dicts[0] else 8
        if len(self.code_weights) != ncodes:
            raise ValueError("code_weights has %d entries, the head regresses %d codes" % (len(self.code_weights), ncodes))
        out = _ops.centerhead_loss(tasks, targets, B, H, W, self.code_weights, self.weight)
        return {'loss': out[:, 0], 'hm_loss': out[:, 1], 'loc_loss': out[:, 2], 'num_positive': out[:, 3],
                'loc_loss_elem': out[:, 4:4 + ncodes]}

    # ------------------------------------------------------------------ decode + NMS on the device
    @staticmethod
    def _rows(v):
        """NCHW head map -> [B*H*W, C] rows (the reference's own permute(0, 2, 3, 1), center_head.py:321-323); maps that
        are already channels-last views of rows are taken in place."""
        cached = getattr(v, "_df3d_rows", None)
        if cached is not None and cached[2] == v._version and cached[0].dtype == torch.float32:
            return cached[0]
        B, C, H, W = v.shape
        return v.float().permute(0, 2, 3, 1).reshape(B * H * W, C)

    @torch.no_grad()
    def predict_device(self, preds_dicts, test_cfg):
        """-> (boxes [T*B, post_max, 9|7], scores, labels (int32, class offsets applied), counts [T*B]) on the device;
        segment index = task * B + sample.  No host synchronisation."""
        get = test_cfg.get if hasattr(test_cfg, "get") else lambda k, d=None: getattr(test_cfg, k, d)
        if get('double_flip', False):
            raise NotImplementedError("double-flip test-time augmentation is not served by the device tail")
        if get('per_class_nms', False):
            raise NotImplementedError("per_class_nms is a no-op in the reference (center_head.py:431-432)")
        nms = get('nms')
        nms_get = nms.get if hasattr(nms, "get") else lambda k, d=None: getattr(nms, k, d)
        B, _, H, W = preds_dicts[0]['hm'].shape
        tasks, base = [], 0
        for t, pd in enumerate(preds_dicts):
            d = {k: self._rows(pd[k]) for k in ('hm', 'reg', 'height', 'dim', 'rot')}
            if 'vel' in pd:
                d['vel'] = self._rows(pd['vel'])
            d['label_base'] = base
            base += self.num_classes[t]
            tasks.append(d)
        rng = get('post_center_limit_range')
        rng = list(rng) if rng is not None and len(rng) > 0 else None
        if get('circular_nms', False):
            radii = list(get('min_radius'))
            if len(set(float(r) for r in radii)) != 1:
                # per-task radii: one call per task keeps the single-threshold ABI simple
                outs = [_ops.centerhead_predict([tk], B, H, W, get('out_size_factor'), get('voxel_size'), get('pc_range'),
                                                rng, get('score_threshold'), _ops.NMS_CIRCLE, float(radii[i]),
                                                min(4096, H * W), nms_get('nms_post_max_size'))
                        for i, tk in enumerate(tasks)]
                return tuple(torch.cat([o[j] for o in outs]) for j in range(4))
            mode, thr, pre = _ops.NMS_CIRCLE, float(radii[0]), min(4096, H * W)
        else:
            mode, thr, pre = _ops.NMS_ROTATED, float(nms_get('nms_iou_threshold')), int(nms_get('nms_pre_max_size'))
        return _ops.centerhead_predict(tasks, B, H, W, get('out_size_factor'), get('voxel_size'), get('pc_range'), rng,
                                       get('score_threshold'), mode, thr, pre, int(nms_get('nms_post_max_size')))

    @torch.no_grad()
    def predict(self, example, preds_dicts, test_cfg, **kwargs):
        """Reference return format: per sample {'box3d_lidar', 'scores', 'label_preds', 'metadata'} with the tasks'
        detections concatenated in task order (center_head.py:436-457).  One host round trip (the counts)."""
        boxes, scores, labels, counts = self.predict_device(preds_dicts, test_cfg)
        T = len(preds_dicts)
        B = boxes.shape[0] // T
        # (the range flag of the fp16 operand format rides on this copy: ops.read_with_range_flag raises SplitRangeError)
        cnt = _ops.read_with_range_flag(counts.view(T, B))
        metas = example.get("metadata", None) if isinstance(example, dict) else None
        if not metas:
            metas = [None] * B
        out = []
        for b in range(B):
            segs = [(t * B + b, cnt[t][b]) for t in range(T)]
            out.append({'box3d_lidar': torch.cat([boxes[s, :n] for s, n in segs]),
                        'scores': torch.cat([scores[s, :n] for s, n in segs]),
                        'label_preds': torch.cat([labels[s, :n] for s, n in segs]).long(),
                        'metadata': metas[b]})
        return out
