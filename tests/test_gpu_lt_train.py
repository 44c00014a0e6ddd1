"""Training of the LocalTransformer (ACTRv2) on the project's kernels: the backward of the attention inside a group
(df3d_group_attention_backward), the differentiable grouping, the encoder layer and the whole module in train() mode, and the
ACTRv2 tree -- every gradient against float64 (tests/lt_f64_reference.py, checked on the host by test_lt_train_host.py).

The bound is the project's yardstick pattern (test_gpu_tftrain.py:115-123): the error of every tensor against float64,
relative to that tensor's largest entry, next to the error PLAIN fp32 torch arithmetic on the host makes of the same formula;
the largest of ours may be 4 x the largest of the yardstick's + 2e-6.  The figures are printed before they are asserted."""
import copy

import numpy as np
import pytest
import torch

import detgen
import lt_f64_reference as ltr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _within_yardstick(rows, what):
    """rows: (our error, plain fp32 torch's error, L2-relative error, name) per tensor."""
    for r in rows:
        print("%s %-44s ours %.3e  fp32-host %.3e  l2 %.3e" % (what, r[3], r[0], r[1], r[2]))
    ours, yard = max(r[0] for r in rows), max(r[1] for r in rows)
    assert ours <= 4.0 * yard + 2e-6, (what, ours, yard, sorted(rows, reverse=True)[:4])


# --------------------------------------------------------------------------------------- 1. the attention backward kernel
@pytest.mark.parametrize("tokens,groups,heads", [(32, 96, 4), (16, 7, 4), (8, 128, 4), (32, 1, 8), (5, 3, 1)])
def test_group_attention_backward_vs_float64(tokens, groups, heads):
    """`ops.group_attention` under grad: output and grad_qkv against float64 autograd of the written-out formula, next to the
    same formula in plain fp32 torch on the host; two runs give the same bits; every element of grad_qkv is written."""
    from dualfusion import ops
    C = heads * 16
    tag = "gab_%d_%d_%d" % (tokens, groups, heads)
    qkv = torch.from_numpy(detgen.randn(tag + "_qkv", (tokens * groups, 3 * C)))
    go = torch.from_numpy(detgen.randn(tag + "_go", (tokens * groups, C)))

    def host(dtype):
        x = qkv.to(dtype).clone().requires_grad_(True)
        y = ltr.attention(x, tokens, groups, heads)
        (y * go.to(dtype)).sum().backward()
        return y.detach(), x.grad

    y64, g64 = host(torch.float64)
    y32, g32 = host(torch.float32)
    xd = qkv.to(DEV).requires_grad_(True)
    yd = ops.group_attention(xd, tokens, groups, heads)
    (yd * go.to(DEV)).sum().backward()
    _within_yardstick([ltr.errors(yd, y64, y32) + ("out",), ltr.errors(xd.grad, g64, g32) + ("grad_qkv",)], tag)
    # a second run gives the same bits (no atomics), and every element is written (the caller does not zero)
    first = xd.grad.clone()
    xd.grad = None
    (ops.group_attention(xd, tokens, groups, heads) * go.to(DEV)).sum().backward()
    assert torch.equal(first, xd.grad)
    from dualfusion import _lib
    out = torch.full_like(first, float("nan"))
    rc = _lib.load().df3d_group_attention_backward(ops._ptr(xd.detach()), ops._ptr(go.to(DEV)), tokens, groups, heads, 16,
                                                   ops._ptr(out), ops._stream())
    assert rc == 0 and torch.equal(out, first)


def test_group_attention_without_grad_is_the_forward_kernel_alone():
    from dualfusion import ops
    qkv = torch.from_numpy(detgen.randn("gab_plain", (32 * 9, 192))).to(DEV)
    a = ops.group_attention(qkv, 32, 9, 4)
    b = ops.group_attention(qkv.clone().requires_grad_(True), 32, 9, 4)
    assert not a.requires_grad and b.requires_grad and torch.equal(a, b.detach())
    with pytest.raises(Exception):
        ops.group_attention(qkv.clone().requires_grad_(True), 32, 9, 4, split_only=True)


# --------------------------------------------------------------------------------------- 2. grouping / gathering under grad
def test_group_and_gather_points_under_grad_equal_index_add():
    """GroupingOperation.backward / GatherPoints.backward (CP/det3d/ops/group_points/group_points.py:176-206): the gradient
    is scatter-added onto the source points; indices repeat (57 points, 40 x 6 and 90 picks)."""
    from dualfusion import ops
    B, C, N, npnt, ns = 2, 12, 57, 40, 6
    feat = torch.from_numpy(detgen.randn("gpg_f", (B, C, N)))
    rs = np.random.RandomState(3)
    gidx = torch.from_numpy(rs.randint(0, N, (B, npnt, ns)).astype(np.int32))
    aidx = torch.from_numpy(rs.randint(0, N, (B, 90)).astype(np.int32))
    assert len(np.unique(gidx[0].numpy())) < npnt * ns and len(np.unique(aidx[0].numpy())) < 90
    for name, fn, idx in (("group_points", ops.group_points, gidx), ("gather_points", ops.gather_points, aidx)):
        x = feat.to(DEV).requires_grad_(True)
        y = fn(x, idx.to(DEV))
        assert y.requires_grad
        plain = fn(feat.to(DEV), idx.to(DEV))                          # without grad: exactly as before
        assert not plain.requires_grad and torch.equal(plain, y.detach())
        go = torch.from_numpy(detgen.randn("gpg_go_" + name, tuple(y.shape)))
        (y * go.to(DEV)).sum().backward()
        flat = idx.reshape(B, -1).long()
        want = torch.zeros(B, C, N, dtype=torch.float64)
        for b in range(B):
            want[b].index_add_(1, flat[b], go[b].reshape(C, -1).double())
        err = float((x.grad.cpu().double() - want).abs().max() / want.abs().max())
        print(name, "gradient error over scale %.3e" % err)
        assert err <= 1e-6, (name, err)


# --------------------------------------------------------------------------------------- 3. the encoder layer
def _loaded(m):
    sd = detgen.det_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()})
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m


def test_encoder_layer_trains_on_row_kernels_vs_float64():
    """TransformerEncoderLayerPreNorm(64, 4, 128, dropout=0) in train() on [32, 96, 64]: the row-kernel path equals the torch
    composition (`_forward_torch`, called directly) to 1e-5 of scale; input and all 12 parameter gradients against float64."""
    from dualfusion.pointformer import TransformerEncoderLayerPreNorm
    m = _loaded(TransformerEncoderLayerPreNorm(64, 4, 128, dropout=0.0)).train()
    L, G = 32, 96
    x = torch.from_numpy(detgen.randn("ltt_layer_x", (L, G, 64)))
    w = torch.from_numpy(detgen.randn("ltt_layer_g", (L, G, 64)))
    md = copy.deepcopy(m).to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    assert md._train_rows_fit(xd, None, None)
    yd = md(xd)
    ref = md._forward_torch(x.to(DEV))                                    # the torch composition, called directly
    assert float((yd - ref).detach().abs().max()) <= 1e-5 * float(ref.detach().abs().max())
    (yd * w.to(DEV)).sum().backward()

    def host(dtype):
        mm = copy.deepcopy(m).to(dtype)
        xx = x.to(dtype).clone().requires_grad_(True)
        y = ltr.encoder_layer(ltr.module_tensors(mm), xx, 4)
        (y * w.to(dtype)).sum().backward()
        return y.detach(), xx.grad, dict(mm.named_parameters())

    y64, gx64, p64 = host(torch.float64)
    y32, gx32, p32 = host(torch.float32)
    rows = [ltr.errors(yd, y64, y32) + ("out",), ltr.errors(xd.grad, gx64, gx32) + ("input",)]
    mine = dict(md.named_parameters())
    assert len(mine) == 12
    for k in sorted(mine):
        assert mine[k].grad is not None, k
        rows.append(ltr.errors(mine[k].grad, p64[k].grad, p32[k].grad) + (k,))
    _within_yardstick(rows, "layer")
    # another configuration keeps the torch composition (and stays differentiable)
    other = TransformerEncoderLayerPreNorm(64, 2, 128, dropout=0.0).to(DEV).train()
    assert not other._train_rows_fit(xd, None, None)
    assert not md._train_rows_fit(xd, None, torch.zeros(G, L, dtype=torch.bool, device=DEV))


# --------------------------------------------------------------------------------------- 4. the module
@pytest.mark.parametrize("C", [64, 128])
def test_local_transformer_trains_with_the_grouped_gradient_vs_float64(C):
    """LocalTransformer in train() mode on the data of test_local_transformer_chunk_as_fused_launches.  The gradient of the
    loss with respect to the input has two terms: through the kept rows of the points in no group, and through the grouped
    rows of every group a point is in -- a path that groups with a kernel outside autograd loses the second (an error of
    order 1).  C = 128: heads of 32 channels, the torch layers over the differentiable grouping."""
    from dualfusion.pointformer import LocalTransformer
    B, N = 2, 1500
    m = _loaded(LocalTransformer(96, 2.5, 32, C, C, num_layers=2)).train()
    g = torch.Generator().manual_seed(9)
    xyz = torch.rand(B, N, 3, generator=g) * torch.tensor([40.0, 40.0, 3.0])
    rows = torch.randn(B, N, C, generator=g)
    w = torch.from_numpy(detgen.randn("ltt_mod_g_%d" % C, (B, N, C)))
    md = copy.deepcopy(m).to(DEV)
    xd = xyz.to(DEV)
    with torch.no_grad():
        group_idx, group_xyz = md._geometry(xd)
    gi, gxyz = group_idx.cpu().long(), group_xyz.cpu()
    counts = torch.stack([torch.bincount(gi[b].reshape(-1), minlength=N) for b in range(B)])
    assert int((counts == 0).sum()) > 0 and int((counts > 1).sum()) > 0
    # the module writes into its input ('replace'): a non-leaf made from the leaf, permuted as the encoder does
    leaf = rows.clone().to(DEV).requires_grad_(True)
    q = leaf * 1.0
    out = md(xd, q.permute(0, 2, 1))
    assert tuple(out.shape) == (B, N, C)
    assert torch.equal(q.detach(), out.detach())                          # the in-place effect on the caller's tensor
    (out * w.to(DEV)).sum().backward()

    def host(dtype):
        mm = copy.deepcopy(m).to(dtype)
        xx = rows.to(dtype).clone().requires_grad_(True)
        stats = {}
        y = ltr.local_transformer(ltr.module_tensors(mm), gi, gxyz.to(dtype), xx, 4, 2, True, stats)
        (y * w.to(dtype)).sum().backward()
        return y.detach(), xx.grad, dict(mm.named_parameters()), stats

    y64, gx64, p64, stats = host(torch.float64)
    y32, gx32, p32, _ = host(torch.float32)
    res = [ltr.errors(out, y64, y32) + ("out",), ltr.errors(leaf.grad, gx64, gx32) + ("input",)]
    mine = dict(md.named_parameters())
    for k in sorted(mine):
        assert mine[k].grad is not None and p64[k].grad is not None, k
        res.append(ltr.errors(mine[k].grad, p64[k].grad, p32[k].grad) + (k,))
    _within_yardstick(res, "module C=%d" % C)
    assert res[1][2] <= 1e-3, res[1]
    # BatchNorm2d's bookkeeping: momentum 0.1 towards the batch mean / unbiased variance, one batch tracked
    bn, bn0 = md.pe[0].bn, m.pe[0].bn
    assert int(bn.num_batches_tracked) == int(bn0.num_batches_tracked) + 1
    for got, old, new in ((bn.running_mean, bn0.running_mean, stats["mean"]), (bn.running_var, bn0.running_var, stats["var_unbiased"])):
        want = 0.9 * old.double() + 0.1 * new
        assert float((got.cpu().double() - want).abs().max()) <= 1e-5 * float(want.abs().max())


# --------------------------------------------------------------------------------------- 5. the ACTRv2 tree
def test_actrv2_tree_trains_vs_float64():
    """actr.build(..., model_name='ACTRv2') at the configuration of tests/golden/vr_fusion.npz in train() mode, one forward +
    backward of (out * G).sum(), against a float64 deep copy on the host whose LocalTransformers are the yardstick and whose
    deformable sampling is f64_reference.msda_core_f64.  Rectifiers are in, so this is the looser form of
    test_training_step_gradients_vs_float64_composition: direction and size of every gradient (a missing term or a wrong
    kernel is an error of order 1).  Dropout is switched off on both sides: a comparison of two arithmetic paths."""
    import f64_reference as fr
    from dualfusion import actr
    from make_golden import VRF
    lt = dict(VRF["lt"])
    m = actr.build(dict(VRF["actr"]), model_name="ACTRv2", lt_cfg=lt, hybrid_cfg=dict(VRF["hybrid"], gate_before_ffn=True))
    _loaded(m).train()
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    B, Q, (H, W) = 2, 260, VRF["hw"]
    v = torch.from_numpy(detgen.randn("ltt_tree_v", (B, Q, 64)))
    grid = torch.from_numpy(detgen.rand("ltt_tree_grid", (B, Q, 2), 0.05, 0.95))
    img = torch.from_numpy(detgen.randn("ltt_tree_img", (B, 256, H // 4, W // 4)))
    lo, hi = np.array([4.0, -12.0, -2.6], np.float32), np.array([45.0, 12.0, 0.6], np.float32)
    lid = torch.from_numpy(detgen.rand("ltt_tree_lid", (B, Q, 3)) * (hi - lo) + lo)
    vi = torch.from_numpy(detgen.randn("ltt_tree_vi", (B, Q, 256)))
    G = torch.from_numpy(detgen.randn("ltt_tree_G", (B, Q, 64)))
    md = copy.deepcopy(m).to(DEV)
    lid_d = lid.to(DEV)
    out = md(v_feat=v.clone().to(DEV), grid=grid.to(DEV), i_feats=[img.to(DEV)], v_i_feat=vi.to(DEV), lidar_grid=lid_d)
    (out * G.to(DEV)).sum().backward()
    with torch.no_grad():
        group_idx, group_xyz = md.transformer.encoder.lidar_attns[0]._geometry(lid_d)
    gi, gxyz = group_idx.cpu().long(), group_xyz.cpu().double()

    d64 = copy.deepcopy(m).double()
    for mod in d64.transformer.encoder.lidar_attns:
        mod.forward = (lambda xyz, features, mod=mod: ltr.local_transformer(
            ltr.module_tensors(mod), gi, gxyz, features.permute(0, 2, 1), 4, lt["num_layers"], True))
    with fr.patched():
        out64 = d64(v_feat=v.double(), grid=grid.double(), i_feats=[img.double()], v_i_feat=vi.double(), lidar_grid=lid.double())
        (out64 * G.double()).sum().backward()
    assert float((out.detach().cpu().double() - out64.detach()).abs().max()) <= 1e-4 * float(out64.detach().abs().max())
    want = dict(d64.named_parameters())
    l2 = []
    for k, p in md.named_parameters():
        wg = want[k].grad
        if wg is None:                                              # never reached, in the reference as here
            assert p.grad is None or float(p.grad.abs().max()) == 0, k
            continue
        if float(wg.abs().max()) < 1e-12:                           # exactly-cancelling sums: noise
            assert p.grad is not None and float(p.grad.abs().max()) < 1e-6, k
            continue
        assert p.grad is not None, k
        l2.append((float((p.grad.double().cpu() - wg).norm() / wg.norm()), k))
    for e, k in sorted(l2, reverse=True)[:8]:
        print("tree %-70s l2 %.3e" % (k, e))
    errs = np.array([e for e, _ in l2])
    print("tree: %d gradients, worst %.3e, median %.3e" % (len(errs), errs.max(), np.median(errs)))
    assert sum("lidar_attns" in k for _, k in l2) == 4 * 29     # every parameter of the four LocalTransformers
    assert errs.max() <= 2e-2 and np.median(errs) <= 1e-3, sorted(l2, reverse=True)[:6]
