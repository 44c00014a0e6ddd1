"""The leaves of the bf16 mixed-precision training mode (BASELINE configs[2] / [3]; `bench.py --workload tf_fusion` runs it by
default) against float64 on the SAME rounded operands.

The contract of every bf16 kernel: operands rounded to bfloat16 (round to nearest even) where the kernel stages them, products of
two bf16 values exact in fp32, fp32 accumulation.  So the reference rounds the same operands with torch's `.bfloat16()` and
computes in float64; the kernel then agrees at the grade of fp32 accumulation (2e-5 of scale for products, 4e-6 for filter
gradients), and where the product rounds its OUTPUT to bfloat16 within one bf16 ulp per element.  A bound taken against the
UNROUNDED operands has to be bf16-sized (~1e-2) and cannot see a wrong rounding, a bf16 accumulator or a silent fall-back to
another path.  Every rounded result of a sparse convolution, and linear_bf16's weight gradient, also asserts that its rounding
is observable (far from the unrounded reference); linear_bf16's y and d x are bfloat16 tensors, rounded by their dtype."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

PROD, WGRAD = 2e-5, 4e-6                        # fp32-accumulation bounds of the suite (of the reference's largest entry)


def _r(t):
    """bf16 rounding (RNE) of a host tensor, back in float64."""
    return t.bfloat16().double()


def _err(got, ref):
    """max |got - ref| / max |ref|, on the host in float64."""
    ref = ref.detach().double().cpu()
    return float((got.detach().double().cpu() - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


def _bf16_ulp(ref):
    """One bf16 ulp of every element of a float64 tensor (8 significant bits: |v| in [2^(e-1), 2^e) -> 2^(e-8))."""
    _, e = torch.frexp(ref)
    return torch.ldexp(torch.ones_like(ref), e - 8)


def _within_one_ulp(got, ref, name):
    """|got - ref| <= one bf16 ulp of ref per element; the floor 2^-20 of scale covers the fp32 accumulation under the
    elements that cancel to (nearly) zero."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    tol = _bf16_ulp(ref) + 2.0 ** -20 * float(ref.abs().max())
    bad = (got - ref).abs() > tol
    assert not bool(bad.any()), (name, int(bad.sum()), float(((got - ref).abs() / tol).max()))


# ------------------------------------------------------------------------------------------------ a. SparseConvFunction, bf16
def _voxels(seed, batch, shape, n_seeds, walk):
    """Distinct, spatially clustered voxels [n, 4] (batch, z, y, x) int32 -- random walks, so neighbourhoods are populated."""
    rs = np.random.RandomState(seed)
    seen, out = set(), []
    for b in range(batch):
        for _ in range(n_seeds):
            p = np.array([rs.randint(0, s) for s in shape])
            for _ in range(walk):
                p = np.clip(p + rs.randint(-1, 2, size=3), 0, np.array(shape) - 1)
                k = (b,) + tuple(int(v) for v in p)
                if k not in seen:
                    seen.add(k)
                    out.append(k)
    return np.asarray(out, np.int32)


def _table(kind, seed):
    """-> (nbr [K, n_out] int32 on the device, n_in, mirror) for one layer class of the reduced TransFusion tree.  One offset
    (with its mirror image where the table serves as its own inverse) is emptied: an offset with no pairs."""
    from dualfusion import ops
    geo, ks = kind[0], kind[1]
    if geo in ("subm", "down"):
        shape = [41, 160, 160]
        ind = torch.from_numpy(_voxels(seed, 2, shape, 9, 420)).to(DEV)
        grid = ops.grid_build(ind, 2, shape)
        if geo == "subm":
            nbr, n_in, mirror = ops.subm_neighbors(grid, ind, ks), ind.shape[0], True
        else:
            stride, pad = kind[2], kind[3]
            oshape = [(v + 2 * p - k) // s + 1 for v, k, s, p in zip(shape, ks, stride, pad)]
            out_ind, _ = ops.conv_out_indices(ind, 2, shape, oshape, ks, stride, pad)
            nbr, n_in, mirror = ops.conv_neighbors(grid, out_ind.contiguous(), ks, stride, pad), ind.shape[0], False
    else:                                                       # BEV pixel rows of the neck: (B, H, W) row-major
        B, H, W = 3, 21, 21
        kh, stride, pad, transposed = ks, kind[2], kind[3], geo == "deconv"
        nbr, _, _ = ops.conv2d_neighbors(B, H, W, kh, kh, stride, pad, transposed, DEV)
        n_in, mirror = B * H * W, (not transposed) and stride == 1 and kh % 2 == 1
    nbr = nbr.clone()
    K = nbr.shape[0]
    if K > 1:
        k0 = 1
        nbr[k0] = -1
        if mirror:
            nbr[K - 1 - k0] = -1
    assert int((nbr >= 0).sum()) > 0
    return nbr.contiguous(), int(n_in), mirror


def _conv64(x, w, nbr, n_out):
    """float64 host reference: out[o] = sum_k x[nbr[k, o]] @ w[k] (w [K, cin, cout])."""
    out = torch.zeros((n_out, w.shape[2]), dtype=torch.float64)
    for k in range(nbr.shape[0]):
        m = nbr[k] >= 0
        if bool(m.any()):
            out[m] += x[nbr[k][m].long()] @ w[k]
    return out


def _conv64_backward(x, w, g, nbr, n_in):
    """-> (d x, d w) of _conv64 for the output gradient g, in float64."""
    gx = torch.zeros((n_in, w.shape[1]), dtype=torch.float64)
    gw = torch.zeros_like(w)
    for k in range(nbr.shape[0]):
        m = nbr[k] >= 0
        if bool(m.any()):
            i = nbr[k][m].long()
            gx.index_add_(0, i, g[m] @ w[k].T)
            gw[k] = x[i].T @ g[m]
    return gx, gw


# (name, geometry, cin, cout, forward bf16, input gradient bf16, filter gradient bf16) -- the expected path of every class the
# reduced TransFusion tree sends through SparseConvFunction in the bf16 mode, written out: the forward and the input gradient
# where ops.conv_bf16_supported(K, cin, cout) / (K, cout, cin) holds (csrc/spconv_split.hip bf16_shape_ok), the filter gradient
# where df3d_sparse_conv_grad_filters_bf16 takes the bf16 kernel (channel counts divisible by 4 and >= 64); everything else runs
# the exact-fp32 kernels
CONV_CLASSES = [
    # sparse encoder (SubM basic blocks, strided downsampling, conv_out)
    ("enc_subm16", ("subm", [3, 3, 3]), 16, 16, False, False, False),
    ("enc_subm32", ("subm", [3, 3, 3]), 32, 32, True, True, False),
    ("enc_subm64", ("subm", [3, 3, 3]), 64, 64, True, True, True),
    ("enc_subm128", ("subm", [3, 3, 3]), 128, 128, True, True, True),
    ("enc_down16_32", ("down", [3, 3, 3], [2, 2, 2], [1, 1, 1]), 16, 32, False, False, False),
    ("enc_down32_64", ("down", [3, 3, 3], [2, 2, 2], [1, 1, 1]), 32, 64, True, True, False),       # input gradient 64 -> 32
    ("enc_down64_128", ("down", [3, 3, 3], [2, 2, 2], [0, 1, 1]), 64, 128, True, True, True),      # input gradient 128 -> 64
    ("enc_out128", ("down", [3, 1, 1], [2, 1, 1], [0, 0, 0]), 128, 128, True, True, True),
    # SECOND / SECONDFPN rows (necks._train_stack): 3 x 3 (K = 9), strided 3 x 3, the 1 x 1 layer, the 2 x 2 transposed layer
    ("neck_3x3_256_128", ("conv", 3, 1, 1), 256, 128, True, True, True),
    ("neck_3x3_128_128", ("conv", 3, 1, 1), 128, 128, True, True, True),
    ("neck_3x3s2_128_256", ("conv", 3, 2, 1), 128, 256, True, True, True),
    ("neck_3x3_256_256", ("conv", 3, 1, 1), 256, 256, True, True, True),
    ("neck_1x1_128_256", ("conv", 1, 1, 0), 128, 256, True, True, True),
    ("neck_deconv2x2_256_256", ("deconv", 2, 2, 0), 256, 256, True, True, True),
]


@pytest.mark.parametrize("name,kind,cin,cout,fwd16,din16,dw16", CONV_CLASSES, ids=[c[0] for c in CONV_CLASSES])
def test_sparse_conv_function_bf16_vs_float64_on_rounded_operands(name, kind, cin, cout, fwd16, din16, dw16):
    """SparseConvFunction in the bf16 mode, forward and backward, per layer class: the output, the input gradient and the
    filter gradient against float64 of the operands rounded where the expected path rounds them (fp32-grade of the unrounded
    operands elsewhere), the bias gradient as the fp32 column sum.  Ragged row counts, one offset without pairs."""
    from dualfusion import ops
    from dualfusion.spconv.conv import SparseConvFunction
    nbr, n_in, mirror = _table(kind, seed=cin * 7 + cout)
    K, n_out = nbr.shape
    gen = torch.Generator().manual_seed(K * 1000 + cin + cout)
    x = torch.randn((n_in, cin), generator=gen)
    w = torch.randn((K, cin, cout), generator=gen) * (1.0 / np.sqrt(K * cin))
    b = torch.randn((cout,), generator=gen)
    g = torch.randn((n_out, cout), generator=gen)
    xa, wa, ba = (t.to(DEV).requires_grad_(True) for t in (x, w, b))
    with ops.precision("bf16"):
        y = SparseConvFunction.apply(xa, wa, ba, nbr, n_out, mirror, None)
    y.backward(g.to(DEV))
    assert y.dtype == torch.float32 and xa.grad.dtype == wa.grad.dtype == torch.float32

    t = nbr.cpu()
    x64, w64, g64 = x.double(), w.double(), g.double()
    rx, rw, rg = _r(x), _r(w), _r(g)
    exact_y = _conv64(x64, w64, t, n_out) + b.double()
    exact_gx, exact_gw = _conv64_backward(x64, w64, g64, t, n_in)
    want_y = _conv64(rx, rw, t, n_out) + b.double() if fwd16 else exact_y
    want_gx = _conv64_backward(rx, rw, rg, t, n_in)[0] if din16 else exact_gx
    want_gw = _conv64_backward(rx, rw, rg, t, n_in)[1] if dw16 else exact_gw
    for got, want, exact, rounded, bound, what in ((y, want_y, exact_y, fwd16, PROD, "y"),
                                                   (xa.grad, want_gx, exact_gx, din16, PROD, "d features"),
                                                   (wa.grad, want_gw, exact_gw, dw16, WGRAD, "d filters")):
        err = _err(got, want)
        assert err <= bound, (name, what, err)
        if rounded:                    # the bf16 path did run: the result is nowhere near the unrounded operands' value
            far = _err(got, exact)
            assert far >= 20 * bound, (name, what, "rounding not observed", far)
    assert _err(ba.grad, g64.sum(0)) <= WGRAD, name


# ------------------------------------------------------------------------------------------------------------ b. linear_bf16
LINEAR_SHAPES = [
    ("per_sample", (6, 3001)),          # 3-D input: one batched product over the samples
    ("per_sample_b1", (1, 3001)),
    ("chunks16", (16 * 1031,)),         # 2-D, rows a multiple of 16 and >= 16384: 16 row chunks
    ("one_product", (5003,)),           # 2-D, rows not a multiple of 16: one product
]


@pytest.mark.parametrize("cin,cout", [(128, 256), (256, 128), (128, 1024), (1024, 128)])
@pytest.mark.parametrize("branch,rows", LINEAR_SHAPES, ids=[s[0] for s in LINEAR_SHAPES])
@pytest.mark.parametrize("bias", [True, False])
def test_linear_bf16_vs_float64_on_rounded_operands(branch, rows, cin, cout, bias):
    """`linear_bf16` (the feed-forward linears of the bf16 training step) on its three weight-gradient branches: y and d x within
    one bf16 ulp of float64 on the rounded x, W, b and gradient (the products round their outputs to bf16), d W within 1e-5 of
    scale (fp32 partials, fp32 sum), d b the fp32 sum of the rounded gradient."""
    from dualfusion.linear_rows import linear_bf16
    gen = torch.Generator().manual_seed(cin * 31 + cout + len(rows))
    x = torch.randn(rows + (cin,), generator=gen)
    w = torch.randn((cout, cin), generator=gen) * (1.0 / np.sqrt(cin))
    b = torch.randn((cout,), generator=gen) if bias else None
    g = torch.randn(rows + (cout,), generator=gen)
    xa, wa = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
    ba = b.to(DEV).requires_grad_(True) if bias else None
    y = linear_bf16(xa, wa, ba)
    assert y.dtype == torch.bfloat16 and y.shape == rows + (cout,)
    y.backward(g.to(DEV).to(torch.bfloat16))
    assert xa.grad.dtype == wa.grad.dtype == torch.float32

    rx, rw, rg = _r(x), _r(w), _r(g)
    want_y = rx @ rw.T + (_r(b) if bias else 0.0)
    _within_one_ulp(y, want_y, "y")
    _within_one_ulp(xa.grad, rg @ rw, "dx")
    want_w = rg.reshape(-1, cout).T @ rx.reshape(-1, cin)
    err = _err(wa.grad, want_w)
    assert err <= 1e-5, ("dw", branch, err)
    far = _err(wa.grad, g.double().reshape(-1, cout).T @ x.double().reshape(-1, cin))
    assert far >= 20 * 1e-5, ("dw: rounding of the operands not observed", far)
    if bias:
        assert ba.grad.dtype == torch.float32
        assert _err(ba.grad, rg.reshape(-1, cout).sum(0)) <= WGRAD


# ----------------------------------------------------------------------------------------------- c. relu_dropout_ on bf16 rows
@pytest.mark.parametrize("n", [1, 7] + [8 * 37 + r for r in range(1, 8)] + [(1 << 20) + 8 * 5])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_relu_dropout_bf16_rows_bit_exact(n, p):
    """df3d_relu_dropout_bf16 / _backward_bf16 on element counts that end in the kernel's tail branch (cnt < 8: 1, 7, 8k + r)
    and one large count, bit for bit: forward (h * scale) rounded to bf16 where the fp32 kernel under the same seed keeps an
    active element, backward (g * scale) rounded to bf16 where the forward's result is non-zero."""
    from dualfusion import ops
    gen = torch.Generator().manual_seed(n * 10 + int(p * 10))
    h16 = torch.randn((n,), generator=gen).bfloat16()
    if n > 2:
        h16[1] = 0.0                                            # an exact zero and a negative zero stay zero
        h16[2] = -0.0
    g16 = torch.randn((n,), generator=gen).bfloat16()
    seed = 4242 + n
    kept = (ops.relu_dropout_(h16.float().to(DEV), p, seed=seed) != 0).cpu()      # the fp32 kernel's mask
    thr = int(ctypes.c_float(p).value * 16777216.0)
    scale = float(np.float32(1.0 / (1.0 - thr / 16777216.0))) if thr else 1.0
    want = torch.where(kept, (h16.float() * scale).bfloat16(), torch.zeros((), dtype=torch.bfloat16))
    leaf = h16.to(DEV).requires_grad_(True)
    out = ops.relu_dropout_(leaf * 1, p, seed=seed)
    assert out.dtype == torch.bfloat16
    got = out.detach().cpu()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (n, p)
    if p == 0.0:
        assert torch.equal(kept, h16.float() > 0)
    out.backward(g16.to(DEV))
    want_g = torch.where(got != 0, (g16.float() * scale).bfloat16(), torch.zeros((), dtype=torch.bfloat16))
    assert leaf.grad.dtype == torch.bfloat16
    assert torch.equal(leaf.grad.cpu().view(torch.int16), want_g.view(torch.int16)), (n, p)


# ------------------------------------------------------------------------------------------- d. dropout_add_layernorm edges
def test_dropout_add_layernorm_below_the_threshold_grain():
    """0 < p < 2^-24: the kernel's 24-bit threshold is 0, it drops nothing and writes no d y -- the gradient of the dropped input
    is then d x, not whatever the caching allocator handed back for it (blocks of the same size are filled and freed first)."""
    from dualfusion import ops
    rows, C = 777, 64
    gen = torch.Generator().manual_seed(5)
    x, y, g = (torch.randn((rows, C), generator=gen) for _ in range(3))
    norm = torch.nn.LayerNorm(C).to(DEV)
    drop = torch.nn.Dropout(1e-8).train()
    xa, ya = x.to(DEV).requires_grad_(True), y.to(DEV).requires_grad_(True)
    out = ops.dropout_add_layernorm(xa, ya, norm, drop)
    assert type(out.grad_fn).__name__ == "_DropoutAddLayerNormBackward"
    stale = [torch.full((rows, C), float("nan"), device=DEV) for _ in range(4)]
    del stale
    out.backward(g.to(DEV))
    assert torch.isfinite(xa.grad).all()
    assert torch.equal(ya.grad, xa.grad)


@pytest.mark.parametrize("C", [4, 128, 1024])
def test_dropout_add_layernorm_single_row(C):
    """One row in all (one wave group holds it, every other lane idle) at the narrowest, a middle and the widest channel count:
    output, d x = d y, d gamma, d beta against nn.LayerNorm in float64 (p = 0)."""
    from dualfusion import ops
    gen = torch.Generator().manual_seed(C)
    x, y, g = (torch.randn((1, C), generator=gen) for _ in range(3))
    norm = torch.nn.LayerNorm(C)
    with torch.no_grad():
        norm.weight.copy_(torch.rand(C, generator=gen) + 0.5)
        norm.bias.copy_(torch.randn(C, generator=gen))
    nd = torch.nn.LayerNorm(C).to(DEV)
    nd.load_state_dict(norm.state_dict())
    xa, ya = x.to(DEV).requires_grad_(True), y.to(DEV).requires_grad_(True)
    out = ops.dropout_add_layernorm(xa, ya, nd, torch.nn.Dropout(0.0))
    assert type(out.grad_fn).__name__ == "_DropoutAddLayerNormBackward"
    out.backward(g.to(DEV))
    n64 = norm.double()
    xr, yr = x.double().requires_grad_(True), y.double().requires_grad_(True)
    ref = n64(xr + yr)
    ref.backward(g.double())
    for a, b, name in ((out, ref, "out"), (xa.grad, xr.grad, "dx"), (ya.grad, yr.grad, "dy"),
                       (nd.weight.grad, n64.weight.grad, "dgamma"), (nd.bias.grad, n64.bias.grad, "dbeta")):
        err = float((a.detach().cpu().double() - b.detach()).abs().max()) / max(1.0, float(b.detach().abs().max()))
        assert err <= (2e-5 if name in ("dgamma", "dbeta") else 5e-6), (name, C, err)
