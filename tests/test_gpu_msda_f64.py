"""Multi-scale deformable attention in float64 on the device (csrc/msda_f64.hip: df3d_ms_deform_attn_forward_f64 /
_backward_f64), the second type of the reference's dispatch and the one its acceptance script ops/test.py runs: allclose against
the torch core in double, torch.autograd.gradcheck on MSDeformAttnFunction.apply.

The reference side of every comparison is tests/f64_reference.py::msda_core_f64 on CPU float64 tensors and torch autograd
through it (except the device-reference case, which compares the float32 kernels with the float64 ones at a size the host
cannot do in the time a test has).

Inputs: a sampling point on a pixel line makes the bilinear kernel non-differentiable, so locations are made in pixel space as
an integer, uniform over -2 .. size inclusive (fully outside, the half-covered border band, the interior), plus a fraction in
[0.1, 0.9], then normalised: loc = (int + frac + 0.5) / size per level and axis.  Every point is then >= 0.1 px from a line
(asserted).  Attention weights are a softmax over L * P, values are randn.

Bound against the host reference: 1e-10 of scale, max |got - want| / max(1, max |want|).  The longest sum in these cases has
~6 000 terms (1025 channels x 4 corners; 6 000 contributions to one pixel): worst-case rounding 6 000 x 1.1e-16 ~ 7e-13 of the
sum of absolute terms; 1e-10 leaves two orders of magnitude for cancellation in the location gradient, and any indexing or
weight error is 1e-3 or worse.  Measured maxima are recorded in DESIGN.md section 4."""
import copy
import sys

import numpy as np
import pytest

import f64_reference as fr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BOUND = 1e-10
SCRIPT_DIMS = dict(N=1, M=2, Lq=2, P=2, maps=[(6, 4), (3, 2)])           # the reference script's own geometry
ANALYTIC_DIMS = dict(N=2, M=3, Lq=37, P=3, maps=[(5, 7), (3, 2)])


def _dev():
    return torch.device("cuda:0")


def _starts(maps):
    out, run = [], 0
    for h, w in maps:
        out.append(run)
        run += h * w
    return out


def _locations(rs, N, Lq, M, P, maps, fixed_int=None):
    """-> [N, Lq, M, L, P, 2] float64 (x, y), by the recipe of the module docstring; fixed_int (iy, ix): every point in that
    pixel cell."""
    loc = np.empty((N, Lq, M, len(maps), P, 2))
    for lvl, (H, W) in enumerate(maps):
        for axis, size in ((0, W), (1, H)):
            if fixed_int is None:
                whole = rs.randint(-2, size + 1, (N, Lq, M, P))
            else:
                whole = np.full((N, Lq, M, P), fixed_int[1 - axis])
            loc[:, :, :, lvl, :, axis] = (whole + rs.uniform(0.1, 0.9, (N, Lq, M, P)) + 0.5) / size
    for lvl, (H, W) in enumerate(maps):                              # the property the recipe is for
        for axis, size in ((0, W), (1, H)):
            pix = loc[:, :, :, lvl, :, axis] * size - 0.5
            assert np.abs(pix - np.round(pix)).min() >= 0.1 - 1e-9
    return loc


def _case(seed, N, M, D, Lq, P, maps, fixed_int=None):
    """Host float64 tensors (value, loc, aw, gout) of one case."""
    rs = np.random.RandomState(seed)
    S, L = sum(h * w for h, w in maps), len(maps)
    value = rs.standard_normal((N, S, M, D))
    loc = _locations(rs, N, Lq, M, P, maps, fixed_int)
    logits = rs.standard_normal((N, Lq, M, L * P))
    aw = np.exp(logits - logits.max(-1, keepdims=True))
    aw = (aw / aw.sum(-1, keepdims=True)).reshape(N, Lq, M, L, P)
    gout = rs.standard_normal((N, Lq, M * D))
    return tuple(torch.from_numpy(np.ascontiguousarray(a)) for a in (value, loc, aw, gout))


_REFERENCES = {}


def _reference(key, maps, value, loc, aw, gout):
    """(out, grad_value, grad_loc, grad_aw) of the host composition in float64, evaluated once per case and kept."""
    if key not in _REFERENCES:
        v, l, a = (t.clone().requires_grad_(True) for t in (value, loc, aw))
        out = fr.msda_core_f64(v, maps, l, a)
        out.backward(gout)
        _REFERENCES[key] = (out.detach(), v.grad, l.grad, a.grad)
    return _REFERENCES[key]


def _level_tensors(maps):
    shapes = torch.as_tensor(maps, dtype=torch.long, device=_dev())
    return shapes, torch.as_tensor(_starts(maps), dtype=torch.long, device=_dev())


def _err(got, want):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    return float((got - want).abs().max()) / max(1.0, float(want.abs().max()))


def _device_run(maps, value, loc, aw, gout):
    """(out, grad_value, grad_loc, grad_aw) through ops.ms_deform_attn_forward / _backward on the device."""
    from dualfusion import ops
    shapes, lstart = _level_tensors(maps)
    v, l, a, g = (t.to(_dev()) for t in (value, loc, aw, gout))
    out = ops.ms_deform_attn_forward(v, shapes, lstart, l, a)
    return (out,) + tuple(ops.ms_deform_attn_backward(v, shapes, lstart, l, a, g))


def _check_against_reference(key, maps, case, label):
    want = _reference(key, maps, *case)
    got = _device_run(maps, *case)
    errs = {}
    for name, g, w in zip(("out", "grad_value", "grad_loc", "grad_aw"), got, want):
        assert g.dtype == torch.float64 and tuple(g.shape) == tuple(w.shape), name
        errs[name] = _err(g, w)
    print("%s: %s" % (label, ", ".join("%s %.3e" % kv for kv in errs.items())))
    for name, e in errs.items():
        assert e <= BOUND, (label, name, e)
    return got, want


# ------------------------------------------------------------------------------------------- 1. the reference script, restated
def _shim_function():
    """An autograd Function on the installed `MultiScaleDeformableAttention` module, bound the way the reference's
    ms_deform_attn_func.py binds the compiled one."""
    from dualfusion import ext
    had = sys.modules.pop("MultiScaleDeformableAttention", None)
    try:
        ext.install()
        import MultiScaleDeformableAttention as MSDA
    finally:
        if had is not None:
            sys.modules["MultiScaleDeformableAttention"] = had

    class ShimFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, value, shapes, lstart, loc, aw, im2col_step):
            ctx.im2col_step = im2col_step
            ctx.save_for_backward(value, shapes, lstart, loc, aw)
            return MSDA.ms_deform_attn_forward(value, shapes, lstart, loc, aw, im2col_step)

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, grad_output):
            value, shapes, lstart, loc, aw = ctx.saved_tensors
            gv, gl, ga = MSDA.ms_deform_attn_backward(value, shapes, lstart, loc, aw, grad_output.contiguous(), ctx.im2col_step)
            assert gv.dtype == gl.dtype == ga.dtype == torch.float64
            return gv, None, None, gl, ga, None

    return ShimFunction


def _function(path):
    if path == "shim":
        return _shim_function()
    from dualfusion.msda import MSDeformAttnFunction
    return MSDeformAttnFunction


@pytest.mark.parametrize("path", ["msda", "shim"])
def test_forward_equals_the_torch_core_in_double(path):
    """check_forward_equal_with_pytorch_double (ops/test.py): torch.allclose at default tolerances."""
    d = SCRIPT_DIMS
    value, loc, aw, _ = _case(11, d["N"], d["M"], 2, d["Lq"], d["P"], d["maps"])
    shapes, lstart = _level_tensors(d["maps"])
    out = _function(path).apply(value.to(_dev()), shapes, lstart, loc.to(_dev()), aw.to(_dev()), 2)
    assert out.dtype == torch.float64
    want = fr.msda_core_f64(value, d["maps"], loc, aw)
    assert torch.allclose(out.cpu(), want)
    assert float(want.abs().max()) > 0


@pytest.mark.parametrize("path", ["msda", "shim"])
@pytest.mark.parametrize("D", [2, 4, 30])
def test_gradcheck_with_default_arguments(path, D):
    """check_gradient_numerical (ops/test.py): gradcheck on the Function with all three floating inputs requiring grad.  It
    also runs the backward twice and compares bit for bit (nondet_tol = 0)."""
    d = SCRIPT_DIMS
    value, loc, aw, _ = _case(20 + D, d["N"], d["M"], D, d["Lq"], d["P"], d["maps"])
    shapes, lstart = _level_tensors(d["maps"])
    v, l, a = (t.to(_dev()).requires_grad_(True) for t in (value, loc, aw))
    assert torch.autograd.gradcheck(_function(path).apply, (v, shapes, lstart, l, a, 2))


# --------------------------------------------------------------------- 2. analytic gradients against autograd of the composition
@pytest.mark.parametrize("D", [1, 30, 71, 1025])
def test_forward_and_gradients_against_float64_autograd(D):
    d = ANALYTIC_DIMS
    case = _case(100 + D, d["N"], d["M"], D, d["Lq"], d["P"], d["maps"])
    _check_against_reference(("analytic", D), d["maps"], case, "case 2, D = %d" % D)


# ------------------------------------------------------------------------------------------------------------ 3. one hot pixel
HOT_MAPS = [(4, 4)]


def _hot_case():
    """Every point of 1500 queries x 4 points in pixel cell (1, 2): rows (1, 2), (1, 3), (2, 2), (2, 3) of each head receive
    6 000 contributions each -- the long-segment ordering."""
    return _case(7, 1, 2, 16, 1500, 4, HOT_MAPS, fixed_int=(1, 2))


def test_one_hot_pixel():
    got, want = _check_against_reference("hot", HOT_MAPS, _hot_case(), "case 3, hot pixel")
    gv = want[1].view(4, 4, 2, 16)
    touched = gv.abs().sum((-1, -2)) > 0
    assert touched.nonzero().tolist() == [[1, 2], [1, 3], [2, 2], [2, 3]]
    assert torch.equal(got[1].cpu().view(4, 4, 2, 16)[~touched], torch.zeros_like(gv[~touched]))


# --------------------------------------------------------------------------------------------------------- 4. reproducibility
@pytest.mark.parametrize("which", ["hot", "analytic_D30"])
def test_backward_is_bit_reproducible(which):
    from dualfusion import ops
    if which == "hot":
        maps, case = HOT_MAPS, _hot_case()
    else:
        d = ANALYTIC_DIMS
        maps, case = d["maps"], _case(130, d["N"], d["M"], 30, d["Lq"], d["P"], d["maps"])
    other_maps = [(3, 5)]
    other = [t.to(_dev()) for t in _case(5, 2, 2, 8, 50, 2, other_maps)]
    oshapes, ostart = _level_tensors(other_maps)
    shapes, lstart = _level_tensors(maps)
    v, l, a, g = (t.to(_dev()) for t in case)
    runs = []
    for _ in range(3):
        runs.append(ops.ms_deform_attn_backward(v, shapes, lstart, l, a, g))
        ops.ms_deform_attn_backward(other[0], oshapes, ostart, other[1], other[2], other[3])     # an unrelated backward between
    for again in runs[1:]:
        for name, x, y in zip(("grad_value", "grad_loc", "grad_aw"), runs[0], again):
            assert torch.equal(x, y), name


# -------------------------------------------------------------------------------------------------- 5. empty rows, no pre-fill
def test_grad_value_needs_no_prefill_and_empty_rows_are_zero(monkeypatch):
    from dualfusion import ops
    d = ANALYTIC_DIMS
    case = _case(55, d["N"], d["M"], 5, 3, 1, d["maps"])               # 3 queries x 1 point per level: most rows untouched
    want = _reference("sparse", d["maps"], *case)
    shapes, lstart = _level_tensors(d["maps"])
    v, l, a, g = (t.to(_dev()) for t in case)
    poisoned = []

    def nan_like(t, **kw):
        poisoned.append(tuple(t.shape))
        return torch.full_like(t, float("nan"), **kw)

    monkeypatch.setattr(torch, "empty_like", nan_like)
    gv, gl, ga = ops.ms_deform_attn_backward(v, shapes, lstart, l, a, g)
    monkeypatch.undo()
    assert tuple(v.shape) in poisoned                                  # (the output buffers did hold NaNs)
    for name, got, w in zip(("grad_value", "grad_loc", "grad_aw"), (gv, gl, ga), want[1:]):
        assert not torch.isnan(got).any(), name
        assert _err(got, w) <= BOUND, name
    empty = want[1].abs().sum(-1) == 0                                 # [N, S, M]: rows no corner touches
    assert empty.any() and (~empty).any()
    assert torch.equal(gv.cpu()[empty], torch.zeros_like(want[1][empty]))


# ------------------------------------------------------------------------------------------- 6. the device reference in use
def test_float32_kernels_against_the_float64_ones_on_the_device():
    """N = 2, one 40 x 56 level, M = 8, D = 16, Lq = 3000, P = 4: the existing float32 forward and backward against the float64
    ones on the same (float32-representable) inputs, all on the device.  Tolerances: the project's own for these kernels
    (tests/test_gpu_ops.py: forward rtol 1e-3, atol 2e-5; backward <= 1e-4 of scale)."""
    from dualfusion import ops
    maps = [(40, 56)]
    case32 = [t.float().to(_dev()) for t in _case(66, 2, 8, 16, 3000, 4, maps)]
    case64 = [t.double() for t in case32]
    pix = case64[1].cpu() * torch.tensor([56.0, 40.0], dtype=torch.float64) - 0.5
    assert float((pix - pix.round()).abs().min()) >= 0.09              # (still off the pixel lines after the cast to float)
    shapes, lstart = _level_tensors(maps)
    out32 = ops.ms_deform_attn_forward(case32[0], shapes, lstart, case32[1], case32[2])
    out64 = ops.ms_deform_attn_forward(case64[0], shapes, lstart, case64[1], case64[2])
    assert out32.dtype == torch.float32 and out64.dtype == torch.float64
    np.testing.assert_allclose(out32.cpu().numpy(), out64.float().cpu().numpy(), rtol=1e-3, atol=2e-5)
    g32 = ops.ms_deform_attn_backward(case32[0], shapes, lstart, case32[1], case32[2], case32[3])
    g64 = ops.ms_deform_attn_backward(case64[0], shapes, lstart, case64[1], case64[2], case64[3])
    for name, got, ref in zip(("grad_value", "grad_loc", "grad_aw"), g32, g64):
        want = ref.float().cpu().numpy()
        err = np.abs(got.cpu().numpy() - want).max() / max(1.0, np.abs(want).max())
        print("case 6, %s: float32 kernels vs float64 kernels %.3e" % (name, err))
        assert err <= 1e-4, (name, err)


# ------------------------------------------------------------------------------------------------------------ 7. module level
MODULE_SEED = 3


def test_double_module_on_the_device_against_the_host_composition():
    from dualfusion.msda import MSDeformAttn
    maps = SCRIPT_DIMS["maps"]
    S, Lq, L = sum(h * w for h, w in maps), 5, len(maps)
    torch.manual_seed(MODULE_SEED)
    host = MSDeformAttn(d_model=32, n_levels=2, n_heads=4, n_points=2).double()
    with torch.no_grad():                                              # (after _reset_parameters, which zeroes these two)
        host.sampling_offsets.weight.copy_(torch.randn_like(host.sampling_offsets.weight) * 0.3)
        host.attention_weights.weight.copy_(torch.randn_like(host.attention_weights.weight) * 0.5)
    query = torch.randn(1, Lq, 32, dtype=torch.float64)
    ref_pts = torch.rand(1, Lq, L, 2, dtype=torch.float64)
    feat = torch.randn(1, S, 32, dtype=torch.float64)
    gout = torch.randn(1, Lq, 32, dtype=torch.float64)
    shapes_h = torch.as_tensor(maps, dtype=torch.long)
    start_h = torch.as_tensor(_starts(maps), dtype=torch.long)
    # the seed keeps every sampling location the module produces >= 1e-3 px from a pixel line
    with torch.no_grad():
        offsets = host.sampling_offsets(query).view(1, Lq, 4, L, 2, 2)
        pix = host._locations(ref_pts, offsets, shapes_h) * shapes_h.flip(-1)[None, None, None, :, None, :].double() - 0.5
    assert float((pix - pix.round()).abs().min()) >= 1e-3

    def run(module, dev):
        q = query.to(dev).requires_grad_(True)
        out = module(q, ref_pts.to(dev), feat.to(dev), shapes_h.to(dev), start_h.to(dev))
        out.backward(gout.to(dev))
        grads = {name: p.grad for name, p in module.named_parameters()}
        assert all(g is not None for g in grads.values())
        return dict(grads, out=out.detach(), query=q.grad)

    device = copy.deepcopy(host).to(_dev())
    got = run(device, _dev())
    with fr.patched():
        want = run(host, torch.device("cpu"))
    assert set(got) == set(want) and len(got) == 10
    worst = 0.0
    for name in sorted(want):
        assert got[name].dtype == torch.float64, name
        e = _err(got[name], want[name])
        worst = max(worst, e)
        assert e <= BOUND, (name, e)
    print("case 7, module: worst of output, query and parameter gradients %.3e" % worst)


# --------------------------------------------------------------------------------------------------------------- 8. refusals
def test_mixed_and_half_dtypes_are_refused():
    from dualfusion import ops
    from dualfusion._lib import Df3dError
    d = SCRIPT_DIMS
    value, loc, aw, gout = (t.to(_dev()) for t in _case(3, d["N"], d["M"], 4, d["Lq"], d["P"], d["maps"]))
    shapes, lstart = _level_tensors(d["maps"])
    with pytest.raises(Df3dError) as e:
        ops.ms_deform_attn_forward(value, shapes, lstart, loc.float(), aw)
    assert "float64" in str(e.value) and "float32" in str(e.value)
    with pytest.raises(Df3dError) as e:
        ops.ms_deform_attn_backward(value, shapes, lstart, loc.float(), aw, gout)
    assert "float64" in str(e.value) and "float32" in str(e.value)
    with pytest.raises(Df3dError):
        ops.ms_deform_attn_forward(value.half(), shapes, lstart, loc.half(), aw.half())
    with pytest.raises(Df3dError):
        ops.ms_deform_attn_forward(value.bfloat16(), shapes, lstart, loc.bfloat16(), aw.bfloat16())
    with pytest.raises(Df3dError) as e:
        ops.ms_deform_attn_backward(value.float(), shapes, lstart, loc.float(), aw.float(), gout)
    assert "float64" in str(e.value) and "float32" in str(e.value)


def test_float64_ignores_the_backward_switch(monkeypatch):
    """DF3D_MSDA_BWD and torch.use_deterministic_algorithms select among the float32 kernels only: the float64 path is one
    path, never 'not served', and the same bits under every setting."""
    from dualfusion import ops
    d = ANALYTIC_DIMS
    v, l, a, g = (t.to(_dev()) for t in _case(130, d["N"], d["M"], 30, d["Lq"], d["P"], d["maps"]))
    shapes, lstart = _level_tensors(d["maps"])
    monkeypatch.delenv("DF3D_MSDA_BWD", raising=False)
    base = ops.ms_deform_attn_backward(v, shapes, lstart, l, a, g)
    for mode in ("atomic", "sorted", "binned", "no-such-mode"):
        monkeypatch.setenv("DF3D_MSDA_BWD", mode)
        for x, y in zip(base, ops.ms_deform_attn_backward(v, shapes, lstart, l, a, g)):
            assert torch.equal(x, y), mode


def test_empty_batch_and_empty_query_list():
    """Empty tensors have null data pointers: N = 0 returns empty results, Lq = 0 a zero grad_value (no point touches a row)."""
    from dualfusion import ops
    maps = SCRIPT_DIMS["maps"]
    shapes, lstart = _level_tensors(maps)
    f64 = dict(dtype=torch.float64, device=_dev())
    value = torch.randn(2, 30, 2, 4, **f64)
    loc, aw, gout = torch.empty(2, 0, 2, 2, 2, 2, **f64), torch.empty(2, 0, 2, 2, 2, **f64), torch.empty(2, 0, 8, **f64)
    assert tuple(ops.ms_deform_attn_forward(value, shapes, lstart, loc, aw).shape) == (2, 0, 8)
    gv, gl, ga = ops.ms_deform_attn_backward(value, shapes, lstart, loc, aw, gout)
    assert torch.equal(gv, torch.zeros_like(value)) and gl.numel() == 0 and ga.numel() == 0
    none = [torch.empty((0,) + tuple(t.shape[1:]), **f64) for t in (value, torch.empty(2, 3, 2, 2, 2, 2), torch.empty(2, 3, 2, 2, 2),
                                                                    torch.empty(2, 3, 8))]
    assert tuple(ops.ms_deform_attn_forward(none[0], shapes, lstart, none[1], none[2]).shape) == (0, 3, 8)
    assert all(g.numel() == 0 for g in ops.ms_deform_attn_backward(none[0], shapes, lstart, none[1], none[2], none[3]))
