"""Dynamic scatter on the device (csrc/dynscatter.hip) against the host reference tests/dynscatter_reference.py.

Every forward case compares voxel_coors, point2voxel_map and voxel_points_count with array_equal.  Per (voxel, channel),
with n the voxel's point count, S = sum |x_i| in float64 and u = 2^-24 (float32) or 2^-53 (float64):
    max   equal;
    sum   |error| <= n u S;
    mean  |error| <= (n + 1) u S / n
-- the textbook bounds of a sum in ANY order plus one rounding of the quotient (a float32 sum in sequential, permuted and
pairwise order reaches at most 0.47 of it for n = 1 .. 5000; an indexing error exceeds it by orders of magnitude).  Where a
float64 result is judged the reference accumulates in np.longdouble, so its own rounding does not eat into the bound.
Backward results are exact: a copy, or one division in the operator's type.  Features are uniform in +-50 unless said.

DynamicVFE has no closed-form bound through Linear + BatchNorm: the yardstick is the same composition in plain float32 torch
on the CPU against float64; the device may deviate at most 4x that, per tensor, as max error over max magnitude (the margin
tests/test_gpu_tftrain.py uses for a float32 formulation against float64).  Measured ("Dynamic scatter"):
yardstick and device values are printed by the test."""
import functools

import numpy as np
import pytest

import dynscatter_reference as ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

U = {np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}
REDUCES = ["sum", "mean", "max"]


def _dev():
    return torch.device("cuda:0")


def _to(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _check_forward(feats, coors, reduce_type):
    """runs the operator on (feats, coors) and holds it to the module docstring's bounds; -> (voxel_feats, plan)"""
    from dualfusion import ops
    dt = feats.dtype.type
    plan = ops.dynamic_scatter_plan(_to(coors))
    vf, vc = ops.dynamic_scatter(_to(feats), plan, reduce_type)
    acc = np.longdouble if dt is np.float64 else np.float64
    want, wc, wmap, wcnt = ref.reduce(feats, coors, reduce_type, acc=acc)
    assert vc.dtype == torch.int32 and np.array_equal(vc.cpu().numpy(), wc)
    assert np.array_equal(plan.point2voxel_map.cpu().numpy(), wmap)
    assert np.array_equal(plan.voxel_points_count.cpu().numpy(), wcnt)
    got = vf.cpu().numpy()
    assert got.dtype == feats.dtype and got.shape == want.shape
    if reduce_type == "max":
        assert np.array_equal(got, want.astype(dt))
        return vf, plan
    n = wcnt[:, None].astype(np.float64)
    S = ref.abs_sums(feats, wmap, len(wc))
    bound = n * U[dt] * S if reduce_type == "sum" else (n + 1) * U[dt] * S / n
    err = np.abs(got.astype(acc) - want).astype(np.float64)
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print("%s %s N=%d C=%d M=%d: max error / bound = %.3f" % (reduce_type, dt.__name__, len(feats), feats.shape[1], len(wc), worst))
    assert (err <= bound).all(), worst
    return vf, plan


@functools.lru_cache(maxsize=None)
def _reference_case(dtype):
    """the reference's own test scaled down: coordinates randint(-1, 20), rows with a negative entry set to -1"""
    rs = np.random.RandomState(0)
    coors = rs.randint(-1, 20, (20000, 3)).astype(np.int32)
    coors[(coors < 0).any(1)] = -1
    return rs.uniform(-50, 50, (20000, 3)).astype(dtype), coors


@functools.lru_cache(maxsize=None)
def _long_case(dtype):
    rs = np.random.RandomState(1)
    return rs.uniform(-50, 50, (12000, 5)).astype(dtype), rs.randint(0, 2, (12000, 3)).astype(np.int32)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("reduce_type", REDUCES)
def test_reference_case(reduce_type, dtype):
    feats, coors = _reference_case(dtype)
    _check_forward(feats, coors, reduce_type)


@pytest.mark.parametrize("reduce_type", REDUCES)
def test_rows_with_any_negative_entry_are_invalid(reduce_type):
    rs = np.random.RandomState(2)
    coors = rs.randint(0, 6, (300, 3)).astype(np.int32)
    coors[17] = (3, -7, 2)
    coors[101] = (-1, 5, 5)
    coors[299] = (5, 5, -2)
    feats = rs.uniform(-50, 50, (300, 4)).astype(np.float32)
    _, plan = _check_forward(feats, coors, reduce_type)
    p2v = plan.point2voxel_map.cpu().numpy()
    assert p2v[17] == -1 and p2v[101] == -1 and p2v[299] == -1 and (p2v >= 0).sum() == 297


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("reduce_type", REDUCES)
def test_long_segments_2x2x2(reduce_type, dtype):
    """~1500 points per voxel: more than a wave and more than a 1024-element sort tile"""
    feats, coors = _long_case(dtype)
    _check_forward(feats, coors, reduce_type)


@pytest.mark.parametrize("channels", [5, 64])
@pytest.mark.parametrize("reduce_type", REDUCES)
def test_single_voxel_of_3000_points(reduce_type, channels):
    rs = np.random.RandomState(5)
    feats = rs.uniform(-50, 50, (3000, channels)).astype(np.float32)
    _, plan = _check_forward(feats, np.full((3000, 3), 7, np.int32), reduce_type)
    assert plan.num_voxels == 1 and np.array_equal(plan.point_ids.cpu().numpy(), np.arange(3000))


@pytest.mark.parametrize("counts", [(64, 66), (63, 67), (65, 65)])
@pytest.mark.parametrize("reduce_type", REDUCES)
def test_counts_straddling_64(reduce_type, counts):
    rs = np.random.RandomState(6)
    coors = np.repeat(np.arange(2, dtype=np.int32), counts)[rs.permutation(130)].reshape(130, 1)
    coors = np.concatenate([coors, coors * 0 + 3], 1)
    feats = rs.uniform(-50, 50, (130, 5)).astype(np.float32)
    _, plan = _check_forward(feats, coors, reduce_type)
    assert tuple(plan.voxel_points_count.tolist()) == counts


@pytest.mark.parametrize("channels", [1, 3, 4, 5, 10, 64, 67, 128])
def test_row_widths(channels):
    """N = 2000; half of the points fall on a 3 x 3 grid (~110 per voxel: the block path), half on 30 x 30 (the wave path)"""
    rs = np.random.RandomState(7)
    coors = np.concatenate([rs.randint(0, 3, (1000, 2)), rs.randint(3, 33, (1000, 2))]).astype(np.int32)[rs.permutation(2000)]
    feats = rs.uniform(-50, 50, (2000, channels)).astype(np.float32)
    for reduce_type in REDUCES:
        _check_forward(feats, coors, reduce_type)


@pytest.mark.parametrize("ndim", [1, 2])
def test_narrow_coordinates(ndim):
    rs = np.random.RandomState(8)
    coors = rs.randint(-1, 25, (1500, ndim)).astype(np.int32)
    feats = rs.uniform(-50, 50, (1500, 3)).astype(np.float32)
    for reduce_type in REDUCES:
        _check_forward(feats, coors, reduce_type)


@pytest.mark.parametrize("average", [True, False])
def test_batched_form_equals_the_per_sample_loop(average):
    """4-column (b, z, y, x) coordinates, batch ids 0..3 sorted: ONE native call against the per-sample loop"""
    from dualfusion.voxel import DynamicScatter
    rs = np.random.RandomState(9)
    coors = np.concatenate([np.sort(rs.randint(0, 4, (4000, 1)), 0), rs.randint(-1, 9, (4000, 3))], 1).astype(np.int32)
    assert coors[-1, 0] == 3 and coors[0, 0] == 0
    feats = rs.uniform(-50, 50, (4000, 4)).astype(np.float32)
    reduce_type = "mean" if average else "max"
    _check_forward(feats, coors, reduce_type)
    want, wc = ref.batched_loop(feats, coors, reduce_type)
    scatter = DynamicScatter([0.2, 0.2, 4], [0, -40, -3, 70.4, 40, 1], average)
    vf, vc = scatter(_to(feats), _to(coors))
    assert np.array_equal(vc.cpu().numpy(), wc)
    cnt = ref.plan(coors)[2][:, None].astype(np.float64)
    bound = (cnt + 1) * U[np.float32] * ref.abs_sums(feats, ref.plan(coors)[1], len(wc)) / cnt if average else 0.0
    assert (np.abs(vf.cpu().numpy().astype(np.float64) - want) <= bound).all()


def test_wide_coordinates():
    rs = np.random.RandomState(10)
    coors = np.stack([rs.randint(0, 8, 3000), rs.randint(0, 41, 3000), rs.randint(0, 1440, 3000), rs.randint(0, 1440, 3000)], 1)
    coors[0] = (7, 40, 1439, 1439)
    coors[1::2, 1:] = coors[0::2, 1:]                  # (so that voxels do hold several points)
    coors[1::2, 0] = coors[0::2, 0]
    feats = rs.uniform(-50, 50, (3000, 4)).astype(np.float32)
    for reduce_type in REDUCES:
        _check_forward(feats, coors.astype(np.int32), reduce_type)


def test_keys_beyond_32_bits_and_the_63_bit_limit():
    from dualfusion import _lib, ops
    rs = np.random.RandomState(11)
    coors = np.array([0, 1, 2000000, 2000001], np.int32)[rs.randint(0, 4, (500, 3))]
    coors[0] = (2000001, 2000001, 2000001)             # key = 2000002^3 - 1 > 2^62
    feats = rs.uniform(-50, 50, (500, 3)).astype(np.float32)
    for reduce_type in REDUCES:
        _, plan = _check_forward(feats, coors, reduce_type)
    assert plan.num_voxels == len(np.unique(coors, axis=0)) > 32
    with pytest.raises(_lib.Df3dError, match="63 bits"):
        ops.dynamic_scatter_plan(_to(np.array([[3000000] * 3, [0, 0, 0]], np.int32)))


@pytest.mark.parametrize("n", [0, 10])
def test_empty_inputs(n):
    from dualfusion import ops
    coors = torch.full((n, 3), -1, dtype=torch.int32, device=_dev())
    if n:
        coors[3] = torch.tensor([4, -1, 2], dtype=torch.int32)
    feats = torch.ones((n, 4), device=_dev(), requires_grad=True)
    for reduce_type in REDUCES:
        vf, vc = ops.dynamic_scatter(feats, coors, reduce_type)
        assert tuple(vf.shape) == (0, 4) and tuple(vc.shape) == (0, 3)
        vf.sum().backward()
        assert torch.equal(feats.grad, torch.zeros_like(feats))
    plan = ops.dynamic_scatter_plan(coors)
    assert tuple(plan.point2voxel_map.shape) == (n,) and bool((plan.point2voxel_map == -1).all())
    assert tuple(plan.voxel_points_count.shape) == (0,) and plan.num_voxels == 0
    assert tuple(ops.voxel_to_point(torch.zeros((0, 4), device=_dev()), plan).shape) == (n, 4)


@pytest.mark.parametrize("reduce_type", REDUCES)
def test_backward_with_ties_is_exact(reduce_type):
    """integer features 0..3: almost every maximum is tied, the gradient goes to the lowest tied point index"""
    from dualfusion import ops
    rs = np.random.RandomState(12)
    coors = rs.randint(-1, 4, (2000, 3)).astype(np.int32)
    feats = rs.randint(0, 4, (2000, 4)).astype(np.float32)
    x = _to(feats).requires_grad_(True)
    vf, vc = ops.dynamic_scatter(x, _to(coors), reduce_type)
    g = rs.uniform(-50, 50, tuple(vf.shape)).astype(np.float32)
    vf.backward(_to(g))
    want = ref.reduce_backward(g, feats, coors, reduce_type, dtype=np.float32)
    assert np.array_equal(x.grad.cpu().numpy(), want)


def _distinct_features(rs, n, c, dtype):
    """all values at least 0.25 apart (no maximum flips inside a finite-difference step), spread over +-50"""
    vals = (rs.permutation(n * c).astype(np.float64) - n * c / 2) * min(0.25, 100.0 / (n * c))
    return torch.from_numpy(vals.reshape(n, c)).to(dtype)


@pytest.mark.parametrize("reduce_type", REDUCES)
def test_gradcheck_float64(reduce_type):
    from dualfusion import ops
    rs = np.random.RandomState(13)
    plan = ops.dynamic_scatter_plan(_to(rs.randint(-1, 3, (100, 3)).astype(np.int32)))
    feats = _distinct_features(rs, 100, 4, torch.float64).to(_dev()).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda f: ops.dynamic_scatter(f, plan, reduce_type)[0], (feats,))


def test_gradcheck_voxel_to_point_float64():
    from dualfusion import ops
    rs = np.random.RandomState(14)
    plan = ops.dynamic_scatter_plan(_to(rs.randint(-1, 3, (100, 3)).astype(np.int32)))
    vf = torch.from_numpy(rs.standard_normal((plan.num_voxels, 4))).to(_dev()).requires_grad_(True)
    out = ops.voxel_to_point(vf, plan)
    p2v = plan.point2voxel_map.long()
    assert torch.equal(out[p2v >= 0], vf[p2v[p2v >= 0]]) and bool((out[p2v < 0] == 0).all()) and bool((p2v < 0).any())
    assert torch.autograd.gradcheck(lambda v: ops.voxel_to_point(v, plan), (vf,))


@pytest.mark.parametrize("average", [True, False])
def test_gradcheck_float32_as_the_reference_calls_it(average):
    from dualfusion.voxel import DynamicScatter
    rs = np.random.RandomState(15)
    coors = _to(rs.randint(-1, 3, (100, 3)).astype(np.int32))
    feats = _distinct_features(rs, 100, 4, torch.float32).to(_dev()).requires_grad_(True)
    scatter = DynamicScatter([0.1, 0.1, 0.1], [-0.5, -0.5, -0.5, 0.5, 0.5, 0.5], average)
    assert torch.autograd.gradcheck(lambda f: scatter(f, coors)[0], (feats,), eps=1e-2, atol=1e-2, rtol=1e-5)


def test_results_repeat_bit_for_bit():
    from dualfusion import ops
    feats, coors = _long_case(np.float32)
    f, c = _to(feats), _to(coors)
    a, _ = ops.dynamic_scatter(f, c, "mean")
    b, _ = ops.dynamic_scatter(f, c, "mean")
    assert torch.equal(a, b)
    plan = ops.dynamic_scatter_plan(c)
    g = _to(np.random.RandomState(16).uniform(-50, 50, (12000, 5)).astype(np.float32))
    grads = []
    for _ in range(2):
        vf = torch.zeros((plan.num_voxels, 5), device=_dev(), requires_grad=True)
        ops.voxel_to_point(vf, plan).backward(g)
        grads.append(vf.grad)
    assert torch.equal(grads[0], grads[1])
    want = ref.reduce(g.cpu().numpy(), coors, "sum")[0]
    n = plan.voxel_points_count.cpu().numpy()[:, None].astype(np.float64)
    bound = n * U[np.float32] * ref.abs_sums(g.cpu().numpy(), plan.point2voxel_map.cpu().numpy(), plan.num_voxels)
    assert (np.abs(grads[0].cpu().numpy().astype(np.float64) - want) <= bound).all()


@pytest.mark.parametrize("reduce_type", REDUCES)
def test_extension_shim_agrees_with_the_op(reduce_type):
    from dualfusion import ext, ops
    vl = ext.load("voxel_layer")
    rs = np.random.RandomState(17)
    coors = _to(rs.randint(-1, 5, (1000, 3)).astype(np.int32))
    feats = _to(rs.randint(0, 6, (1000, 4)).astype(np.float32))
    vf, vc, p2v, cnt = vl.dynamic_point_to_voxel_forward(feats, coors, reduce_type)
    x = feats.clone().requires_grad_(True)
    of, oc = ops.dynamic_scatter(x, coors, reduce_type)
    assert torch.equal(vf, of) and torch.equal(vc, oc)
    assert p2v.shape == (1000,) and cnt.shape == (vc.shape[0],) and int(cnt.sum()) == int((p2v >= 0).sum())
    g = _to(rs.uniform(-1, 1, tuple(vf.shape)).astype(np.float32))
    grad_feats = torch.full_like(feats, 7.0)                      # caller-allocated, fully overwritten
    assert vl.dynamic_point_to_voxel_backward(grad_feats, g, feats, vf, p2v, cnt, reduce_type) is None
    of.backward(g)
    assert torch.equal(grad_feats, x.grad)
    with pytest.raises(RuntimeError):
        vl.dynamic_point_to_voxel_forward(feats, coors, "median")


def test_dynamic_simple_vfe_on_dynamic_voxelisation():
    from dualfusion import ops, synth
    from dualfusion.voxel import DynamicSimpleVFE, Voxelization
    pts = synth.nusc_sweep(seed=3)[:6000].astype(np.float32)
    pts[:40, 0] += 200.0                                             # some points outside the grid
    dev_pts = _to(pts)
    coors = Voxelization(synth.NUSC_VOXEL, synth.NUSC_RANGE, -1)(dev_pts)
    assert coors.dtype == torch.int32 and tuple(coors.shape) == (6000, 3) and bool((coors[:40] == -1).all())
    x = dev_pts.clone().requires_grad_(True)
    mean, vc = DynamicSimpleVFE(synth.NUSC_VOXEL, synth.NUSC_RANGE)(x, coors)
    assert not mean.requires_grad
    want, wc, wmap, wcnt = ref.reduce(pts, coors.cpu().numpy(), "mean")
    assert np.array_equal(vc.cpu().numpy(), wc)
    n = wcnt[:, None].astype(np.float64)
    bound = (n + 1) * U[np.float32] * ref.abs_sums(pts, wmap, len(wc)) / n
    assert (np.abs(mean.cpu().numpy().astype(np.float64) - want) <= bound).all()
    # the same voxel set as the hard voxeliser with caps that drop nothing
    _, hc, hn, _ = ops.hard_voxelize(dev_pts, synth.NUSC_VOXEL, synth.NUSC_RANGE, 64, 6000)
    hc, hn = hc.cpu().numpy(), hn.cpu().numpy()
    order = np.lexsort(hc.T[::-1])
    assert hn.max() < 64 and np.array_equal(hc[order], wc) and np.array_equal(hn[order], wcnt)


VFE_VOXEL, VFE_RANGE = (0.8, 0.8, 2.0), (0.0, -4.0, -2.0, 8.0, 4.0, 2.0)


def _rel(a, b):
    return float((a.double() - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("mode", ["max", "avg"])
def test_dynamic_vfe_against_the_float64_composition(mode):
    from dualfusion.voxel import DynamicVFE, Voxelization
    rs = np.random.RandomState(18)
    clouds = [np.concatenate([rs.uniform((-0.3, -4.2, -2.1), (8.3, 4.2, 2.1), (n, 3)), rs.uniform(0, 1, (n, 1))], 1)
              .astype(np.float32) for n in (1400, 1600)]
    layer = Voxelization(VFE_VOXEL, VFE_RANGE, -1)
    coors = torch.cat([torch.nn.functional.pad(layer(_to(c)), (1, 0), value=b) for b, c in enumerate(clouds)])
    assert coors.dtype == torch.int32 and bool((coors[:, 1:] < 0).any())
    pts = np.concatenate(clouds)
    torch.manual_seed(19)
    model = DynamicVFE(in_channels=4, feat_channels=[16, 32], with_cluster_center=True, with_voxel_center=True,
                       voxel_size=VFE_VOXEL, point_cloud_range=VFE_RANGE, mode=mode).train()
    with torch.no_grad():
        for layer_ in model.vfe_layers:                               # (a norm at its initial 1 / 0 hides two gradients)
            layer_[1].weight.uniform_(0.5, 1.5)
            layer_[1].bias.uniform_(-0.5, 0.5)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    results = {}
    for name, dtype in (("f64", torch.float64), ("f32", torch.float32)):
        m = ref.DynamicVFERef(4, [16, 32], VFE_VOXEL, VFE_RANGE, mode, dtype=dtype).train()
        m.load_state_dict({k: (v.to(dtype) if v.is_floating_point() else v) for k, v in state.items()})
        x = torch.from_numpy(pts).to(dtype).requires_grad_(True)
        out, oc = m(x, coors.cpu())
        if name == "f64":
            w = torch.from_numpy(np.random.RandomState(20).standard_normal(tuple(out.shape)))
        (out * w.to(dtype)).sum().backward()
        results[name] = [("out", out.detach()), ("grad features", x.grad)] + \
            [("grad " + k, p.grad) for k, p in m.named_parameters()]
    model = model.to(_dev())
    x = _to(pts).requires_grad_(True)
    out, vc = model(x, coors)
    assert np.array_equal(vc.cpu().numpy(), oc.numpy()) and tuple(out.shape) == (len(oc), 32)
    (out * w.float().to(_dev())).sum().backward()
    device = [("out", out.detach()), ("grad features", x.grad)] + [("grad " + k, p.grad) for k, p in model.named_parameters()]
    assert [k for k, _ in device] == [k for k, _ in results["f64"]]
    failures = []
    for (k, want), (_, yard), (_, got) in zip(results["f64"], results["f32"], device):
        y, d = _rel(yard, want), _rel(got.cpu(), want)
        print("DynamicVFE %s %-32s float32 yardstick %.3e  device %.3e" % (mode, k, y, d))
        if not d <= 4 * y:
            failures.append((k, y, d))
    assert not failures, failures
    # return_point_feats hands back the last layer's point rows
    model.return_point_feats = True
    assert tuple(model(x.detach(), coors).shape) == (3000, 32)
