"""RoI grid pooling on the device (csrc/roipool.hip) against the host references of tests/roipool_reference.py.

Query: indices and the empty mask are compared EXACTLY; the fixture has no candidate within 8 ulp of radius^2 (asserted),
so the comparison never rests on a rounding mode, and one hand-made case has dist2 == radius^2 exactly.
Grouping: the forward is a copy (exact); the backward is a float32 sum of n terms in some order: |error| <= n 2^-24 sum|g|
per element (the bound tests/test_gpu_dynscatter.py uses), bit-identical from run to run.
Everything through Linear / BatchNorm layers has no closed-form bound: the yardstick is the same composition in plain
float32 torch on the CPU against float64, fed the reference's indices; the device may deviate at most 4x that, per tensor,
as max error over max magnitude (tests/test_gpu_dynscatter.py, tests/test_gpu_tftrain.py).  Both values are printed."""
import copy
import functools

import numpy as np
import pytest

import roipool_reference as ref

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
U32 = 2.0 ** -24


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def fixture(seed, sort_rows=False):
    fx = ref.base_fixture(seed, sort_rows=sort_rows)
    fx["ref"] = [ref.voxel_query(fx["table"], fx["xyz"], fx["new_xyz"], fx["new_coords"], *s) for s in ref.SETTINGS]
    return fx


def directory(indices, batch, shape):
    from dualfusion import ops
    return ops.grid_build(dev(indices), batch, list(shape))


def both_queries(indices, batch, shape, xyz, new_xyz, new_coords, rng, radius, nsample):
    """raw idx of the directory and the dense entry point"""
    from dualfusion import ops
    args = (rng, radius, nsample, dev(xyz), dev(new_xyz), dev(new_coords))
    a = ops.voxel_query(*args, directory(indices, batch, shape))
    b = ops.voxel_query(*args, dev(ref.dense_table(indices, batch, shape)))
    return a.cpu().numpy(), b.cpu().numpy()


# ---------------------------------------------------------------------------------------------------- query
@pytest.mark.parametrize("seed,sort_rows", [(0, False), (1, False), (2, False), (0, True)])
def test_query_equals_the_triple_loop(seed, sort_rows):
    from dualfusion import ops
    from dualfusion import pointnet2_stack as ps
    fx = fixture(seed, sort_rows)
    for (rng, radius, nsample), (want, found) in zip(ref.SETTINGS, fx["ref"]):
        assert ref.near_boundary(fx["table"], fx["xyz"], fx["new_xyz"], fx["new_coords"], rng, radius) == 0
        a, b = both_queries(fx["indices"], fx["batch"], fx["shape"], fx["xyz"], fx["new_xyz"], fx["new_coords"], rng, radius,
                            nsample)
        assert np.array_equal(a, want), (rng, np.nonzero((a != want).any(1))[0][:5])
        assert np.array_equal(b, want), (rng, np.nonzero((b != want).any(1))[0][:5])
    # rows already in flat order: the directory needs no permutation
    if sort_rows:
        g = ops.grid_build(dev(fx["indices"]), fx["batch"], list(fx["shape"]), rows_sorted=True)
        assert g.perm is None
        rng, radius, nsample = ref.SETTINGS[1]
        a = ops.voxel_query(rng, radius, nsample, dev(fx["xyz"]), dev(fx["new_xyz"]), dev(fx["new_coords"]), g)
        assert np.array_equal(a.cpu().numpy(), fx["ref"][1][0])
    # the reference's wrapper: empty rows zeroed, and the mask
    rng, radius, nsample = ref.SETTINGS[1]
    want, found = fx["ref"][1]
    idx, empty = ps.voxel_query(rng, radius, nsample, dev(fx["xyz"]), dev(fx["new_xyz"]), dev(fx["new_coords"]),
                                directory(fx["indices"], fx["batch"], fx["shape"]))
    assert np.array_equal(empty.cpu().numpy(), found == 0) and empty.dtype == torch.bool
    assert np.array_equal(idx.cpu().numpy(), np.where((found == 0)[:, None], 0, want))
    assert (found > nsample).sum() >= 10 and (found == 0).sum() >= 40


def test_query_accepts_a_neighbour_exactly_on_the_sphere():
    # voxel (z, y, x) = (2, 12, 2): centre x = -1 + 2.5 * 0.4 = 0.0; the query centre is displaced by 0.5 along x, radius 0.5
    indices = np.asarray([[0, 2, 12, 2], [0, 2, 12, 4]], dtype=np.int32)
    xyz = ref.cell_centers(indices)
    assert xyz[0, 0] == 0.0
    new_xyz = xyz[:1].copy()
    new_xyz[0, 0] = np.float32(0.5)
    new_coords = ref.coords_of(new_xyz, [0])
    assert list(new_coords[0]) == [0, 2, 12, 3]
    assert ref.dist2_f32(xyz[0], new_xyz[0]) == np.float32(0.25) == np.float32(0.5) * np.float32(0.5)
    want, found = ref.voxel_query(ref.dense_table(indices, 1, ref.GRID), xyz, new_xyz, new_coords, (1, 1, 1), 0.5, 4)
    assert found[0] == 2 and list(want[0]) == [0, 1, 0, 0]          # 0.3 away on the other side, and the one ON the sphere
    a, b = both_queries(indices, 1, ref.GRID, xyz, new_xyz, new_coords, (1, 1, 1), 0.5, 4)
    assert np.array_equal(a, want) and np.array_equal(b, want)


def test_query_from_centres_outside_every_face():
    Z, Y, X = ref.GRID
    zz, yy, xx = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    indices = np.stack([np.zeros(Z * Y * X, dtype=np.int64), zz.ravel(), yy.ravel(), xx.ravel()], 1).astype(np.int32)
    indices = indices[np.random.RandomState(5).permutation(len(indices))]
    xyz = ref.cell_centers(indices)
    cells = np.asarray([[-1, 10, 9], [Z, 10, 9], [2, -1, 9], [2, Y, 9], [2, 10, -1], [2, 10, X], [-1, -1, -1], [Z, Y, X],
                        [-4, 10, 9], [2, 10, X + 3]], dtype=np.int32)
    new_coords = np.ascontiguousarray(np.concatenate([np.zeros((len(cells), 1), dtype=np.int32), cells], 1))
    new_xyz = ref.cell_centers(new_coords)
    table = ref.dense_table(indices, 1, ref.GRID)
    for rng, radius, nsample in (((1, 1, 1), 0.75, 8), ((2, 3, 2), 0.9, 16)):
        want, found = ref.voxel_query(table, xyz, new_xyz, new_coords, rng, radius, nsample)
        assert (found[:6] > 0).all()                                  # a centre outside still finds in-range neighbours
        assert ref.near_boundary(table, xyz, new_xyz, new_coords, rng, radius) == 0
        a, b = both_queries(indices, 1, ref.GRID, xyz, new_xyz, new_coords, rng, radius, nsample)
        assert np.array_equal(a, want) and np.array_equal(b, want)
    assert want[8, 0] == -1 and want[9, 0] == -1                      # too far outside for either range to reach


def test_query_keeps_frames_apart():
    fx = fixture(0)
    n0 = int(fx["xyz_cnt"][0])
    one = fx["indices"][:n0]
    two = one.copy()
    two[:, 0] = 1
    indices = np.ascontiguousarray(np.concatenate([one, two[::-1]]))   # the same cells in both frames, other row order
    xyz = ref.cell_centers(indices)
    new_coords = fx["new_coords"].copy()
    new_coords[:, 0] = 1
    rng, radius, nsample = ref.SETTINGS[1]
    want, found = ref.voxel_query(ref.dense_table(indices, 2, ref.GRID), xyz, fx["new_xyz"], new_coords, rng, radius, nsample)
    a, b = both_queries(indices, 2, ref.GRID, xyz, fx["new_xyz"], new_coords, rng, radius, nsample)
    assert np.array_equal(a, want) and np.array_equal(b, want)
    hit = a[:, 0] >= 0
    assert hit.sum() > 20 and (a[hit] >= n0).all()


def test_refusals_name_the_limit():
    from dualfusion import _lib, ops
    fx = fixture(0)
    g = directory(fx["indices"], fx["batch"], fx["shape"])
    args = (dev(fx["xyz"]), dev(fx["new_xyz"]), dev(fx["new_coords"]))
    with pytest.raises(_lib.Df3dError, match="above the limit of 15"):
        ops.voxel_query((1, 1, 16), 0.5, 4, *args, g)
    with pytest.raises(_lib.Df3dError, match="use the composed path"):
        ops.voxel_pool_fused(torch.zeros(len(fx["xyz"]), 32, device="cuda"), args[0], g, args[1], args[2], (1, 1, 1), 0.5, 17,
                             torch.zeros(32, 4, device="cuda"))


# ---------------------------------------------------------------------------------------------------- grouping
@pytest.mark.parametrize("C", [5, 32])
@pytest.mark.parametrize("hot", [False, True])
def test_grouping_forward_is_a_copy_and_backward_an_ordered_sum(C, hot):
    from dualfusion import ops
    fx = fixture(0)
    rs = np.random.RandomState(11 + C)
    feat_cnt = fx["xyz_cnt"]
    idx_cnt = np.asarray([40, 68], dtype=np.int32)
    N, ns = int(feat_cnt.sum()), 16
    idx = np.concatenate([rs.randint(0, feat_cnt[0], (40, ns)), rs.randint(0, feat_cnt[1], (68, ns))]).astype(np.int32)
    if hot:
        idx[40:, :] = 7                                               # one row of frame 1 referenced 68 * 16 = 1088 times
    features = rs.uniform(-50, 50, (N, C)).astype(np.float32)
    grad_out = rs.uniform(-50, 50, (108, C, ns)).astype(np.float32)
    f = dev(features).requires_grad_(True)
    out = ops.group_points_stack(f, dev(feat_cnt), dev(idx), dev(idx_cnt))
    assert np.array_equal(out.detach().cpu().numpy(), ref.group_points_stack(features, feat_cnt, idx, idx_cnt))
    out.backward(dev(grad_out))
    got = f.grad.cpu().numpy()
    again = ops.group_points_stack_backward(dev(grad_out), dev(idx), dev(idx_cnt), dev(feat_cnt), N).cpu().numpy()
    assert np.array_equal(got.view(np.int32), again.view(np.int32))   # the same bits on every run
    want, mag, refs = ref.group_points_stack_grad(grad_out, idx, idx_cnt, feat_cnt, N)
    assert (refs == 0).any() and (got[refs == 0] == 0).all()          # rows nobody refers to: exactly 0
    if hot:
        assert refs.max() == 1088 and refs[int(feat_cnt[0]) + 7] == 1088
    bound = refs[:, None] * U32 * mag
    err = np.abs(got.astype(np.float64) - want)
    print("grouping backward C=%d hot=%s: max error %.3e, bound there %.3e" % (C, hot, err.max(), bound.ravel()[err.argmax()]))
    assert (err <= bound).all()
    # the pybind-name shim writes into caller-allocated tensors
    from dualfusion import ext
    shim = ext.load("pointnet2_stack_cuda")
    o2 = torch.empty_like(out)
    shim.group_points_wrapper(2, 108, C, ns, dev(features), dev(feat_cnt), dev(idx), dev(idx_cnt), o2)
    assert torch.equal(o2, out.detach())
    g2 = torch.full((N, C), 3.0, device="cuda")
    shim.group_points_grad_wrapper(2, 108, C, N, ns, dev(grad_out), dev(idx), dev(idx_cnt), dev(feat_cnt), g2)
    assert np.array_equal(g2.cpu().numpy().view(np.int32), got.view(np.int32))


# ---------------------------------------------------------------------------------------------------- layers
def randomize_bn(module, seed):
    g = torch.Generator().manual_seed(seed)
    for m in module.modules():
        if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
            with torch.no_grad():
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.3)
                m.running_mean.copy_(torch.randn(m.bias.shape, generator=g) * 0.3)
                m.running_var.copy_(torch.rand(m.bias.shape, generator=g) * 1.5 + 0.5)


def numpy_state(module):
    return {k: v.detach().cpu().numpy() for k, v in module.state_dict().items()}


def compose(mod, k, features, xyz, new_xyz, raw_idx):
    """Scale k of NeighborVoxelSAModuleMSG.forward in plain torch on the CPU, in the dtype of `mod`, fed the reference's
    raw indices: the float64 reference of the gradients and, in float32, the yardstick.  Returns (out, pooled)."""
    dt = next(mod.parameters()).dtype
    empty = torch.from_numpy(raw_idx[:, 0] == -1)
    rows = torch.from_numpy(np.where((raw_idx[:, 0] == -1)[:, None], 0, raw_idx).astype(np.int64))
    keep = (~empty)[:, None, None].to(dt)
    feats_in = mod.mlps_in[k](features.to(dt).t().unsqueeze(0)).squeeze(0).t()                       # [N, C]
    grouped = feats_in[rows].permute(0, 2, 1) * keep                                                 # [M, C, ns]
    rel = (xyz.to(dt)[rows].permute(0, 2, 1) - new_xyz.to(dt).unsqueeze(-1)) * keep                  # [M, 3, ns]
    pos = mod.mlps_pos[k](rel.permute(1, 0, 2).unsqueeze(0))                                         # [1, C, M, ns]
    act = torch.relu(grouped.permute(1, 0, 2).unsqueeze(0) + pos)
    pooled = act.max(-1)[0] if mod.pool_method == "max_pool" else act.mean(-1)                      # [1, C, M]
    return mod.mlps_out[k](pooled).squeeze(0).t(), pooled.squeeze(0).t()


def rel_err(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


def judge(what, pairs):
    """pairs: (name, float64 reference, float32 yardstick, device); device error <= 4 x yardstick error, per tensor"""
    failures = []
    for name, want, yard, got in pairs:
        y, d = rel_err(yard, want), rel_err(got, want)
        print("%s %-40s float32 yardstick %.3e  device %.3e" % (what, name, y, d))
        if not d <= 4 * y:
            failures.append((name, y, d))
    assert not failures, failures


def sa_module(cin, specs, pool, seed, settings):
    from dualfusion.pointnet2_stack import NeighborVoxelSAModuleMSG
    torch.manual_seed(seed)
    mod = NeighborVoxelSAModuleMSG(query_ranges=[list(s[0]) for s in settings], radii=[s[1] for s in settings],
                                   nsamples=[s[2] for s in settings], mlps=[[cin] + list(s) for s in specs], pool_method=pool)
    randomize_bn(mod, seed)
    return mod


def module_inputs(fx, cin, seed):
    rs = np.random.RandomState(seed)
    features = rs.standard_normal((len(fx["xyz"]), cin)).astype(np.float32)
    coords_bxyz = np.ascontiguousarray(fx["new_coords"][:, [0, 3, 2, 1]])
    return features, coords_bxyz


@pytest.mark.parametrize("pool", ["max_pool", "avg_pool"])
@pytest.mark.parametrize("C", [16, 32, 64])
def test_fused_pool_against_float64(pool, C):
    from dualfusion import ops
    from dualfusion.pointnet2_stack import _bn_fold
    fx = fixture(1)
    cin = 8
    features, _ = module_inputs(fx, cin, 21)
    g = directory(fx["indices"], fx["batch"], fx["shape"])
    for si in (0, 1):                                               # nsample 4 (most balls overfull) and 16 (most padded)
        rng, radius, nsample = ref.SETTINGS[si]
        raw, found = fx["ref"][si]
        mod = sa_module(cin, [[C, 24]], pool, 30 + si, [ref.SETTINGS[si]]).eval()
        p = numpy_state(mod)
        want_out, want_pooled = ref.neighbor_sa_scale(p, 0, features, fx["xyz"], fx["new_xyz"], raw, pool)
        with torch.no_grad():
            yard_out, yard_pooled = compose(mod, 0, torch.from_numpy(features), torch.from_numpy(fx["xyz"]),
                                            torch.from_numpy(fx["new_xyz"]), raw)
            m = copy.deepcopy(mod).cuda()
            conv, bn = m.mlps_in[0]
            scale, shift = _bn_fold(bn)
            rows_in = torch.nn.functional.linear(dev(features), conv.weight[:, :, 0] * scale[:, None], shift).contiguous()
            conv, bn = m.mlps_pos[0]
            scale, shift = _bn_fold(bn)
            w_pos = torch.cat([conv.weight[:, :, 0, 0] * scale[:, None], shift[:, None]], 1).contiguous()
            pooled, idx, empty = ops.voxel_pool_fused(rows_in, dev(fx["xyz"]), g, dev(fx["new_xyz"]), dev(fx["new_coords"]),
                                                      rng, radius, nsample, w_pos, pool, want_idx=True)
            out = m(dev(fx["xyz"]), dev(fx["xyz_cnt"]), dev(fx["new_xyz"]), dev(fx["new_cnt"]),
                    dev(module_inputs(fx, cin, 21)[1]), dev(features), g)
        assert np.array_equal(idx.cpu().numpy(), raw) and np.array_equal(empty.cpu().numpy(), found == 0)
        pooled, out = pooled.cpu().numpy(), out.cpu().numpy()
        what = "fused %s C=%d nsample=%d" % (pool, C, nsample)
        judge(what, [("pooled", want_pooled, yard_pooled.numpy(), pooled), ("out", want_out, yard_out.numpy(), out)])
        # empty balls: features and relative coordinates are zeroed BEFORE the position branch: relu(shift_pos), not 0
        e = found == 0
        assert e.sum() >= 40
        assert np.array_equal(pooled[e], np.broadcast_to(np.maximum(w_pos[:, 3].cpu().numpy(), 0), pooled[e].shape))
        assert np.abs(pooled[e]).max() > 0
        # ... and through mlps_out: a float32 dot product of C terms, a scale and a shift: (C + 4) roundings of the magnitudes
        s_out, t_out = ref.bn_fold(p, "mlps_out.0.1")
        mag = np.abs(want_pooled[e]) @ np.abs(p["mlps_out.0.0.weight"][:, :, 0].astype(np.float64).T * s_out) + np.abs(t_out)
        assert (np.abs(out[e] - want_out[e]) <= (C + 4) * U32 * mag).all()
        assert (out[e] == out[e][:1]).all()
        # slots past the hit count repeat the first hit: it counts nsample - cnt + 1 times in the mean
        part = (found > 0) & (found < nsample)
        assert part.sum() >= 5
        judge(what, [("pooled, partly filled balls", want_pooled[part], yard_pooled.numpy()[part], pooled[part])])


def test_module_fused_composed_and_dense_agree_with_float64(monkeypatch):
    fx = fixture(2)
    cin = 8
    features, coords = module_inputs(fx, cin, 41)
    settings = [ref.SETTINGS[0], ref.SETTINGS[1]]
    mod = sa_module(cin, [[16, 24], [32, 32]], "max_pool", 50, settings).eval()
    p = numpy_state(mod)
    want = np.concatenate([ref.neighbor_sa_scale(p, k, features, fx["xyz"], fx["new_xyz"], fx["ref"][k][0], "max_pool")[0]
                           for k in range(2)], 1)
    with torch.no_grad():
        yard = torch.cat([compose(mod, k, torch.from_numpy(features), torch.from_numpy(fx["xyz"]),
                                  torch.from_numpy(fx["new_xyz"]), fx["ref"][k][0])[0] for k in range(2)], 1).numpy()
    m = copy.deepcopy(mod).cuda()
    g = directory(fx["indices"], fx["batch"], fx["shape"])
    args = (dev(fx["xyz"]), dev(fx["xyz_cnt"]), dev(fx["new_xyz"]), dev(fx["new_cnt"]), dev(coords), dev(features))
    with torch.no_grad():
        assert m.takes_fused(0, g) and m.takes_fused(1, g)
        fused = m(*args, g)
        monkeypatch.setenv("DF3D_ROI_POOL_FUSED", "0")
        assert not m.takes_fused(0, g)
        composed = m(*args, g)
        dense = m(*args, dev(fx["table"]))
        monkeypatch.delenv("DF3D_ROI_POOL_FUSED")
        assert not m.takes_fused(0, dev(fx["table"]))                 # the dense table always takes the composition
    assert not m.takes_fused(0, g)                                    # autograd on: the composition
    assert fused.shape == (108, 56)
    judge("module eval", [("fused", want, yard, fused.cpu().numpy()), ("composed", want, yard, composed.cpu().numpy())])
    assert torch.equal(composed, dense)


def test_module_trains_through_the_composed_path():
    fx = fixture(2)
    cin = 8
    features, coords = module_inputs(fx, cin, 61)
    settings = [ref.SETTINGS[0], ref.SETTINGS[1]]
    mod = sa_module(cin, [[16, 24], [32, 32]], "max_pool", 70, settings).train()
    weight = torch.from_numpy(np.random.RandomState(71).standard_normal((108, 56)).astype(np.float32))

    def host(dtype):
        m = copy.deepcopy(mod).to(dtype)
        f = torch.from_numpy(features).to(dtype).requires_grad_(True)
        out = torch.cat([compose(m, k, f, torch.from_numpy(fx["xyz"]), torch.from_numpy(fx["new_xyz"]), fx["ref"][k][0])[0]
                         for k in range(2)], 1)
        (out * weight.to(dtype)).sum().backward()
        res = {"out": out.detach().numpy(), "grad features": f.grad.numpy()}
        res.update({"grad " + n: q.grad.numpy() for n, q in m.named_parameters()})
        return res

    want, yard = host(torch.float64), host(torch.float32)
    m = copy.deepcopy(mod).cuda()
    f = dev(features).requires_grad_(True)
    out = m(dev(fx["xyz"]), dev(fx["xyz_cnt"]), dev(fx["new_xyz"]), dev(fx["new_cnt"]), dev(coords), f,
            directory(fx["indices"], fx["batch"], fx["shape"]))
    (out * weight.cuda()).sum().backward()
    got = {"out": out.detach().cpu().numpy(), "grad features": f.grad.cpu().numpy()}
    got.update({"grad " + n: q.grad.cpu().numpy() for n, q in m.named_parameters()})
    assert sorted(got) == sorted(want) and len(got) == 2 + 2 * 9
    judge("module train", [(k, want[k], yard[k], got[k]) for k in sorted(want)])


# ---------------------------------------------------------------------------------------------------- head
HEAD_LEVELS = (("x_a", 1, 8), ("x_b", 2, 16), ("x_c", 4, 16))
HEAD_RANGE = [-1.0, -2.4, 0.0, 7.0, 2.4, 1.0]                        # (x, y, z) minimum and maximum of the base grid
HEAD_VOXEL = [0.4, 0.2, 0.2]                                         # (x, y, z) cell size of the base grid


def head_cfg():
    def layer(radius, nsample, c, cout):
        return {"MLPS": [[c, cout]], "QUERY_RANGES": [[2, 2, 2]], "POOL_RADIUS": [radius], "NSAMPLE": [nsample],
                "POOL_METHOD": "max_pool"}
    return {"CLASS_AGNOSTIC": True, "SHARED_FC": [64, 64], "CLS_FC": [32], "REG_FC": [32], "DP_RATIO": 0.3,
            "ROI_GRID_POOL": {"FEATURES_SOURCE": [n for n, _, _ in HEAD_LEVELS], "GRID_SIZE": 3,
                              "POOL_LAYERS": {"x_a": layer(0.57, 8, 16, 16), "x_b": layer(1.0, 16, 32, 32),
                                              "x_c": layer(1.6, 16, 16, 32)}}}


def test_head_forward_against_float64():
    from dualfusion import roi_heads
    from dualfusion.spconv import SparseConvTensor
    fx = fixture(0)
    rs = np.random.RandomState(81)
    torch.manual_seed(82)
    head = roi_heads.VoxelRCNNHead({n: c for n, _, c in HEAD_LEVELS}, head_cfg(), HEAD_RANGE, HEAD_VOXEL).eval()
    randomize_bn(head, 83)
    rois = np.asarray([[[1.5, -0.6, 0.5, 1.6, 0.8, 0.6, 0.0], [3.0, 0.7, 0.4, 2.0, 1.0, 0.7, 0.6], [6.8, 1.9, 0.6, 1.8, 0.9, 0.6, -1.1]],
                       [[0.2, -1.5, 0.3, 1.4, 0.7, 0.5, 2.4], [4.4, 0.1, 0.5, 1.7, 0.9, 0.6, 0.0], [2.2, 1.2, 0.7, 1.2, 0.6, 0.8, 1.57]]],
                      dtype=np.float32)                              # three rotated, [0][2] partly outside the range
    levels, tensors = {}, {}
    for name, stride, c in HEAD_LEVELS:
        ind = fx["indices"].astype(np.int64)
        ind = np.unique(np.concatenate([ind[:, :1], ind[:, 1:] // stride], 1), axis=0)
        ind = ind[rs.permutation(len(ind))]
        ind = np.ascontiguousarray(ind[np.argsort(ind[:, 0], kind="stable")].astype(np.int32))
        shape = [-(-s // stride) for s in ref.GRID]
        feats = rs.standard_normal((len(ind), c)).astype(np.float32)
        levels[name] = (ind, shape, feats, stride)
        tensors[name] = SparseConvTensor(dev(feats), dev(ind), shape, 2)
    hd = copy.deepcopy(head).cuda()
    batch = {"batch_size": 2, "rois": dev(rois), "multi_scale_3d_features": tensors,
             "multi_scale_3d_strides": {n: s for n, s, _ in HEAD_LEVELS}}
    with torch.no_grad():
        grid_xyz = hd.get_global_grid_points_of_roi(dev(rois), 3)[0].cpu().numpy()
        out = hd(batch)
    with pytest.raises(KeyError, match="rois"):
        hd({k: v for k, v in batch.items() if k != "rois"})
    assert tuple(out["rcnn_cls"].shape) == (6, 1) and tuple(out["rcnn_reg"].shape) == (6, 7)
    # grid points: float32 products and sums of |coordinate| <= 8 m: a rotation (two products, one sum, float32 sine and
    # cosine) and the centre: a handful of roundings of 2^-24 relative each; 8 of them at the largest coordinate
    want_xyz = ref.global_grid_points(rois.reshape(6, 7), 3)
    assert grid_xyz.shape == (6, 27, 3)
    assert np.abs(grid_xyz - want_xyz).max() <= 8 * U32 * np.abs(want_xyz).max()
    new_xyz = np.ascontiguousarray(grid_xyz.reshape(-1, 3))
    frames = np.repeat(np.arange(2), 3 * 27)
    p = numpy_state(head)
    want_levels, yard_levels = [], []
    for k, (name, stride, c) in enumerate(HEAD_LEVELS):
        ind, shape, feats, _ = levels[name]
        xyz = np.ascontiguousarray(ref.voxel_centers(ind[:, 1:], stride, HEAD_VOXEL, HEAD_RANGE))
        cxyz = ref.grid_coords(new_xyz, HEAD_RANGE, HEAD_VOXEL, stride)
        new_coords = np.ascontiguousarray(np.concatenate([frames[:, None].astype(np.int32), cxyz[:, ::-1]], 1))
        g = head.roi_grid_pool_layers[k].groupers[0]
        table = ref.dense_table(ind, 2, shape)
        assert ref.near_boundary(table, xyz, new_xyz, new_coords, g.max_range, g.radius) == 0
        raw, found = ref.voxel_query(table, xyz, new_xyz, new_coords, g.max_range, g.radius, g.nsample)
        assert (found > 0).sum() >= 40
        pk = {q[len("roi_grid_pool_layers.%d." % k):]: v for q, v in p.items() if q.startswith("roi_grid_pool_layers.%d." % k)}
        want_levels.append(ref.neighbor_sa_scale(pk, 0, feats, xyz, new_xyz, raw, "max_pool")[0])
        with torch.no_grad():
            yard_levels.append(compose(head.roi_grid_pool_layers[k], 0, torch.from_numpy(feats), torch.from_numpy(xyz),
                                       torch.from_numpy(new_xyz), raw)[0])
    want_pooled = np.concatenate(want_levels, 1).reshape(6, -1)
    want_cls, want_reg = ref.head_layers(p, want_pooled)
    with torch.no_grad():
        shared = head.shared_fc_layer(torch.cat(yard_levels, 1).reshape(6, -1))
        yard_cls = head.cls_pred_layer(head.cls_fc_layers(shared)).numpy()
        yard_reg = head.reg_pred_layer(head.reg_fc_layers(shared)).numpy()
    judge("head", [("rcnn_cls", want_cls, yard_cls, out["rcnn_cls"].cpu().numpy()),
                   ("rcnn_reg", want_reg, yard_reg, out["rcnn_reg"].cpu().numpy())])
