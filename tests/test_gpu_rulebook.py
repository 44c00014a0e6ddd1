"""Rulebook geometry (csrc/rulebook.hip) and the device-wide scan under it (csrc/common.hip) against the brute-force
rulebooks of tests/rulebook_reference.py, which tests/test_rulebook_host.py pins to the oracle and the reference build.

Everything about indices is compared EXACTLY: the output set, the neighbour table element for element (it is deterministic
by construction, so no canonical form is needed), the reference-format pairs in ascending output row, the inverse table, and
a second build bit for bit.  Only the convolution values have a tolerance: the suite's bound for the exact-fp32 path, max
abs error <= 1e-3 max |float64 sum| (tests/test_gpu_ops.py::test_sparse_conv_transpose_golden); the measured figures are
printed.

The directory is one bit per cell and an exclusive popcount prefix per 64-cell word, scanned in tiles of 1024 words; the
grids of GRIDS sit on the word and tile edges of that layout (a 1 x 1 x 1 submanifold table is rank-through-perm at every
occupied word, a 1 x 1 x 1 stride-1 convolution is the enumeration of every word with its carries and the grand total)."""
import functools

import numpy as np
import pytest

import rulebook_reference as rb

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
B, SHAPE = rb.SWEEP_BATCH, rb.SWEEP_SHAPE
ONE = (1, 1, 1)
SCAN_TILE = 1024          # items per tile of the scan (csrc/common.hip)


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()         # (a copy: the shared references are read-only)


def host(t):
    return t.cpu().numpy()


def same(t, want):
    """exact equality of a device tensor and a host array, shape included"""
    got = host(t)
    return got.shape == tuple(np.shape(want)) and np.array_equal(got, want)


def device_rulebook(ind_d, batch, shape, kind, geometry, rows_sorted=False):
    """-> (outids, nbr, out_shape) through the kernel-facing entry points"""
    from dualfusion import ops
    grid = ops.grid_build(ind_d, batch, list(shape), rows_sorted=rows_sorted)
    if kind == "subm":
        return ind_d, ops.subm_neighbors(grid, ind_d, list(geometry)), list(shape)
    if kind == "forward":
        ks, st, pd = geometry
        dl, tr = ONE, False
        out_shape = rb.conv_out_shape(shape, ks, st, pd)
    else:
        ks, st, pd, op, dl = geometry
        tr = True
        out_shape = rb.deconv_out_shape(shape, ks, st, pd, op)
    outids, _ = ops.conv_out_indices(ind_d, batch, list(shape), out_shape, list(ks), list(st), list(pd), list(dl), transpose=tr)
    nbr = ops.conv_neighbors(grid, outids, list(ks), list(st), list(pd), list(dl), transpose=tr)
    return outids, nbr, out_shape


# ------------------------------------------------------------------------------------------ a. geometry sweep
def check_geometry(kind, geometry):
    from dualfusion import ops
    ind = rb.sweep_voxels()
    n = len(ind)
    want_out, want_nbr, want_shape, want_pairs, want_num = rb.sweep_rulebook(kind, geometry)
    ind_d = dev(ind)
    outids, nbr, out_shape = device_rulebook(ind_d, B, SHAPE, kind, geometry)
    assert list(out_shape) == list(want_shape)
    assert outids.shape[0] == len(want_out), (outids.shape[0], len(want_out))
    assert same(outids, want_out)
    assert same(nbr, want_nbr), np.argwhere(host(nbr) != want_nbr)[:5]
    pairs, num = ops.nbr_to_pairs(nbr, n)
    assert same(num, want_num) and same(pairs, want_pairs)
    assert torch.equal(ops.pairs_to_nbr(pairs.contiguous(), num, nbr.shape[1]), nbr)
    if kind != "transposed":
        want_inv = rb.inverse_of(want_nbr, n)
        assert same(ops.invert_neighbors(nbr, n), want_inv)
        if kind == "subm":     # what the backward of a submanifold convolution relies on: the mirrored table IS the inverse
            assert np.array_equal(want_inv, want_nbr[::-1])
    outids2, nbr2, _ = device_rulebook(dev(ind), B, SHAPE, kind, geometry)
    assert torch.equal(outids2, outids) and torch.equal(nbr2, nbr)
    return outids, nbr


@pytest.mark.parametrize("ks,st,pd", rb.FORWARD, ids=[rb.tag(g) for g in rb.FORWARD])
def test_forward_geometry(ks, st, pd):
    outids, nbr = check_geometry("forward", (ks, st, pd))
    assert nbr.shape[0] == ks[0] * ks[1] * ks[2] and outids.shape[0] > 0


@pytest.mark.parametrize("ks", rb.SUBM, ids=[rb.tag(g) for g in rb.SUBM])
def test_submanifold_geometry(ks):
    check_geometry("subm", ks)


@pytest.mark.parametrize("ks,st,pd,op,dl", rb.TRANSPOSED, ids=[rb.tag(g) for g in rb.TRANSPOSED])
def test_transposed_geometry(ks, st, pd, op, dl):
    check_geometry("transposed", (ks, st, pd, op, dl))


def test_reference_format_entry_point_and_module():
    from dualfusion import spconv
    ind = rb.sweep_voxels()
    ind_d = dev(ind)
    fwd = ((2, 4, 4), (2, 2, 2), (0, 1, 1))
    want = rb.sweep_rulebook("forward", fwd)
    outids, pairs, num = spconv.ops.get_indice_pairs(ind_d, B, SHAPE, list(fwd[0]), list(fwd[1]), list(fwd[2]), 1, 0, subm=False)
    assert same(outids, want[0]) and same(pairs, want[3]) and same(num, want[4])
    tr = ((2, 2, 2), (3, 3, 3), (0, 0, 0), (1, 0, 2), (1, 1, 1))
    want = rb.sweep_rulebook("transposed", tr)
    outids, pairs, num = spconv.ops.get_indice_pairs(ind_d, B, SHAPE, list(tr[0]), list(tr[1]), list(tr[2]), list(tr[4]),
                                                     list(tr[3]), subm=False, transpose=True)
    assert same(outids, want[0]) and same(pairs, want[3]) and same(num, want[4])
    sub = (3, 1, 5)
    want = rb.sweep_rulebook("subm", sub)
    outids, pairs, num = spconv.ops.get_indice_pairs(ind_d, B, SHAPE, list(sub), 1, [1, 0, 2], 1, 0, subm=True)
    assert same(outids, want[0]) and same(pairs, want[3]) and same(num, want[4])
    mod = ((1, 3, 2), (1, 2, 3), (0, 1, 2))
    want = rb.sweep_rulebook("forward", mod)
    m = spconv.SparseConv3d(16, 16, mod[0], stride=mod[1], padding=mod[2], bias=False).cuda().eval()
    with torch.no_grad():
        y = m(spconv.SparseConvTensor(torch.zeros((len(ind), 16), device="cuda"), ind_d, SHAPE, B))
    assert same(y.indices, want[0]) and list(y.spatial_shape) == list(want[2]) and y.features.shape == (len(want[0]), 16)


# ------------------------------------------------------------------------------------------ b. values, K in {1, 6, 8, 25, 32}
@functools.lru_cache(maxsize=None)
def value_case(geometry):
    """operands and the float64 sums over the brute-force table, once per geometry"""
    ks = geometry[0]
    K = ks[0] * ks[1] * ks[2]
    outids, nbr = rb.sweep_rulebook("forward", geometry)[:2]
    rs = np.random.RandomState(1000 + K)
    n = len(rb.sweep_voxels())
    x = rs.standard_normal((n, 16)).astype(np.float32)
    w = (rs.standard_normal((K, 16, 16)) * 0.2).astype(np.float32)
    g = rs.standard_normal((len(outids), 16)).astype(np.float32)
    return x, w, g, rb.conv(x, w, nbr), rb.conv_input_grad(g, w, nbr, n), rb.conv_filter_grad(x, g, nbr)


def rel(got, want):
    return float(np.abs(host(got).astype(np.float64).reshape(want.shape) - want).max() / np.abs(want).max())


@pytest.mark.parametrize("ks,st,pd", rb.VALUE_GEOMETRIES, ids=[rb.tag(g) for g in rb.VALUE_GEOMETRIES])
def test_values_and_gradients_at_other_kernel_volumes(ks, st, pd):
    from dualfusion import ops, spconv
    from dualfusion.spconv.conv import SparseConvFunction
    K = ks[0] * ks[1] * ks[2]
    assert K in (1, 6, 8, 25, 32)
    x, w, g, want_y, want_gx, want_gw = value_case((ks, st, pd))
    ind_d = dev(rb.sweep_voxels())
    outids, nbr, out_shape = device_rulebook(ind_d, B, SHAPE, "forward", (ks, st, pd))
    n_out = outids.shape[0]
    assert n_out == len(want_y)
    figures = {}
    with ops.precision("fp32"):
        assert ops.conv_kind(K, 16, 16) == "fp32"
        figures["y"] = rel(ops.sparse_conv_fused(dev(x), dev(w), nbr, n_out), want_y)
        # the autograd function of the modules, on the kernel-facing table (a 1 x 1 x 1 module is a plain matrix product and
        # never reaches the convolution kernels, so the function is called directly as well)
        xf, wf = dev(x).requires_grad_(True), dev(w.reshape(tuple(ks) + (16, 16))).requires_grad_(True)
        y = SparseConvFunction.apply(xf, wf, None, nbr, n_out, False)
        y.backward(dev(g))
        figures["fn y"], figures["fn gx"], figures["fn gw"] = rel(y.detach(), want_y), rel(xf.grad, want_gx), rel(wf.grad, want_gw)
        m = spconv.SparseConv3d(16, 16, ks, stride=st, padding=pd, bias=False).cuda().train()
        with torch.no_grad():
            m.weight.copy_(dev(w.reshape(tuple(ks) + (16, 16))))
        xm = dev(x).requires_grad_(True)
        out = m(spconv.SparseConvTensor(xm, ind_d, SHAPE, B))
        want_out, want_nbr = rb.sweep_rulebook("forward", (ks, st, pd))[:2]
        # (like the reference's, the 1 x 1 x 1 module leaves the rows where they are: output row o is input row nbr[0][o])
        rows = dev(want_nbr[0].astype(np.int64)) if K == 1 else torch.arange(n_out, device="cuda")
        assert same(out.indices[rows], want_out)
        gm = torch.zeros_like(out.features)
        gm[rows] = dev(g)
        out.features.backward(gm)
        figures["module y"], figures["module gx"] = rel(out.features.detach()[rows], want_y), rel(xm.grad, want_gx)
        figures["module gw"] = rel(m.weight.grad, want_gw)
    print("K = %2d: max abs error / max |float64| (bound 1e-3): %s"
          % (K, ", ".join("%s %.2e" % kv for kv in sorted(figures.items()))))
    for name, v in figures.items():
        assert v <= 1e-3, (name, v)


# ------------------------------------------------------------------------------------------ c. word and tile edges
GRIDS = [  # (batch, shape, words, tiles of the scan)
    (1, (1, 3, 5), 1, 1),               # 15 cells: a partial single word
    (1, (1, 8, 8), 1, 1),               # exactly one full word
    (1, (1, 5, 13), 2, 1),              # one cell into the second word
    (3, (3, 7, 11), 11, 1),             # volume 231: batch edges inside words
    (2, (2, 3, 64), 12, 1),             # X = 64
    (2, (2, 3, 65), 13, 1),             # X = 65
    (2, (9, 7, 1), 2, 1),               # X = 1
    (1, (2, 3, 129), 13, 1),            # X = 129
    (1, (16, 64, 64), 1024, 1),         # exactly one tile: the last launch-free size
    (1, (1, 255, 257), 1024, 1),        # one tile whose last word is one cell short
    (1, (1, 241, 272), 1025, 2),        # one tile plus one word
    (1, (1, 285, 460), 2049, 3),        # two tiles plus one word
    (2, (41, 453, 452), 262344, 257),   # just past 256 tiles: the tile-sum loop makes a second pass in some threads only
    (1, (41, 1000, 960), 615000, 601),  # more than 512 tiles
]


def coords_of(flat, shape):
    Z, Y, X = shape
    flat = np.asarray(flat, dtype=np.int64)
    return np.stack([flat // (Z * Y * X), flat // (Y * X) % Z, flat // X % Y, flat % X], 1).astype(np.int32)


def edge_cells(batch, shape, seed):
    """sorted flat indices: the first cell, the last cell of every batch element, both sides of every 64-cell boundary (so of
    every 1024-word boundary too), 192 consecutive cells across the first tile boundary, and some thousand random cells"""
    vol = shape[0] * shape[1] * shape[2]
    ncells = batch * vol
    edges = 64 * np.arange(1, (ncells - 1) // 64 + 1, dtype=np.int64)
    parts = [np.zeros(1, np.int64), vol * np.arange(1, batch + 1, dtype=np.int64) - 1, edges - 1, edges]
    tile = 64 * SCAN_TILE
    if ncells >= tile + 96:
        parts.append(np.arange(tile - 96, tile + 96, dtype=np.int64))
    parts.append(np.random.RandomState(seed).randint(0, ncells, size=min(3000, max(ncells // 3, 1))).astype(np.int64))
    flat = np.unique(np.concatenate(parts))
    assert flat[0] == 0 and flat[-1] == ncells - 1
    return flat


def check_directory(batch, shape, flat, seed, brute_force):
    """flat: sorted distinct flat indices of the occupied cells"""
    from dualfusion import ops
    n = len(flat)
    rows_sorted = coords_of(flat, shape)
    order = np.random.RandomState(seed).permutation(n)
    ind_d, sorted_d = dev(rows_sorted[order]), dev(rows_sorted)
    rank = torch.arange(n, dtype=torch.int32, device="cuda").view(1, n)
    grid = ops.grid_build(ind_d, batch, list(shape))
    assert grid.perm is not None
    assert torch.equal(ops.subm_neighbors(grid, ind_d, [1, 1, 1]), rank)
    plain = ops.grid_build(sorted_d, batch, list(shape), rows_sorted=True)
    assert plain.perm is None
    assert torch.equal(ops.subm_neighbors(plain, sorted_d, [1, 1, 1]), rank)
    outids, _ = ops.conv_out_indices(ind_d, batch, list(shape), list(shape), [1, 1, 1], [1, 1, 1], [0, 0, 0])
    assert outids.shape[0] == n
    assert torch.equal(outids, sorted_d)
    if brute_force:
        want = rb.submanifold(rows_sorted[order], shape, (3, 3, 3))[1]
        assert same(ops.subm_neighbors(grid, ind_d, [3, 3, 3]), want)
        want = rb.submanifold(rows_sorted, shape, (3, 3, 3))[1]
        assert same(ops.subm_neighbors(plain, sorted_d, [3, 3, 3]), want)


@pytest.mark.parametrize("batch,shape,words,tiles", GRIDS, ids=["%dx%dx%dx%d" % ((g[0],) + g[1]) for g in GRIDS])
def test_directory_at_word_and_tile_edges(batch, shape, words, tiles):
    ncells = batch * shape[0] * shape[1] * shape[2]
    assert (ncells + 63) // 64 == words and (words + SCAN_TILE - 1) // SCAN_TILE == tiles
    flat = edge_cells(batch, shape, seed=words)
    check_directory(batch, shape, flat, seed=words + 1, brute_force=ncells <= 70000)


def test_directory_fully_occupied_and_last_cell_only():
    shape = (3, 5, 7)
    check_directory(2, shape, np.arange(2 * 105, dtype=np.int64), seed=3, brute_force=True)
    check_directory(2, shape, np.asarray([2 * 105 - 1], dtype=np.int64), seed=4, brute_force=True)
    # the last cell of the last word of a grid that fills its words exactly
    check_directory(1, (1, 8, 8), np.asarray([63], dtype=np.int64), seed=5, brute_force=True)
    check_directory(2, (2, 4, 8), np.asarray([0, 63, 64, 127], dtype=np.int64), seed=6, brute_force=True)


def test_empty_voxel_set():
    from dualfusion import ops, spconv
    ind = torch.empty((0, 4), dtype=torch.int32, device="cuda")
    shape = [3, 5, 7]
    for rows_sorted in (False, True):
        grid = ops.grid_build(ind, 2, shape, rows_sorted=rows_sorted)
        assert tuple(ops.subm_neighbors(grid, ind, [1, 1, 1]).shape) == (1, 0)
        assert tuple(ops.subm_neighbors(grid, ind, [3, 3, 3]).shape) == (27, 0)
    outids, out_dir = ops.conv_out_indices(ind, 2, shape, shape, [1, 1, 1], [1, 1, 1], [0, 0, 0])
    assert tuple(outids.shape) == (0, 4)
    outids, out_dir = ops.conv_out_indices(ind, 2, shape, [2, 3, 4], [3, 3, 3], [2, 2, 2], [1, 1, 1])
    assert tuple(outids.shape) == (0, 4)
    nbr = ops.conv_neighbors(grid, outids, [3, 3, 3], [2, 2, 2], [1, 1, 1])
    assert tuple(nbr.shape) == (27, 0)
    pairs, num = ops.nbr_to_pairs(nbr, 0)
    assert tuple(pairs.shape) == (27, 2, 0) and same(num, np.zeros(27, np.int32))
    assert tuple(ops.pairs_to_nbr(pairs.contiguous(), num, 0).shape) == (27, 0)
    assert tuple(ops.invert_neighbors(nbr, 0).shape) == (27, 0)
    outids, pairs, num = spconv.ops.get_indice_pairs(ind, 2, shape, 3, 2, 1, 1, 0, subm=False, transpose=True)
    assert tuple(outids.shape) == (0, 4) and same(num, np.zeros(27, np.int32))
    # an occupied directory queried by an empty output list, and an empty one by occupied rows
    full = dev(coords_of(np.arange(10), shape))
    assert tuple(ops.conv_neighbors(ops.grid_build(full, 2, shape), outids, [3, 3, 3], [2, 2, 2], [1, 1, 1]).shape) == (27, 0)
    assert same(ops.subm_neighbors(grid, full, [3, 3, 3]), np.full((27, 10), -1, np.int32))


@pytest.mark.parametrize("K,n_out", [(8, 128), (1, 1025), (27, 9710), (1, 1), (32, 33)])
def test_pairs_from_a_table_at_the_scan_edges(K, n_out):
    """nbr_to_pairs scans K n_out flags: exactly one tile, one tile plus one item, just past 256 tiles"""
    from dualfusion import ops
    items = K * n_out
    assert items in (1024, 1025, 1, 1056) or items > 256 * SCAN_TILE
    rs = np.random.RandomState(items % 9973)
    nbr = np.where(rs.uniform(size=(K, n_out)) < 0.6, rs.randint(0, n_out, size=(K, n_out)), -1).astype(np.int32)
    nbr[:, 0], nbr[:, -1] = 0, n_out - 1                           # the first and the last item of every segment are set ...
    if K > 1:
        nbr[K // 2] = -1                                           # ... one segment is empty, one is full
        nbr[K - 1] = np.arange(n_out)
    want_pairs, want_num = rb.pairs_of(nbr, n_out)
    nbr_d = dev(nbr)
    pairs, num = ops.nbr_to_pairs(nbr_d, n_out)
    assert same(num, want_num)
    assert same(pairs, want_pairs)
    assert torch.equal(ops.pairs_to_nbr(pairs.contiguous(), num, n_out), nbr_d)
    pairs2, num2 = ops.nbr_to_pairs(nbr_d, n_out)
    assert torch.equal(pairs2, pairs) and torch.equal(num2, num)


# ------------------------------------------------------------------------------------------ d. capacity bound at equality
@pytest.mark.parametrize("ks,st,pd,first,fan", [((3, 3, 3), (1, 1, 1), (1, 1, 1), 2, 27), ((3, 3, 3), (2, 2, 2), (1, 1, 1), 1, 8)],
                         ids=["k333-s111-p111", "k333-s222-p111"])
def test_output_count_reaches_the_capacity_bound(ks, st, pd, first, fan):
    """isolated interior voxels, 4 cells apart: every input makes prod(ceil(k / s)) outputs of its own, which is exactly the
    capacity conv_out_indices allocates (n min(prod ceil(k / s), K), below the output volume here)"""
    from dualfusion import ops
    batch, shape = 2, (9, 13, 17)
    cells = [(b, z, y, x) for b in range(batch) for z in range(first, 8, 4) for y in range(first, 12, 4)
             for x in range(first, 16, 4)]
    ind = np.asarray(cells, dtype=np.int32)[np.random.RandomState(8).permutation(len(cells))]
    n = len(ind)
    assert n == 48
    want_out, want_nbr, out_shape = rb.forward(ind, shape, ks, st, pd)
    cap = n * min(int(np.prod([-(-k // s) for k, s in zip(ks, st)])), 27)
    assert len(want_out) == fan * n == cap < batch * int(np.prod(out_shape))
    outids, nbr, _ = device_rulebook(dev(ind), batch, shape, "forward", (ks, st, pd))
    assert outids.shape[0] == cap
    assert same(outids, want_out) and same(nbr, want_nbr)
    assert int((nbr >= 0).sum()) == cap                            # one input per output


# ------------------------------------------------------------------------------------------ e. refusals are reported
def test_unsupported_geometries_raise():
    from dualfusion import ops, spconv
    from dualfusion._lib import Df3dError
    ind_d = dev(rb.sweep_voxels())
    n = ind_d.shape[0]
    grid = ops.grid_build(ind_d, B, SHAPE)
    with pytest.raises(Df3dError):
        ops.conv_out_indices(ind_d, B, SHAPE, rb.conv_out_shape(SHAPE, (3, 3, 3), ONE, (2, 2, 2), (2, 2, 2)), [3, 3, 3], [1, 1, 1],
                             [2, 2, 2], [2, 2, 2])
    with pytest.raises(Df3dError):
        ops.subm_neighbors(grid, ind_d, [3, 3, 3], [2, 2, 2])
    with pytest.raises(Df3dError):
        ops.subm_neighbors(grid, ind_d, [3, 3, 3], [1, 2, 1])
    x = spconv.SparseConvTensor(torch.zeros((n, 16), device="cuda"), ind_d, SHAPE, B)
    with pytest.raises(Df3dError), torch.no_grad():
        spconv.SparseConv3d(16, 16, 3, stride=1, padding=2, dilation=2, bias=False).cuda().eval()(x)
    x = spconv.SparseConvTensor(torch.zeros((n, 16), device="cuda"), ind_d, SHAPE, B)
    with pytest.raises(Df3dError), torch.no_grad():
        spconv.SubMConv3d(16, 16, 3, dilation=2, bias=False).cuda().eval()(x)
    for ks in ([2, 2, 2], [3, 3, 2], [1, 4, 1]):
        with pytest.raises(Df3dError):
            ops.subm_neighbors(grid, ind_d, ks)
    big = [3, 3, 4]                                                # K = 36 > 32
    out_shape = rb.conv_out_shape(SHAPE, big, ONE, (1, 1, 1))
    with pytest.raises(Df3dError):
        ops.conv_out_indices(ind_d, B, SHAPE, out_shape, big, [1, 1, 1], [1, 1, 1])
    with pytest.raises(Df3dError):
        ops.conv_out_indices(ind_d, B, SHAPE, rb.deconv_out_shape(SHAPE, big, ONE, (1, 1, 1)), big, [1, 1, 1], [1, 1, 1],
                             transpose=True)
    with pytest.raises(Df3dError):
        ops.conv_neighbors(grid, ind_d, big, [1, 1, 1], [1, 1, 1])
    with pytest.raises(Df3dError):
        ops.conv_neighbors(grid, ind_d, big, [1, 1, 1], [1, 1, 1], transpose=True)
    with pytest.raises(Df3dError):
        ops.subm_neighbors(grid, ind_d, [3, 3, 5])                 # odd, K = 45
    # K = 32 is the limit and is served (the table itself is checked in test_forward_geometry)
    geometry = ((2, 4, 4), (2, 2, 2), (0, 1, 1))
    outids, nbr, _ = device_rulebook(ind_d, B, SHAPE, "forward", geometry)
    assert nbr.shape == (32, len(rb.sweep_rulebook("forward", geometry)[0]))
    # and the directory still answers after the refusals
    assert torch.equal(ops.subm_neighbors(grid, ind_d, [1, 1, 1]), torch.arange(n, dtype=torch.int32, device="cuda").view(1, n))
