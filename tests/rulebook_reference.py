"""Brute-force sparse-convolution rulebooks, written from the definitions: a coordinate -> row dict and plain loops.
No grid, no sort trick, nothing shared with oracle/ or the package.

A rulebook here is (outids [n_out, 4] int32 rows (b, z, y, x), nbr [K, n_out] int32, out_shape): nbr[k][o] is the input
row that output row o reads through kernel index k (z-major, then y, then x), or -1.

forward       out shape (s + 2p - d(k-1) - 1) // st + 1; the outputs are every (in + p - k d) / st that divides exactly
              and lies in range, sorted by (b, z, y, x); nbr[k][o] = row of the cell o st - p + k d.
submanifold   the outputs are the inputs in input row order; pad k // 2, stride 1.
transposed    out shape (s - 1) st - 2p + k + output_padding (dilation does not enter, as in the reference); the outputs are
              every in-range in st - p + k d; nbr[k][o] = row of (o + p - k d) / st where it divides exactly.
"""
import functools
import itertools

import numpy as np

# the geometries of tests/test_rulebook_host.py and tests/test_gpu_rulebook.py
FORWARD = [  # (ksize, stride, padding), dilation 1
    ((1, 1, 1), (1, 1, 1), (0, 0, 0)),
    ((3, 3, 3), (1, 1, 1), (1, 1, 1)),
    ((3, 3, 3), (1, 1, 1), (0, 0, 0)),
    ((3, 3, 3), (2, 2, 2), (1, 1, 1)),
    ((3, 3, 3), (2, 2, 2), (2, 2, 2)),
    ((3, 3, 3), (3, 3, 3), (0, 0, 0)),
    ((2, 2, 2), (2, 2, 2), (0, 0, 0)),
    ((2, 2, 2), (2, 2, 2), (1, 1, 1)),
    ((2, 2, 2), (3, 3, 3), (0, 0, 0)),
    ((2, 2, 2), (1, 1, 1), (0, 0, 0)),
    ((1, 3, 2), (1, 2, 3), (0, 1, 2)),
    ((1, 5, 5), (1, 2, 2), (0, 2, 2)),
    ((2, 4, 4), (2, 2, 2), (0, 1, 1)),
    ((5, 5, 1), (2, 1, 1), (2, 0, 0)),
    ((3, 3, 3), (1, 2, 3), (1, 0, 2)),
    ((3, 1, 1), (2, 1, 1), (0, 0, 0)),
]
SUBM = [(1, 1, 1), (3, 3, 3), (1, 3, 3), (3, 1, 5), (5, 5, 1)]
TRANSPOSED = [  # (ksize, stride, padding, output_padding, dilation)
    ((3, 3, 3), (2, 2, 2), (1, 1, 1), (0, 0, 0), (1, 1, 1)),
    ((2, 2, 2), (2, 2, 2), (0, 0, 0), (0, 0, 0), (1, 1, 1)),
    ((3, 3, 3), (2, 2, 2), (1, 1, 1), (1, 1, 1), (1, 1, 1)),
    ((3, 3, 3), (1, 1, 1), (1, 1, 1), (0, 0, 0), (1, 1, 1)),
    ((2, 2, 2), (3, 3, 3), (0, 0, 0), (1, 0, 2), (1, 1, 1)),
    ((1, 3, 2), (1, 2, 3), (0, 1, 1), (0, 1, 0), (1, 1, 1)),
    ((3, 3, 3), (3, 3, 3), (2, 2, 2), (0, 0, 0), (1, 1, 1)),
    ((2, 4, 4), (2, 2, 2), (0, 1, 1), (0, 0, 0), (1, 1, 1)),
    ((3, 3, 3), (2, 2, 2), (1, 1, 1), (0, 0, 0), (2, 2, 2)),
]
# the forward geometries whose kernel volume no other device test reaches: K = 1, 6, 8, 25, 32
VALUE_GEOMETRIES = [g for g in FORWARD if g[0] in ((1, 1, 1), (1, 3, 2), (1, 5, 5), (2, 4, 4))] + [FORWARD[6]]

SWEEP_BATCH, SWEEP_SHAPE = 3, [5, 13, 70]


@functools.lru_cache(maxsize=None)
def sweep_voxels():
    """About 1300 clustered voxels, batch 3, X > 64, rows NOT in flat-index order."""
    import detgen
    return _frozen(detgen.clustered_voxels("rulebook_sweep", SWEEP_BATCH, SWEEP_SHAPE, n_seeds=4, walk=150))


@functools.lru_cache(maxsize=None)
def sweep_rulebook(kind, geometry):
    """The rulebook of `sweep_voxels()` at one entry of FORWARD / SUBM / TRANSPOSED, computed once per process and shared
    read-only: (outids, nbr, out_shape, pairs, num)."""
    ind = sweep_voxels()
    if kind == "forward":
        outids, nbr, out_shape = forward(ind, SWEEP_SHAPE, *geometry)
    elif kind == "subm":
        outids, nbr, out_shape = submanifold(ind, SWEEP_SHAPE, geometry)
    else:
        outids, nbr, out_shape = transposed(ind, SWEEP_SHAPE, *geometry)
    pairs, num = pairs_of(nbr, len(ind))
    return _frozen(outids), _frozen(nbr), tuple(out_shape), _frozen(pairs), _frozen(num)


def _frozen(a):
    a.setflags(write=False)
    return a


def tag(geometry):
    """test id of a geometry: k333-s222-p111[-o000-d222]"""
    parts = geometry if isinstance(geometry[0], tuple) else (geometry,)
    return "-".join(c + "".join(str(v) for v in p) for c, p in zip("kspod", parts))


def taps(ksize):
    return list(itertools.product(range(ksize[0]), range(ksize[1]), range(ksize[2])))


def rows_of(indices):
    table = {}
    for r, c in enumerate(np.asarray(indices).tolist()):
        assert tuple(c) not in table, "duplicate voxel"
        table[tuple(c)] = r
    return table


def conv_out_shape(shape, ksize, stride, padding, dilation=(1, 1, 1)):
    return [(shape[d] + 2 * padding[d] - dilation[d] * (ksize[d] - 1) - 1) // stride[d] + 1 for d in range(3)]


def deconv_out_shape(shape, ksize, stride, padding, output_padding=(0, 0, 0)):
    return [(shape[d] - 1) * stride[d] - 2 * padding[d] + ksize[d] + output_padding[d] for d in range(3)]


def _ids(cells):
    return np.asarray(sorted(cells), dtype=np.int32).reshape(-1, 4)


def _table(outids, ksize, source):
    """nbr[k][o] = source(output cell, tap) -> input row or -1"""
    kk = taps(ksize)
    nbr = np.full((len(kk), len(outids)), -1, dtype=np.int32)
    for o, c in enumerate(outids.tolist()):
        for k, t in enumerate(kk):
            nbr[k, o] = source(c, t)
    return nbr


def forward(indices, shape, ksize, stride, padding, dilation=(1, 1, 1)):
    out_shape = conv_out_shape(shape, ksize, stride, padding, dilation)
    table = rows_of(indices)
    cells = set()
    for (b, *c) in table:
        for t in taps(ksize):
            num = [c[d] + padding[d] - t[d] * dilation[d] for d in range(3)]
            if all(num[d] % stride[d] == 0 and 0 <= num[d] // stride[d] < out_shape[d] for d in range(3)):
                cells.add((b,) + tuple(num[d] // stride[d] for d in range(3)))
    outids = _ids(cells)

    def source(c, t):
        return table.get((c[0],) + tuple(c[1 + d] * stride[d] - padding[d] + t[d] * dilation[d] for d in range(3)), -1)

    return outids, _table(outids, ksize, source), out_shape


def submanifold(indices, shape, ksize):
    table = rows_of(indices)
    outids = np.asarray(indices, dtype=np.int32).reshape(-1, 4)

    def source(c, t):
        return table.get((c[0],) + tuple(c[1 + d] - ksize[d] // 2 + t[d] for d in range(3)), -1)

    return outids, _table(outids, ksize, source), list(shape)


def transposed(indices, shape, ksize, stride, padding, output_padding=(0, 0, 0), dilation=(1, 1, 1)):
    out_shape = deconv_out_shape(shape, ksize, stride, padding, output_padding)
    table = rows_of(indices)
    cells = set()
    for (b, *c) in table:
        for t in taps(ksize):
            o = [c[d] * stride[d] - padding[d] + t[d] * dilation[d] for d in range(3)]
            if all(0 <= o[d] < out_shape[d] for d in range(3)):
                cells.add((b,) + tuple(o))
    outids = _ids(cells)

    def source(c, t):
        num = [c[1 + d] + padding[d] - t[d] * dilation[d] for d in range(3)]
        if any(num[d] % stride[d] for d in range(3)):
            return -1
        return table.get((c[0],) + tuple(num[d] // stride[d] for d in range(3)), -1)

    return outids, _table(outids, ksize, source), out_shape


# ------------------------------------------------------------------------------------------------ derived forms
def pairs_of(nbr, n_in):
    """-> (pairs [K, 2, n_in] int32 padded with -1, num [K] int32): per kernel index the (input row, output row) pairs in
    ascending output row."""
    K, n_out = nbr.shape
    pairs = np.full((K, 2, n_in), -1, dtype=np.int32)
    num = np.zeros((K,), dtype=np.int32)
    for k in range(K):
        rows = np.nonzero(nbr[k] >= 0)[0]                  # ascending output row
        num[k] = len(rows)
        pairs[k, 0, :len(rows)], pairs[k, 1, :len(rows)] = nbr[k, rows], rows
    return pairs, num


def inverse_of(nbr, n_in):
    """inv[k][i] = o for every pair (a forward or submanifold (k, i) has at most one output: asserted)"""
    K, n_out = nbr.shape
    inv = np.full((K, n_in), -1, dtype=np.int32)
    for k in range(K):
        rows = np.nonzero(nbr[k] >= 0)[0]
        assert len(set(nbr[k, rows].tolist())) == len(rows)
        inv[k, nbr[k, rows]] = rows
    return inv


def conv(features, filters, nbr):
    """out[o] = sum_k features[nbr[k][o]] @ filters[k], float64"""
    x, w = np.asarray(features, np.float64), np.asarray(filters, np.float64)
    out = np.zeros((nbr.shape[1], w.shape[2]))
    for k in range(nbr.shape[0]):
        for o in np.nonzero(nbr[k] >= 0)[0]:
            out[o] += x[nbr[k, o]] @ w[k]
    return out


def conv_input_grad(grad_out, filters, nbr, n_in):
    g, w = np.asarray(grad_out, np.float64), np.asarray(filters, np.float64)
    gin = np.zeros((n_in, w.shape[1]))
    for k in range(nbr.shape[0]):
        for o in np.nonzero(nbr[k] >= 0)[0]:
            gin[nbr[k, o]] += w[k] @ g[o]
    return gin


def conv_filter_grad(features, grad_out, nbr):
    x, g = np.asarray(features, np.float64), np.asarray(grad_out, np.float64)
    gw = np.zeros((nbr.shape[0], x.shape[1], g.shape[1]))
    for k in range(nbr.shape[0]):
        for o in np.nonzero(nbr[k] >= 0)[0]:
            gw[k] += np.outer(x[nbr[k, o]], g[o])
    return gw
