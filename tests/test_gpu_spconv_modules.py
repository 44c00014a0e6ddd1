"""Every module of dualfusion/spconv -- values, active sets and gradients -- against the dense float64 network of
tests/spconv_dense_reference.py (torch.nn.functional on the CPU; tests/test_spconv_dense_host.py pins it to the goldens and
to the brute-force rulebooks).  The dense reference shares no rulebook, no `view(K, cin, cout)`, no offset order, no
row-to-coordinate mapping and no module wiring with the code under test: rows meet by coordinate only.

One cloud serves every case: batch 3 on [5, 9, 11] (odd sizes: stride 2 leaves a remainder), about 200 clustered voxels with
the first and the last cell of samples 0 and 2, sample 1 empty, rows not in flat-index order; the 2-D cases batch 2 on
[9, 11].  Features, weights (scaled by 1 / sqrt(K cin)) and the out-gradient G are seeded normals; G is a dense tensor read at
the module's own `out.indices`, so both sides get the same G by coordinate.

Per case and arithmetic mode ("fp32", "split", "split3", "bf16" under `ops.precision`): `out.indices` duplicate-free and equal
to the dense occupancy set, `out.spatial_shape`, the eval() forward under no_grad (fused inference path, cached packs), the
train() forward (SparseConvFunction), and d features / d weight / d bias of loss = (out.features * G).sum().

Bounds (tests/spconv_dense_reference.py `excess`): max |got - ref| <= 1e-4 max |ref| in the modes "fp32", "split", "split3",
for the pools and dense() (test_conv_backward_golden_and_autograd's bound on these modules; the pool forward and dense() are
exact); "bf16": elementwise |got - ref| <= ((1 + 2^-8)^(2 L) - 1) A + L 2e-5 max A with A the same computation on absolute
values and L the convolutions in a row (one layer: 2^-7 (1 + 2^-9) A + 2e-5 max A) -- two operands of each product rounded
to 8 significant bits, fp32 accumulation; for a gradient of an L-layer chain every path from an operand to the loss crosses
L products, forward or backward, so the same L holds.  Through five layers that worst case (every |w| summed without a sign,
five times over) is orders above the values themselves, so the chains are ALSO checked layer by layer on the rows the device
fed each layer (`chain_layerwise`), where the one-layer bound holds as it stands and has teeth in every mode.

`SparseConvTranspose3d`'s constructor takes no output_padding and refuses dilation 2 with stride 2 (like the reference's);
both are set on the module, as test_sparse_conv_transpose_golden does.

Measured on an MI355X over every case of this module, largest max |got - ref| / max |ref| (and the largest fraction of the
bound any element reached):
    fp32    2.0e-06  (0.020)   convT3d-k3s2p1op1, 32 -> 64
    split   1.4e-06  (0.014)   convT3d-k3s2p1d2, 32 -> 64
    split3  1.6e-06  (0.016)   the chain, end to end
    bf16    7.0e-03  (0.42)    the chain end to end (one layer: 2.2e-03 .. 3.3e-03); fraction: convT3d-k2s2, 32 -> 64
    pools   8.2e-08 on the gradient, forward exact;  dense() exact
No case measures above 1e-5 outside the bf16 mode.  (16, 16) and (12, 20) print the same figure in every mode: no format has
a matrix-core kernel for them (`ops.conv_kind`), so they fall to the exact-fp32 kernels whatever the mode.
"""
import functools
import math

import numpy as np
import pytest

import detgen
import spconv_dense_reference as sd

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

F64 = torch.float64
B3, SHAPE3 = 3, [5, 9, 11]
B2, SHAPE2 = 2, [9, 11]
# (cin, cout, bias): (32, 64) reaches the matrix-core kernels in every mode, (12, 20) falls to the exact-fp32 kernels
CHANNELS = [(16, 16, True), (32, 64, False), (12, 20, True)]


# ------------------------------------------------------------------------------------------------------------ inputs
def _with_corners(cells, batches, shape):
    cells = [tuple(c) for c in cells]
    for b in batches:
        for c in ((b,) + (0,) * len(shape), (b,) + tuple(s - 1 for s in shape)):
            if c not in cells:
                cells.append(c)
    arr = np.array(cells, np.int32)
    np.random.RandomState(7).shuffle(arr)
    key = sd.flat_key(arr, shape).numpy()
    assert (np.diff(key) < 0).any() and len(np.unique(key)) == len(key)      # not in flat-index order, no duplicates
    arr.setflags(write=False)
    return arr


@functools.lru_cache(maxsize=None)
def cloud(ndim):
    if ndim == 3:
        ind = detgen.clustered_voxels("spconv_modules_3d", B3, SHAPE3, n_seeds=2, walk=90)
        arr = _with_corners([c for c in ind.tolist() if c[0] != 1], (0, 2), SHAPE3)          # sample 1 is empty
        assert 150 <= len(arr) <= 250, len(arr)
        return arr
    ind = detgen.clustered_voxels("spconv_modules_2d", B2, [1] + SHAPE2, n_seeds=2, walk=40)
    return _with_corners([(c[0], c[2], c[3]) for c in ind.tolist()], (0, 1), SHAPE2)


def space(ndim):
    return (B3, SHAPE3) if ndim == 3 else (B2, SHAPE2)


def field(name, batch, channels, shape):
    """a dense seeded normal tensor [batch, channels, *shape]: rows are read from it by coordinate (fp32 values, in float64)"""
    return torch.from_numpy(detgen.randn(name, (batch, channels) + tuple(shape))).to(F64)


def weights(name, ks, cin, cout, bias):
    w = torch.from_numpy(detgen.randn(name + "_w", tuple(ks) + (cin, cout), 1.0 / math.sqrt(np.prod(ks) * cin))).to(F64)
    b = torch.from_numpy(detgen.randn(name + "_b", (cout,), 0.1)).to(F64) if bias else None
    return w, b


def cuda32(t):
    return t.detach().to(torch.float32).cuda().contiguous()


def load(module, w, b):
    """new values into the module's parameters IN PLACE (what an optimiser step does); gradients cleared"""
    with torch.no_grad():
        module.weight.copy_(cuda32(w))
        if b is not None:
            module.bias.copy_(cuda32(b))
    module.weight.grad = None
    if module.bias is not None:
        module.bias.grad = None


class Figures(object):
    """measured errors of one case: per mode the largest max |got - ref| / max |ref| and the largest fraction of the bound"""

    def __init__(self, label):
        self.label, self.rel, self.frac, self.failed = label, {}, {}, []

    def add(self, mode, what, got, ref, A=None, layers=1):
        rel, frac = sd.excess(got, ref, A, mode, layers)
        self.rel[mode] = max(self.rel.get(mode, 0.0), rel)
        self.frac[mode] = max(self.frac.get(mode, 0.0), frac)
        if not frac <= 1.0:
            self.failed.append("%s %s: %.3e of max |ref|, %.3g x the bound" % (mode, what, rel, frac))

    def same(self, mode, what, ok):
        if not ok:
            self.failed.append("%s %s" % (mode, what))

    def close(self):
        print("%s: max |got - ref| / max |ref| (x its bound): %s"
              % (self.label, ", ".join("%s %.2e (%.2g)" % (m, self.rel[m], self.frac[m]) for m in self.rel)))
        assert not self.failed, "%s: %s" % (self.label, "; ".join(self.failed))


def check_sites(fig, mode, out, ref_coords, ref_shape):
    """out.indices duplicate-free, = the dense occupancy set, out.spatial_shape -> reference row of every output row"""
    got = out.indices.cpu().long()
    fig.same(mode, "spatial_shape %s != %s" % (out.spatial_shape, ref_shape), list(out.spatial_shape) == list(ref_shape))
    assert got.shape[1] == ref_coords.shape[1]
    assert bool((got[:, 1:] >= 0).all()) and bool((got[:, 1:] < torch.tensor(ref_shape)).all()), "output index outside the output shape"
    assert not sd.has_duplicates(got, ref_shape), "duplicate rows in out.indices"
    assert sd.same_set(got, ref_coords, ref_shape), "active set differs from the dense occupancy set"
    return sd.rows_at(ref_coords, ref_shape, got)


# ------------------------------------------------------------------------------------------------- single modules
def geo3(k, s=1, p=0, op=0, d=1):
    t = lambda v: tuple(v) if isinstance(v, tuple) else (v,) * 3
    return dict(k=t(k), s=t(s), p=t(p), op=t(op), d=t(d))


def geo2(k, s=1, p=0, op=0):
    t = lambda v: tuple(v) if isinstance(v, tuple) else (v,) * 2
    return dict(k=t(k), s=t(s), p=t(p), op=t(op), d=(1, 1))


CASES = [  # (id, kind, ndim, geometry)
    ("subm3d-k333", "subm", 3, geo3(3)),
    ("subm3d-k133", "subm", 3, geo3((1, 3, 3))),
    ("subm3d-k315", "subm", 3, geo3((3, 1, 5))),
    ("subm3d-k551", "subm", 3, geo3((5, 5, 1))),
    ("conv3d-k3s2p1", "conv", 3, geo3(3, 2, 1)),
    ("conv3d-k3s1p1", "conv", 3, geo3(3, 1, 1)),
    ("conv3d-k3s1p0", "conv", 3, geo3(3, 1, 0)),
    ("conv3d-k2s2p0", "conv", 3, geo3(2, 2, 0)),
    ("conv3d-k2s2p1", "conv", 3, geo3(2, 2, 1)),
    ("conv3d-k311s211p0", "conv", 3, geo3((3, 1, 1), (2, 1, 1), 0)),
    ("conv3d-k3s2p011", "conv", 3, geo3(3, 2, (0, 1, 1))),
    ("conv3d-k244s2p011", "conv", 3, geo3((2, 4, 4), 2, (0, 1, 1))),
    ("conv3d-k132s123p012", "conv", 3, geo3((1, 3, 2), (1, 2, 3), (0, 1, 2))),
    ("conv3d-k111", "conv", 3, geo3(1)),
    ("convT3d-k3s2p1", "convT", 3, geo3(3, 2, 1)),
    ("convT3d-k2s2", "convT", 3, geo3(2, 2, 0)),
    ("convT3d-k3s2p1op1", "convT", 3, geo3(3, 2, 1, 1)),
    ("convT3d-k132s123p011op010", "convT", 3, geo3((1, 3, 2), (1, 2, 3), (0, 1, 1), (0, 1, 0))),
    ("convT3d-k2s3op102", "convT", 3, geo3(2, 3, 0, (1, 0, 2))),
    ("convT3d-k3s2p1d2", "convT", 3, geo3(3, 2, 1, 0, 2)),
    ("inverse3d-k3s2p1", "inv", 3, geo3(3, 2, 1)),
    ("inverse3d-k2s2", "inv", 3, geo3(2, 2, 0)),
    ("inverse3d-k311s211", "inv", 3, geo3((3, 1, 1), (2, 1, 1), 0)),
    ("inverse3d-k3s2p011", "inv", 3, geo3(3, 2, (0, 1, 1))),
    ("subm2d-k3", "subm", 2, geo2(3)),
    ("conv2d-k3s2p1", "conv", 2, geo2(3, 2, 1)),
    ("convT2d-k2s2", "convT", 2, geo2(2, 2, 0)),
    ("convT2d-k3s2p1op1", "convT", 2, geo2(3, 2, 1, 1)),
    ("convT2d-k3s2p1op10", "convT", 2, geo2(3, 2, 1, (1, 0))),       # (y, x) differ: the 3-D twin must keep their order
]


def make_module(kind, ndim, cin, cout, bias, g):
    """-> the module on the device in the reference's constructor arguments"""
    from dualfusion import spconv
    k, s, p = list(g["k"]), list(g["s"]), list(g["p"])
    if kind == "subm":
        m = (spconv.SubMConv3d if ndim == 3 else spconv.SubMConv2d)(cin, cout, k, bias=bias)
    elif kind == "conv":
        m = (spconv.SparseConv3d if ndim == 3 else spconv.SparseConv2d)(cin, cout, k, stride=s, padding=p, bias=bias)
    elif kind == "convT":
        m = (spconv.SparseConvTranspose3d if ndim == 3 else spconv.SparseConvTranspose2d)(cin, cout, k, stride=s, padding=p,
                                                                                        bias=bias)
        m.output_padding = list(g["op"])
        m.dilation = list(g["d"])
    else:
        m = spconv.SparseInverseConv3d(cin, cout, k, indice_key="d", bias=bias)
    return m.cuda()


def reference_call(kind, g, sites, shape):
    """-> (function of spconv_dense_reference, its geometry arguments)"""
    if kind == "subm":
        return sd.subm, {}
    if kind == "conv":
        return sd.conv, dict(stride=g["s"], padding=g["p"])
    if kind == "convT":
        return sd.conv_transpose, dict(stride=g["s"], padding=g["p"], output_padding=g["op"], dilation=g["d"])
    return sd.inverse, dict(sites=sites, sites_shape=shape, stride=g["s"], padding=g["p"])


@pytest.mark.parametrize("cin,cout,bias", CHANNELS, ids=["c%dx%d" % c[:2] for c in CHANNELS])
@pytest.mark.parametrize("label,kind,ndim,g", CASES, ids=[c[0] for c in CASES])
def test_module_values_and_gradients(label, kind, ndim, g, cin, cout, bias):
    from dualfusion import ops, spconv
    batch, shape = space(ndim)
    sites = cloud(ndim)
    name = "%s_%dx%d" % (label, cin, cout)
    ind_t = torch.from_numpy(np.array(sites)).cuda()
    if kind == "inv":
        # the layer's input lives on the output sites of the forward convolution registered under the key
        down = spconv.SparseConv3d(cout, cin, list(g["k"]), stride=list(g["s"]), padding=list(g["p"]), bias=False,
                                   indice_key="d").cuda().eval()
        in_ref, in_shape = sd.occupancy(sites, shape, batch, g["k"], g["s"], g["p"])

        def tensor_of(rows_of):
            with torch.no_grad():
                mid = down(spconv.SparseConvTensor(torch.zeros((len(sites), cout), device="cuda"), ind_t, shape, batch))
            return mid.replace_feature(rows_of(mid.indices.cpu().long()))
    else:
        in_ref, in_shape = torch.from_numpy(np.array(sites)).long(), shape

        def tensor_of(rows_of):
            return spconv.SparseConvTensor(rows_of(in_ref), ind_t, shape, batch)

    X = field(name + "_x", batch, cin, in_shape)
    w, b = weights(name, g["k"], cin, cout, bias)
    fn, kw = reference_call(kind, g, sites, shape)
    x = sd.gather(X, in_ref).requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    br = b.clone().requires_grad_(True) if bias else None
    ref_coords, ref_shape, y = fn(x, in_ref, in_shape, batch, wr, br, **kw)
    G = field(name + "_g", batch, cout, ref_shape)
    g_rows = sd.gather(G, ref_coords)
    grads = torch.autograd.grad(y, [x, wr] + ([br] if bias else []), g_rows)
    A_y, A_x, A_w, A_b = sd.abs_bound(fn, x, in_ref, in_shape, batch, w, b, grad=g_rows, **kw)

    m = make_module(kind, ndim, cin, cout, bias, g)
    fig = Figures(name)
    for mode in sd.MODES:
        load(m, w, b)
        with ops.precision(mode):
            m.eval()
            with torch.no_grad():
                out = m(tensor_of(lambda c: cuda32(sd.gather(X, c))))
            pos = check_sites(fig, mode, out, ref_coords, ref_shape)
            fig.add(mode, "eval y", out.features, y[pos], A_y[pos])
            m.train()
            feats = []

            def rows_with_grad(c):
                feats.append((cuda32(sd.gather(X, c)).requires_grad_(True), c))
                return feats[0][0]

            out = m(tensor_of(rows_with_grad))
            pos = check_sites(fig, mode, out, ref_coords, ref_shape)
            fig.add(mode, "train y", out.features, y[pos], A_y[pos])
            (out.features * cuda32(g_rows[pos])).sum().backward()
            xg, in_dev = feats[0]
            pin = sd.rows_at(in_ref, in_shape, in_dev)
            fig.add(mode, "d features", xg.grad, grads[0][pin], A_x[pin])
            fig.add(mode, "d weight", m.weight.grad, grads[1], A_w)
            if bias:
                fig.add(mode, "d bias", m.bias.grad, grads[2], A_b)
    fig.close()


# ------------------------------------------------------------------------------------------------ pools and dense()
POOLS = [("pool3d-k3s2p1", 3, 3, 2, 1), ("pool3d-k2s2", 3, 2, 2, 0), ("pool2d-k3s2p1", 2, 3, 2, 1)]
POOL_C, POOL_NEG = 16, 5


@pytest.mark.parametrize("label,ndim,k,s,p", POOLS, ids=[c[0] for c in POOLS])
def test_pool_values_and_gradients(label, ndim, k, s, p):
    """One channel is negative everywhere: the pooled value starts from zero.  Normals have no ties, so torch's one-winner
    gradient is the fan-out over equal values of the reference."""
    from dualfusion import spconv
    batch, shape = space(ndim)
    sites = cloud(ndim)
    ind = torch.from_numpy(np.array(sites)).long()
    X = field(label + "_x", batch, POOL_C, shape)
    X[:, POOL_NEG] = -X[:, POOL_NEG].abs() - 0.1
    x = sd.gather(X, ind).requires_grad_(True)
    ref_coords, ref_shape, y = sd.maxpool(x, ind, shape, batch, k, s, p)
    g_rows = sd.gather(field(label + "_g", batch, POOL_C, ref_shape), ref_coords)
    (gx,) = torch.autograd.grad(y, [x], g_rows)
    assert float(y.detach()[:, POOL_NEG].abs().max()) == 0.0 and float(gx[:, POOL_NEG].abs().max()) == 0.0
    pool = (spconv.SparseMaxPool3d if ndim == 3 else spconv.SparseMaxPool2d)(k, s, p)
    fig = Figures(label)
    ind_t = ind.int().cuda()
    with torch.no_grad():
        out = pool(spconv.SparseConvTensor(cuda32(x), ind_t, shape, batch))
    pos = check_sites(fig, "pool", out, ref_coords, ref_shape)
    assert torch.equal(out.features.cpu(), y[pos].detach().float()), "pool forward (no_grad) is not exact"
    feats = cuda32(x).requires_grad_(True)
    out = pool(spconv.SparseConvTensor(feats, ind_t, shape, batch))
    pos = check_sites(fig, "pool", out, ref_coords, ref_shape)
    assert torch.equal(out.features.detach().cpu(), y[pos].detach().float()), "pool forward is not exact"
    (out.features * cuda32(g_rows[pos])).sum().backward()
    fig.add("pool", "d features", feats.grad, gx)
    fig.close()


@pytest.mark.parametrize("ndim", [3, 2])
def test_dense_values_and_gradient(ndim):
    """SparseConvTensor.dense() (its own autograd function) against the densified rows; the gradient is G at the sites."""
    from dualfusion import spconv
    batch, shape = space(ndim)
    ind = torch.from_numpy(np.array(cloud(ndim))).long()
    C = 12
    x = sd.gather(field("dense%d_x" % ndim, batch, C, shape), ind)
    want = sd.dense(x, ind, shape, batch).float()
    G = field("dense%d_g" % ndim, batch, C, shape)
    ind_t = ind.int().cuda()
    with torch.no_grad():
        got = spconv.SparseConvTensor(cuda32(x), ind_t, shape, batch).dense()
    assert tuple(got.shape) == (batch, C) + tuple(shape) and torch.equal(got.cpu(), want)
    feats = cuda32(x).requires_grad_(True)
    t = spconv.SparseConvTensor(feats, ind_t, shape, batch)
    got = t.dense()
    assert torch.equal(got.detach().cpu(), want)
    (got * cuda32(G)).sum().backward()
    assert torch.equal(feats.grad.cpu(), sd.gather(G, ind).float())
    feats.grad = None
    last = t.dense(channels_first=False)                                          # [B, *shape, C]
    assert torch.equal(last.detach().cpu(), want.movedim(1, -1))
    (last * cuda32(G.movedim(1, -1))).sum().backward()
    assert torch.equal(feats.grad.cpu(), sd.gather(G, ind).float())


# -------------------------------------------------------------------------------------------------- chains and caches
CHAIN_C = [(16, 32), (32, 64), (64, 64), (64, 32), (32, 16)]
CHAIN_K = [(3, 3, 3)] * 5
CHAIN_LAYERS = 5


def chain_modules():
    """SubM (key a) -> strided conv (key d) -> SubM -> inverse conv (key d) -> SubM (key a), all with bias"""
    from dualfusion import spconv
    c = CHAIN_C
    return [spconv.SubMConv3d(c[0][0], c[0][1], 3, bias=True, indice_key="a").cuda(),
            spconv.SparseConv3d(c[1][0], c[1][1], 3, stride=2, padding=1, bias=True, indice_key="d").cuda(),
            spconv.SubMConv3d(c[2][0], c[2][1], 3, bias=True).cuda(),
            spconv.SparseInverseConv3d(c[3][0], c[3][1], 3, indice_key="d", bias=True).cuda(),
            spconv.SubMConv3d(c[4][0], c[4][1], 3, bias=True, indice_key="a").cuda()]


def chain_reference(x, ind, shape, batch, ws, bs):
    """the dense chain, masked to the active set at every stage -> rows at the input sites"""
    _, _, h = sd.subm(x, ind, shape, batch, ws[0], bs[0])
    mid, mid_shape, h = sd.conv(h, ind, shape, batch, ws[1], bs[1], 2, 1)
    _, _, h = sd.subm(h, mid, mid_shape, batch, ws[2], bs[2])
    _, _, h = sd.inverse(h, mid, mid_shape, batch, ws[3], bs[3], ind, shape, 2, 1)
    return sd.subm(h, ind, shape, batch, ws[4], bs[4])[2]


CHAIN_KIND = ["subm", "conv", "subm", "inv", "subm"]


def chain_layerwise(fig, mode, what, ts, g_last, mods, wb):
    """Every layer of the chain on its own, on the rows the DEVICE fed it: ts[l] -> ts[l + 1] against the dense layer of
    ts[l].features (and, with g_last, d ts[l].features / d weight / d bias against the dense layer's backward of the device's
    d ts[l + 1].features).  One convolution between operands and result, so the one-layer bound holds as it stands -- in the
    "bf16" mode this is the check with teeth: the elementwise bound of five layers in a row, every |w| summed without a sign
    five times over, is orders above the values themselves."""
    ind = torch.from_numpy(np.array(cloud(3))).long()
    for l, (m, (w, b)) in enumerate(zip(mods, wb)):
        t_in, t_out = ts[l], ts[l + 1]
        in_dev, in_shape = t_in.indices.cpu().long(), t_in.spatial_shape
        fn, kw = reference_call(CHAIN_KIND[l], dict(s=(2, 2, 2), p=(1, 1, 1)), ind, SHAPE3)
        x = t_in.features.detach().cpu().to(F64).requires_grad_(True)
        wr, br = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        ref_coords, ref_shape, y = fn(x, in_dev, in_shape, B3, wr, br, **kw)
        pos = check_sites(fig, mode, t_out, ref_coords, ref_shape)
        g_dev = None
        if g_last is not None:
            g_dev = (g_last if l == len(mods) - 1 else t_out.features.grad).detach().cpu().to(F64)
            g_ref = torch.zeros_like(y)
            g_ref[pos] = g_dev                                     # the device's out-gradient rows, by coordinate
        A = sd.abs_bound(fn, x, in_dev, in_shape, B3, w, b, grad=(g_ref if g_dev is not None else None), **kw)
        A_y = A[0] if g_dev is not None else A
        fig.add(mode, "%s layer %d y" % (what, l), t_out.features, y[pos], A_y[pos])
        if g_dev is not None:
            gx, gw, gb = torch.autograd.grad(y, [x, wr, br], g_ref)
            fig.add(mode, "%s layer %d d features" % (what, l), t_in.features.grad, gx, A[1])
            fig.add(mode, "%s layer %d d weight" % (what, l), m.weight.grad, gw, A[2])
            fig.add(mode, "%s layer %d d bias" % (what, l), m.bias.grad, gb, A[3])


def chain_step(fig, mods, step, mode, tensor_of):
    """One training step (and an eval forward) of the chain with the features and weights of `step`, against its own dense
    reference, end to end and layer by layer.  tensor_of(features) -> the input SparseConvTensor."""
    from dualfusion import ops
    ind = torch.from_numpy(np.array(cloud(3))).long()
    name = "chain_step%d" % step
    x = sd.gather(field(name + "_x", B3, CHAIN_C[0][0], SHAPE3), ind).requires_grad_(True)
    wb = [weights("%s_l%d" % (name, i), CHAIN_K[i], c[0], c[1], True) for i, c in enumerate(CHAIN_C)]
    ws, bs = [w.clone().requires_grad_(True) for w, _ in wb], [b.clone().requires_grad_(True) for _, b in wb]
    y = chain_reference(x, ind, SHAPE3, B3, ws, bs)
    g_rows = sd.gather(field(name + "_g", B3, CHAIN_C[-1][1], SHAPE3), ind)
    grads = torch.autograd.grad(y, [x] + ws + bs, g_rows)
    xa = x.detach().abs().requires_grad_(True)
    wa, ba = [w.abs().requires_grad_(True) for w, _ in wb], [b.abs().requires_grad_(True) for _, b in wb]
    A_y = chain_reference(xa, ind, SHAPE3, B3, wa, ba)
    A = torch.autograd.grad(A_y, [xa] + wa + ba, g_rows.abs())
    for m, (w, b) in zip(mods, wb):
        load(m, w, b)
    tag = "%s step %d" % (mode, step)
    with ops.precision(mode):
        for m in mods:
            m.eval()
        with torch.no_grad():
            ts = [tensor_of(cuda32(x))]
            for m in mods:
                ts.append(m(ts[-1]))
        t = ts[-1]
        fig.same(tag, "eval out.indices", torch.equal(t.indices.cpu().long(), ind) and t.spatial_shape == SHAPE3)
        fig.add(mode, "step %d eval y" % step, t.features, y, A_y.detach(), CHAIN_LAYERS)
        chain_layerwise(fig, mode, "step %d eval" % step, ts, None, mods, wb)
        for m in mods:
            m.train()
        feats = cuda32(x).requires_grad_(True)
        ts = [tensor_of(feats)]
        for m in mods:
            ts.append(m(ts[-1]))
            ts[-1].features.retain_grad()
        t = ts[-1]
        fig.same(tag, "train out.indices", torch.equal(t.indices.cpu().long(), ind) and t.spatial_shape == SHAPE3)
        fig.add(mode, "step %d train y" % step, t.features, y, A_y.detach(), CHAIN_LAYERS)
        (t.features * cuda32(g_rows)).sum().backward()
    fig.add(mode, "step %d d features" % step, feats.grad, grads[0], A[0], CHAIN_LAYERS)
    for i, m in enumerate(mods):
        fig.add(mode, "step %d d weight %d" % (step, i), m.weight.grad, grads[1 + i], A[1 + i], CHAIN_LAYERS)
        fig.add(mode, "step %d d bias %d" % (step, i), m.bias.grad, grads[6 + i], A[6 + i], CHAIN_LAYERS)
    chain_layerwise(fig, mode, "step %d train" % step, ts, cuda32(g_rows), mods, wb)


def run_chain(label, modes):
    """Step after step on the SAME module instances: new features, new weights copied in place, a new SparseConvTensor over
    the same `indices` tensor; the last step once more on the tensor of the step before (`replace_feature`: its rulebooks,
    their mirrored / inverted tables and the inverse rulebook are the cached ones).  A cache keyed too coarsely -- a filter
    pack, a mirrored table, `_inverse` -- would serve the step before."""
    from dualfusion import spconv
    ind_t = torch.from_numpy(np.array(cloud(3))).cuda()
    mods = chain_modules()
    fig = Figures(label)
    kept = []

    def fresh(feats):
        kept.append(spconv.SparseConvTensor(feats, ind_t, SHAPE3, B3))
        return kept[-1]

    for step, mode in enumerate(modes):
        chain_step(fig, mods, step, mode, fresh)
    chain_step(fig, mods, len(modes), modes[-1], lambda feats: kept[-1].replace_feature(feats))
    fig.close()


@pytest.mark.parametrize("mode", sd.MODES)
def test_chain_two_steps(mode):
    run_chain("chain %s" % mode, [mode, mode])


def test_chain_mode_changes_between_steps():
    run_chain("chain split -> bf16", ["split", "bf16"])


def test_conv_transpose2d_twin_over_steps():
    """SparseConvTranspose2d runs as a cached 3-D twin of itself on a cached lifted tensor: the twin must follow the
    parameters, the lifted tensor the features.  Steps: "split", "bf16" on a new tensor, "fp32" on the SAME tensor object
    with new features."""
    from dualfusion import ops, spconv
    sites = cloud(2)
    ind = torch.from_numpy(np.array(sites)).long()
    ind_t = ind.int().cuda()
    cin, cout, g = 32, 64, geo2(3, 2, 1, 1)
    m = make_module("convT", 2, cin, cout, True, g)
    fn, kw = reference_call("convT", g, sites, SHAPE2)
    fig = Figures("convT2d twin")
    t_in = None
    for step, mode in enumerate(["split", "bf16", "fp32"]):
        name = "convT2d_twin_step%d" % step
        x = sd.gather(field(name + "_x", B2, cin, SHAPE2), ind).requires_grad_(True)
        w, b = weights(name, g["k"], cin, cout, True)
        wr, br = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        ref_coords, ref_shape, y = fn(x, ind, SHAPE2, B2, wr, br, **kw)
        g_rows = sd.gather(field(name + "_g", B2, cout, ref_shape), ref_coords)
        grads = torch.autograd.grad(y, [x, wr, br], g_rows)
        A_y, A_x, A_w, A_b = sd.abs_bound(fn, x, ind, SHAPE2, B2, w, b, grad=g_rows, **kw)
        load(m, w, b)
        with ops.precision(mode):
            m.eval()
            with torch.no_grad():
                out = m(spconv.SparseConvTensor(cuda32(x), ind_t, SHAPE2, B2))
            pos = check_sites(fig, mode, out, ref_coords, ref_shape)
            fig.add(mode, "step %d eval y" % step, out.features, y[pos], A_y[pos])
            m.train()
            feats = cuda32(x).requires_grad_(True)
            if step < 2:
                t_in = spconv.SparseConvTensor(feats, ind_t, SHAPE2, B2)
            else:
                t_in.features = feats
            out = m(t_in)
            pos = check_sites(fig, mode, out, ref_coords, ref_shape)
            fig.add(mode, "step %d train y" % step, out.features, y[pos], A_y[pos])
            (out.features * cuda32(g_rows[pos])).sum().backward()
        fig.add(mode, "step %d d features" % step, feats.grad, grads[0], A_x)
        fig.add(mode, "step %d d weight" % step, m.weight.grad, grads[1], A_w)
        fig.add(mode, "step %d d bias" % step, m.bias.grad, grads[2], A_b)
    fig.close()
