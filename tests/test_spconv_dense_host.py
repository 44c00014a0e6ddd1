"""The dense float64 reference of tests/spconv_dense_reference.py, validated on the host before any device test leans on it:

a. against the committed goldens of the reference's compiled CPU code -- transposed convolution values and output sets,
   the convolution backward, the inverse convolution and the max pool with its gradient -- to the suite's fp32 grade, 5e-6 of
   max |golden| (test_sparse_conv_split_precision; the goldens are fp32 sums, measured 1e-7 .. 6e-7), identical active sets;
b. against the brute-force rulebooks of tests/rulebook_reference.py at every geometry of FORWARD, SUBM and TRANSPOSED:
   the same active set, and forward, d x and d w to 1e-12 relative (both sides are float64)."""
import numpy as np
import pytest

import detgen
import rulebook_reference as rb
import spconv_dense_reference as sd
from make_golden import CONV_BWD_BATCH, CONV_BWD_SHAPE, CONVT_CASES, conv_bwd_case, convt_case

torch = pytest.importorskip("torch")

FP32_GRADE = 5e-6
F64 = torch.float64


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(F64)


def rel(got, want):
    want = np.asarray(want, np.float64)
    return float(np.abs(got.detach().numpy() - want).max() / np.abs(want).max())


# ------------------------------------------------------------------------------------------------------- a. goldens
@pytest.mark.parametrize("tag,ks,st,pd,op", CONVT_CASES, ids=[c[0] for c in CONVT_CASES])
def test_conv_transpose_golden(golden, tag, ks, st, pd, op):
    g = golden("conv_transpose.npz")
    ind, f = convt_case()
    w = detgen.randn("convt_w_" + tag, tuple(ks) + (16, 16), 0.2)
    coords, out_shape, y = sd.conv_transpose(t64(f), ind, CONV_BWD_SHAPE, CONV_BWD_BATCH, t64(w), None, st, pd, op)
    assert out_shape == list(g["oshape_" + tag])
    assert np.array_equal(coords.numpy(), g["outids_" + tag])            # both in ascending (b, z, y, x) order
    err = rel(y, g["y_" + tag])
    print("conv_transpose %s: %.2e of max |golden|" % (tag, err))
    assert err <= FP32_GRADE


@pytest.mark.parametrize("subm", [1, 0])
def test_conv_backward_golden(golden, subm):
    g = golden("conv_bwd.npz")
    ind, ks, st, pd, f, w = conv_bwd_case(subm)
    x, wt = t64(f).requires_grad_(True), t64(w).requires_grad_(True)
    if subm:
        coords, out_shape, y = sd.subm(x, ind, CONV_BWD_SHAPE, CONV_BWD_BATCH, wt)
    else:
        coords, out_shape, y = sd.conv(x, ind, CONV_BWD_SHAPE, CONV_BWD_BATCH, wt, None, st, pd)
    ref_ids = g["outids_%d" % subm]
    assert sd.same_set(coords, ref_ids, out_shape) and len(coords) == len(ref_ids)
    # the golden's out-gradient rows are in the reference's own row order; `order` sorts them onto ref_ids
    go = detgen.randn("bwd_g%d" % subm, (len(ref_ids), 20))[g["order_%d" % subm]]
    (y * t64(go)[sd.rows_at(ref_ids, out_shape, coords)]).sum().backward()
    e_gi, e_gw = rel(x.grad, g["gi_%d" % subm]), rel(wt.grad, g["gw_%d" % subm])
    print("conv_bwd subm=%d: gi %.2e gw %.2e of max |golden|" % (subm, e_gi, e_gw))
    assert e_gi <= FP32_GRADE and e_gw <= FP32_GRADE


def test_inverse_conv_golden(golden):
    g = golden("pool.npz")
    ind, ks, st, pd, f, w = conv_bwd_case(0)
    mid, mid_shape = sd.occupancy(ind, CONV_BWD_SHAPE, CONV_BWD_BATCH, ks, st, pd)
    assert np.array_equal(mid.numpy(), g["outids"])
    fo = detgen.randn("inv_f", (len(mid), 20))[g["order"]]               # rows on the strided conv's output sites, sorted
    wi = detgen.randn("inv_w", (3, 3, 3, 20, 12), 0.2)
    coords, shape, y = sd.inverse(t64(fo), mid, mid_shape, CONV_BWD_BATCH, t64(wi), None, ind, CONV_BWD_SHAPE, st, pd)
    assert shape == CONV_BWD_SHAPE and np.array_equal(coords.numpy(), ind)
    err = rel(y, g["inv"])
    print("inverse conv: %.2e of max |golden|" % err)
    assert err <= FP32_GRADE


def test_maxpool_golden(golden):
    g = golden("pool.npz")
    ind, ks, st, pd, f, _ = conv_bwd_case(0)
    x = t64(f).requires_grad_(True)
    coords, out_shape, y = sd.maxpool(x, ind, CONV_BWD_SHAPE, CONV_BWD_BATCH, ks, st, pd)
    assert out_shape == [4, 10, 11] and np.array_equal(coords.numpy(), g["outids"])
    assert np.array_equal(y.detach().numpy().astype(np.float32), g["y"][g["order"]])
    go = detgen.randn("pool_g", tuple(y.shape))[g["order"]]
    (y * t64(go)).sum().backward()
    # random normals have no ties inside a window, so torch's single winner is the reference's fan-out; the reference adds
    # fp32 gradients, so this one is held to an absolute bound at the scale of its values
    err = float(np.abs(x.grad.numpy() - g["gin"]).max())
    print("max pool gradient: %.2e absolute (max |golden| %.2f)" % (err, np.abs(g["gin"]).max()))
    assert err <= FP32_GRADE * np.abs(g["gin"]).max()


# --------------------------------------------------------------------------------------- b. brute-force rulebooks
SWEEP = [("forward", g) for g in rb.FORWARD] + [("subm", g) for g in rb.SUBM] + [("transposed", g) for g in rb.TRANSPOSED]
C = 8


@pytest.mark.parametrize("kind,geometry", SWEEP, ids=["%s-%s" % (k, rb.tag(g)) for k, g in SWEEP])
def test_dense_equals_brute_force_rulebook(kind, geometry):
    ind = rb.sweep_voxels()
    outids, nbr, out_shape = rb.sweep_rulebook(kind, geometry)[:3]
    ks = geometry if kind == "subm" else geometry[0]
    name = "dense_host_%s_%s" % (kind, rb.tag(geometry))
    x = t64(detgen.randn(name + "_x", (len(ind), C))).requires_grad_(True)
    w = t64(detgen.randn(name + "_w", tuple(ks) + (C, C))).requires_grad_(True)
    go = t64(detgen.randn(name + "_g", (len(outids), C)))
    if kind == "forward":
        coords, shape, y = sd.conv(x, ind, rb.SWEEP_SHAPE, rb.SWEEP_BATCH, w, None, geometry[1], geometry[2])
    elif kind == "subm":
        coords, shape, y = sd.subm(x, ind, rb.SWEEP_SHAPE, rb.SWEEP_BATCH, w)
    else:
        coords, shape, y = sd.conv_transpose(x, ind, rb.SWEEP_SHAPE, rb.SWEEP_BATCH, w, None, *geometry[1:])
    assert tuple(shape) == tuple(out_shape)
    assert not sd.has_duplicates(coords, shape) and sd.same_set(coords, outids, shape)
    assert np.array_equal(coords.numpy(), outids)            # (and in the brute-force table's row order, so rows compare as they are)
    (y * go).sum().backward()
    filters = w.detach().numpy().reshape(-1, C, C)
    for got, want, what in ((y, rb.conv(x.detach().numpy(), filters, nbr), "y"),
                            (x.grad, rb.conv_input_grad(go.numpy(), filters, nbr, len(ind)), "d x"),
                            (w.grad.reshape(-1, C, C), rb.conv_filter_grad(x.detach().numpy(), go.numpy(), nbr), "d w")):
        assert rel(got, want) <= 1e-12, (what, rel(got, want))
