"""tests/conv_f64_reference.py is checked without a GPU: against the numpy loop that test_sparse_conv_split_precision writes out
(agreement to 1e-12 of scale on a 300-row case), and against itself with one deliberate mistake -- a comparison with it can fail:
one neighbour index moved by one row, or two filter taps swapped, is an error above 1e-3 of scale, 250 times the bound of the
two- and three-part kernels."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import conv_f64_reference as cref  # noqa: E402


def _case(cin=32, cout=48, K=27, n_in=260, n_out=300, density=0.5, seed=5):
    gen = torch.Generator().manual_seed(seed)
    nbr = torch.randint(0, n_in, (K, n_out), generator=gen, dtype=torch.int32)
    nbr[torch.rand((K, n_out), generator=gen) >= density] = -1
    nbr[1] = -1                                              # an offset without pairs
    nbr[:, 40:72] = -1                                       # rows without any neighbour
    x = torch.randn((n_in, cin), generator=gen)
    filt = torch.randn((K, cin, cout), generator=gen) * (0.5 / cin ** 0.5)
    bias, shift = torch.randn((cout,), generator=gen) * 0.1, torch.randn((cout,), generator=gen) * 0.1
    scale = 1 + torch.randn((cout,), generator=gen) * 0.1
    res = torch.randn((n_out, cout), generator=gen)
    return x, filt, nbr, n_out, bias, scale, shift, res


def _numpy_loop(x, filt, nbr, n_out, bias, scale, shift, res):
    """test_sparse_conv_split_precision's reference, as written there."""
    feats, filt, nb = x.numpy(), filt.numpy(), nbr.numpy()
    acc = np.zeros((n_out, filt.shape[2]), np.float64)
    for k in range(filt.shape[0]):
        m = nb[k] >= 0
        acc[m] += feats[nb[k][m]].astype(np.float64) @ filt[k].astype(np.float64)
    return acc, np.maximum((acc + bias.numpy()) * scale.numpy() + shift.numpy() + res.numpy(), 0)


def test_reference_equals_the_numpy_loop_on_300_rows():
    x, filt, nbr, n_out, bias, scale, shift, res = _case()
    acc, want = _numpy_loop(x, filt, nbr, n_out, bias, scale, shift, res)
    got = cref.conv_rows_f64(x, filt, nbr, n_out, bias, scale, shift, res, True)
    assert got.dtype == torch.float64 and tuple(got.shape) == want.shape
    assert np.abs(got.numpy() - want).max() <= 1e-12 * np.abs(want).max()
    plain = cref.conv_rows_f64(x, filt, nbr, n_out)
    assert np.abs(plain.numpy() - acc).max() <= 1e-12 * np.abs(acc).max()
    assert torch.equal(plain[40:72], torch.zeros_like(plain[40:72]))                   # rows without a neighbour
    only_bias = cref.conv_rows_f64(x, filt, nbr, n_out, bias=bias, shift=shift)
    assert torch.equal(only_bias[40:72], (bias.double() + shift.double()).expand(32, -1))
    # groups: G convolutions over one table = the per-group calls side by side
    G, cin = 3, 8
    filt_g = torch.stack([filt[:, g * cin:(g + 1) * cin, :16] * (g + 1) for g in range(G)])
    got_g = cref.conv_rows_f64(x, filt_g, nbr, n_out, groups=G, in_group_stride=cin)
    for g in range(G):
        one = cref.conv_rows_f64(x[:, g * cin:(g + 1) * cin], filt_g[g], nbr, n_out)
        assert torch.equal(got_g[:, g * 16:(g + 1) * 16], one)
    shared = cref.conv_rows_f64(x[:, :cin], filt_g, nbr, n_out, groups=G, in_group_stride=0)
    assert torch.equal(shared[:, 16:32], cref.conv_rows_f64(x[:, :cin], filt_g[1], nbr, n_out))


def test_a_comparison_with_the_reference_can_fail():
    x, filt, nbr, n_out, bias, scale, shift, res = _case()
    want = cref.conv_rows_f64(x, filt, nbr, n_out, bias, scale, shift, res, True)
    sc = float(want.abs().max())

    def err(x_=x, filt_=filt, nbr_=nbr):
        return float((cref.conv_rows_f64(x_, filt_, nbr_, n_out, bias, scale, shift, res, True) - want).abs().max()) / sc
    assert err() == 0.0
    moved = nbr.clone()
    k, o = [(k, o) for k in range(27) for o in range(n_out) if nbr[k, o] >= 0 and nbr[k, o] + 1 < x.shape[0]][0]
    moved[k, o] += 1                                         # ONE index, one row further
    assert err(nbr_=moved) > 1e-3
    swapped = filt.clone()
    swapped[[5, 6]] = filt[[6, 5]]                           # two taps of the filter exchanged
    assert err(filt_=swapped) > 1e-3
    dropped = nbr.clone()
    dropped[k, o] = -1                                       # one pair lost
    assert err(nbr_=dropped) > 1e-3
