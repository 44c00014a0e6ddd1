"""The brute-force rulebooks of tests/rulebook_reference.py against the oracle's restatement of the reference's algorithm
(oracle/df3d_oracle.c) and, where oracle/_ref is built, against the reference's own compiled code -- at every geometry the
device tests of tests/test_gpu_rulebook.py use.  The comparison is oracle.canonical_rulebook's order-independent form, and
the output shapes must be the same."""
import numpy as np
import pytest

import rulebook_reference as rb
from oracle import oracle as orc
from oracle import ref

needs_ref = pytest.mark.skipif(not ref.available("sparse_conv_ext"), reason="oracle/_ref not built")
B, SHAPE = rb.SWEEP_BATCH, rb.SWEEP_SHAPE


def voxels():
    return rb.sweep_voxels()


def test_the_inputs_are_what_the_sweep_needs():
    ind = voxels()
    assert 1200 <= len(ind) <= 1500 and len(set(map(tuple, ind.tolist()))) == len(ind)
    flat = ((ind[:, 0].astype(np.int64) * SHAPE[0] + ind[:, 1]) * SHAPE[1] + ind[:, 2]) * SHAPE[2] + ind[:, 3]
    assert (np.diff(flat) < 0).sum() > 100                        # rows are not in flat-index order
    assert ind[:, 3].max() >= 64 and set(ind[:, 0].tolist()) == {0, 1, 2}


def same_rulebook(mine, theirs):
    outids, nbr, out_shape, pairs, num = mine
    t_out, t_pairs, t_num, t_shape = (np.asarray(t) for t in theirs)
    assert list(out_shape) == [int(v) for v in t_shape]
    assert np.array_equal(num, t_num)
    # every output row has a pair (it exists because an input touches it), so the rows their pairs name count their
    # outputs: the reference build returns the output buffer of a transposed rulebook at its full capacity
    t_n_out = max([int(t_pairs[k, 1, :t_num[k]].max()) + 1 for k in range(len(t_num)) if t_num[k]] + [0])
    assert t_n_out == len(outids) <= len(t_out)
    a_ids, a_lists = orc.canonical_rulebook(outids, pairs, num)
    b_ids, b_lists = orc.canonical_rulebook(t_out[:t_n_out], t_pairs, t_num)
    assert np.array_equal(a_ids, b_ids)
    assert len(a_lists) == len(b_lists)
    for x, y in zip(a_lists, b_lists):
        assert np.array_equal(x, y)


def _forward(theirs, ks, st, pd):
    same_rulebook(rb.sweep_rulebook("forward", (ks, st, pd)),
                  theirs(voxels().copy(), B, SHAPE, list(ks), list(st), list(pd), [1, 1, 1], 0))


def _subm(theirs, ks):
    same_rulebook(rb.sweep_rulebook("subm", ks),
                  theirs(voxels().copy(), B, SHAPE, list(ks), [1, 1, 1], [k // 2 for k in ks], [1, 1, 1], 1))


def _transposed(theirs, ks, st, pd, op, dl):
    same_rulebook(rb.sweep_rulebook("transposed", (ks, st, pd, op, dl)),
                  theirs(voxels().copy(), B, SHAPE, list(ks), list(st), list(pd), list(dl), list(op)))


@pytest.mark.parametrize("ks,st,pd", rb.FORWARD, ids=[rb.tag(g) for g in rb.FORWARD])
def test_forward_equals_the_oracle(ks, st, pd):
    _forward(orc.get_indice_pairs, ks, st, pd)


@pytest.mark.parametrize("ks", rb.SUBM, ids=[rb.tag(g) for g in rb.SUBM])
def test_submanifold_equals_the_oracle(ks):
    _subm(orc.get_indice_pairs, ks)


@pytest.mark.parametrize("ks,st,pd,op,dl", rb.TRANSPOSED, ids=[rb.tag(g) for g in rb.TRANSPOSED])
def test_transposed_equals_the_oracle(ks, st, pd, op, dl):
    _transposed(orc.get_indice_pairs_transpose, ks, st, pd, op, dl)


@needs_ref
def test_every_geometry_equals_the_reference_build():
    for ks, st, pd in rb.FORWARD:
        _forward(ref.get_indice_pairs, ks, st, pd)
    for ks in rb.SUBM:
        _subm(ref.get_indice_pairs, ks)
    for g in rb.TRANSPOSED:
        _transposed(ref.get_indice_pairs_transpose, *g)


def test_derived_forms_on_a_hand_made_case():
    """two voxels in a row, kernel (1, 1, 3): the table, the pairs, the inverse and the float64 sums by hand"""
    ind = np.asarray([[0, 0, 0, 1], [0, 0, 0, 0]], dtype=np.int32)
    outids, nbr, shape = rb.submanifold(ind, [1, 1, 2], (1, 1, 3))
    assert nbr.tolist() == [[1, -1], [0, 1], [-1, 0]] and shape == [1, 1, 2] and np.array_equal(outids, ind)
    pairs, num = rb.pairs_of(nbr, 2)
    assert num.tolist() == [1, 2, 1] and pairs.tolist() == [[[1, -1], [0, -1]], [[0, 1], [0, 1]], [[0, -1], [1, -1]]]
    assert rb.inverse_of(nbr, 2).tolist() == [[-1, 0], [0, 1], [1, -1]]
    x, w, g = np.asarray([[2.0], [3.0]]), np.asarray([[[5.0]], [[7.0]], [[11.0]]]), np.asarray([[1.0], [10.0]])
    assert rb.conv(x, w, nbr).tolist() == [[3 * 5 + 2 * 7.0], [3 * 7 + 2 * 11.0]]
    assert rb.conv_input_grad(g, w, nbr, 2).tolist() == [[7 * 1 + 11 * 10.0], [5 * 1 + 7 * 10.0]]
    assert rb.conv_filter_grad(x, g, nbr).tolist() == [[[3 * 1.0]], [[2 * 1 + 3 * 10.0]], [[2 * 10.0]]]
    # forward (1, 1, 2) stride 2 and its transposed twin
    o, n, s = rb.forward(ind, [1, 1, 2], (1, 1, 2), (1, 1, 2), (0, 0, 0))
    assert o.tolist() == [[0, 0, 0, 0]] and n.tolist() == [[1], [0]] and s == [1, 1, 1]
    o, n, s = rb.transposed(ind[:1], [1, 1, 2], (1, 1, 2), (1, 1, 2), (0, 0, 0))
    assert o.tolist() == [[0, 0, 0, 2], [0, 0, 0, 3]] and n.tolist() == [[0, -1], [-1, 0]] and s == [1, 1, 4]
