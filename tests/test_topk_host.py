"""df3d_topk_keys without a GPU: the key families of tests/topk_reference.py reach the paths of topk_final_kernel they are
built for (the condition that keeps tests/test_gpu_topk.py honest), the capacity edges fall on both sides of their
comparison, the key range (bits 55:54) does not change the route, the oracle equals the inline sort of the older test, and
the entry refuses bad arguments before any launch."""
import ctypes

import numpy as np
import pytest

import topk_reference as tr

FAMILIES = sorted(tr.TIE_KINDS)
K_TIES = 100                                                   # more than the 37 keys below the tie group: the threshold lies inside it


def test_the_restated_constants_are_those_of_the_source():
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "3d-dual-fusion_amd", "csrc", "topk.hip")).read()
    for name, want in (("TK_BINS", tr.BINS), ("TK_TIE_CAP", tr.TIE_CAP), ("TK_BUF", tr.BUF)):
        assert int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1)) == want
    assert int(re.search(r"TK_MAX_N = (0x[0-9A-Fa-f]+)ll;", src).group(1), 16) == tr.MAX_N
    assert "(key & 0x00FFFFFFFFFFFFFFull) >> %d;" % tr.PREFIX_SHIFT in src and "p > 0xFFFFFFull ? 0xFFFFFFu" in src
    assert "sh = max(18 - 12 * level, 0);" in src and "level = clamp ? -3 : 0; level < 3" in src
    assert [max(18 - 12 * level, 0) for level in range(-3, 3)] == list(tr.CLAMP_SHIFTS + tr.LEVEL_SHIFTS)


@pytest.mark.parametrize("name", FAMILIES)
def test_every_family_takes_the_path_it_is_built_for(name):
    row = tr.family(name)
    assert len(row) % 1024 != 0 and (row == tr.ONES).sum() >= 24
    got = tr.trace(row, K_TIES)
    assert got["path"] == tr.INTENDED[name], got
    assert got["A"] >= 24 and got["P"] > tr.TIE_CAP, got       # keys below the tie group exist; region 1 overflows
    assert tr.trace(row, tr.MAX_K)["path"] == tr.INTENDED[name]


def test_the_families_cover_every_radix_path_and_the_region_sort_is_the_ordinary_case():
    assert {tr.INTENDED[n] for n in FAMILIES} == set(tr.PATHS) - {"region"}
    assert tr.branch(tr.family("ties_l1", tie=1000), K_TIES) == "region"


@pytest.mark.parametrize("name", FAMILIES)
@pytest.mark.parametrize("hi", [1, 3])
def test_the_key_range_does_not_change_the_route(name, hi):
    """bits 55:54 != 0 puts every key into the clamp bin of the 24-bit prefix (A = 0: the keys below the tie group tie with
    it on the clamped prefix); levels -3 .. -1 separate them again, and the exit level is the one of hi = 0"""
    for k in (K_TIES, tr.MAX_K):
        got = tr.trace(tr.family(name, hi), k)
        assert got["path"] == tr.INTENDED[name] and got["A"] == 0, (k, got)


@pytest.mark.parametrize("hi", [0, 1, 3])
def test_capacity_edges_fall_on_both_sides(hi):
    got = {name: tr.trace(row(hi), k) for name, (row, k, _) in tr.EDGES.items()}
    for name, (_, _, want) in tr.EDGES.items():
        assert got[name]["path"] == want, (name, got[name])
    assert got["P_4096"]["P"] == tr.TIE_CAP and got["P_4097"]["P"] == tr.TIE_CAP + 1
    assert got["fill_8192"]["fill"] == tr.BUF and got["fill_8193"]["fill"] == tr.BUF + 1
    assert got["k4096_A4095"]["A"] == (4095 if hi == 0 else 0)
    out, cnt = tr.select(tr.EDGES["k4096_A4095"][0](hi)[None], 4096)
    assert cnt[0] == 4096 and (out[0, 4095] & np.uint64((1 << 30) - 1)) == 0      # the last key is the tie group's first


def test_degenerate_sizes_take_the_region_sort_and_the_oracle_pads():
    rows = tr.small_rows()
    for name in ("k_1", "n_1", "n_below_k", "all_masked"):
        assert tr.branch(*rows[name]) == "region", name
    assert tr.branch(*rows["k_1_ties"]) == "level1"            # k = 1 inside 8972 ties: one key from the radix levels
    out, cnt = tr.select(rows["n_below_k"][0][None], 100)
    assert cnt.tolist() == [45] and (out[0, 45:] == tr.ONES).all() and (out[0, :44] <= out[0, 1:45]).all()
    out, cnt = tr.select(rows["all_masked"][0][None], 60)
    assert cnt.tolist() == [0] and (out == tr.ONES).all()
    out, cnt = tr.select(rows["n_1"][0][None], 5)
    assert cnt.tolist() == [1] and out[0, 0] == rows["n_1"][0][0] and (out[0, 1:] == tr.ONES).all()


def test_select_equals_the_inline_sort_of_the_older_test():
    """every case of test_gpu_nms.test_topk_keys_equals_full_sort, its keys and its expected values, against `select`"""
    import test_gpu_nms as old
    cases = [m for m in old.test_topk_keys_equals_full_sort.pytestmark if m.name == "parametrize"][0].args[1]
    assert len(cases) == 9
    for S, n, k, kind in cases:
        keys = old._score_keys(np.random.RandomState(S * 1000 + k), S, n, kind)
        want = np.sort(keys, axis=1)[:, :k]
        if n < k:
            want = np.concatenate([want, np.full((S, k - n), 0xFFFFFFFFFFFFFFFF, np.uint64)], 1)
        out, cnt = tr.select(keys, k)
        assert np.array_equal(out, want), (S, n, k, kind)
        assert cnt.tolist() == (want != np.uint64(0xFFFFFFFFFFFFFFFF)).sum(1).tolist()


def test_argument_errors_without_a_gpu():
    from dualfusion import _lib
    lib = _lib.bind(ctypes.CDLL(_lib.LIB_PATH), check=False)
    fn, size = lib.df3d_topk_keys, lib.df3d_topk_keys_workspace_bytes
    one = ctypes.c_void_p(16)                                  # a non-null address nobody dereferences: the checks come first
    need = size(2, 100, 10)
    assert need > 0

    def refused(text, *args):
        return fn(*args) == -1 and text in lib.df3d_last_error()
    assert refused(b"0 < K", one, 2, 100, 0, one, None, one, need, None) and size(2, 100, 0) == 0
    assert refused(b"0 < K", one, 2, 100, tr.MAX_K + 1, one, None, one, 1 << 30, None) and size(2, 100, tr.MAX_K + 1) == 0
    assert refused(b"n > 0", one, 2, 0, 10, one, None, one, need, None) and size(2, 0, 10) == 0
    assert refused(b"segments", one, 0, 100, 10, one, None, one, need, None) and size(0, 100, 10) == 0
    assert refused(b"segments", one, 65536, 100, 10, one, None, one, 1 << 40, None)
    assert refused(b"workspace", one, 2, 100, 10, one, None, one, need - 1, None)
    for keys, out, ws in ((None, one, one), (one, None, one), (one, one, None)):
        assert refused(b"null", keys, 2, 100, 10, out, None, ws, need, None)
    # the counters of all four kernels are 32-bit: a segment of 2^31 keys or more is refused, the longest one below is sized
    assert size(1, tr.MAX_N, 10) == size(1, 100, 10) > 0 and size(1, tr.MAX_N + 1, 10) == 0 and size(1, 1 << 40, 10) == 0
    assert refused(b"32-bit counters", one, 1, tr.MAX_N + 1, 10, one, None, one, 1 << 40, None)
