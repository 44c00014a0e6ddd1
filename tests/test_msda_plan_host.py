"""Which kernels the MSDA backward runs for a shape is pinned without a GPU: df3d_ms_deform_attn_backward_plan (the choice
function of csrc/msda.hip) and `ops.msda_backward_plan` on top of it.  The atomic, the binned and the ordered value gradient
agree to 2e-5, so a shape that silently fell back to the atomic kernels would pass every numerical test."""
import ctypes
import os

import pytest

DEFAULT, ATOMIC, SORTED = 0, 1, 2                      # the C function's modes
P_ATOMIC, P_BINNED, P_SORTED, P_REFUSED = 0, 1, 2, -1  # ... and its answers
NAMES = {P_ATOMIC: "atomic", P_BINNED: "binned", P_SORTED: "sorted"}
COMMON = [(13, 17), (7, 9), (4, 5), (2, 3)]


def _lib():
    import __graft_entry__ as ge
    ge._load(os.path.join(ge.PKG, "csrc", "build.py"), "df3d_build").build()
    from dualfusion import _lib
    return _lib.bind(ctypes.CDLL(_lib.LIB_PATH), check=False)


class _Env(object):
    """`with _Env(name, value):` -- the variable set (None: unset) inside, restored on the way out."""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = os.environ.get(self.name)
        os.environ.pop(self.name, None)
        if self.value is not None:
            os.environ[self.name] = self.value

    def __exit__(self, *exc):
        os.environ.pop(self.name, None)
        if self.old is not None:
            os.environ[self.name] = self.old
        return False


def _starts(maps):
    out, run = [], 0
    for h, w in maps:
        out.append(run)
        run += h * w
    return out, run


def _i64(values):
    return (ctypes.c_int64 * len(values))(*values)


def _case(maps, M, D, P, Lq=300, N=2, S=None, starts=None):
    st, pixels = _starts(maps)
    return dict(N=N, S=pixels if S is None else S, M=M, D=D, Lq=Lq, L=len(maps), P=P, maps=list(maps),
                starts=st if starts is None else starts)


def _plan(c, mode):
    hw = _i64([v for m in c["maps"] for v in m])
    st = _i64(c["starts"])
    return int(_lib().df3d_ms_deform_attn_backward_plan(c["N"], c["S"], c["M"], c["D"], c["Lq"], c["L"], c["P"],
                                                        ctypes.cast(hw, ctypes.c_void_p), ctypes.cast(st, ctypes.c_void_p), mode))


# (name, case, default-mode answer, sorted-mode answer, a word the refusal must carry)
CASES = [
    ("L1_D16", _case([(37, 61)], 8, 16, 4), P_BINNED, P_SORTED, None),
    ("L4_P4_D32", _case(COMMON, 8, 32, 4), P_BINNED, P_SORTED, None),
    ("L2_D64", _case([(9, 8), (17, 33)], 4, 64, 2), P_BINNED, P_SORTED, None),
    ("D8", _case([(37, 61)], 8, 8, 4), P_ATOMIC, P_REFUSED, "D = 8"),
    ("D2", _case([(37, 61)], 8, 2, 4), P_ATOMIC, P_REFUSED, "D = 2"),
    ("LP20", _case(COMMON + [(1, 1)], 8, 16, 4), P_ATOMIC, P_REFUSED, "L * P"),
    # 7680 tiles of the first level + the one tile of the second, one head: 7681 bins (7681 is prime)
    ("bins7681", _case([(8, 8 * 7680), (1, 1)], 1, 16, 4), P_ATOMIC, P_REFUSED, "7680"),
    ("S_larger", _case(COMMON, 8, 32, 4, S=_starts(COMMON)[1] + 1), P_ATOMIC, P_REFUSED, "S ="),
    ("start_gap", _case(COMMON, 8, 32, 4, S=_starts(COMMON)[1] + 3, starts=[0, 221, 221 + 63 + 3, 221 + 63 + 3 + 20]), P_ATOMIC,
     P_REFUSED, "level_start_index[2]"),
]


@pytest.mark.parametrize("name,case,default,ordered,word", CASES, ids=[c[0] for c in CASES])
def test_plan_function_over_the_envelope(name, case, default, ordered, word):
    lib = _lib()
    assert _plan(case, DEFAULT) == default
    assert _plan(case, SORTED) == ordered
    if ordered == P_REFUSED:
        assert word in lib.df3d_last_error().decode(), lib.df3d_last_error()     # reported, never silent: the limit is named
    assert _plan(case, ATOMIC) == P_ATOMIC


def test_the_last_bin_that_fits_is_served():
    """7680 bins exactly (the scan kernel's 1024 x 8 and the 61 KB histogram) are inside the envelope."""
    assert _plan(_case([(8, 8 * 7679), (1, 1)], 1, 16, 4), DEFAULT) == P_BINNED
    assert _plan(_case([(8, 8 * 960)], 8, 16, 4), SORTED) == P_SORTED


def test_workspace_and_slab_bytes_are_positive_and_monotone():
    lib = _lib()
    hw = _i64([v for m in COMMON for v in m])
    p = ctypes.cast(hw, ctypes.c_void_p)
    N, M, L, P = 2, 8, 4, 4
    for ordered in (0, 1):
        ws = [int(lib.df3d_ms_deform_attn_backward_binned_ml_workspace_bytes(N, M, lq, L, P, p, ordered)) for lq in (1, 300, 10000)]
        assert ws[0] > 0 and ws[0] <= ws[1] < ws[2], ws
    plain = int(lib.df3d_ms_deform_attn_backward_binned_ml_workspace_bytes(N, M, 300, L, P, p, 0))
    assert int(lib.df3d_ms_deform_attn_backward_binned_ml_workspace_bytes(N, M, 300, L, P, p, 1)) > plain   # the ordered copy
    by_d = [int(lib.df3d_ms_deform_attn_backward_binned_ml_slab_bytes(N, M, d, 300, L, P, p)) for d in (16, 32, 64)]
    assert by_d[0] > 0 and by_d[0] < by_d[1] < by_d[2], by_d
    by_lq = [int(lib.df3d_ms_deform_attn_backward_binned_ml_slab_bytes(N, M, 32, lq, L, P, p)) for lq in (1, 300, 10000)]
    assert by_lq[0] > 0 and by_lq[0] <= by_lq[1] < by_lq[2], by_lq
    # one level, 16 channels: the same work items as the single-level entry, so the same slab
    one = _i64([37, 61])
    assert int(lib.df3d_ms_deform_attn_backward_binned_ml_slab_bytes(3, 8, 16, 700, 1, 4, ctypes.cast(one, ctypes.c_void_p))) == \
        int(lib.df3d_ms_deform_attn_backward_binned_slab_bytes(3, 8, 16, 700, 4, 37, 61))


# (N, M, Lq, P, H, W): an odd map, a one-tile map, a map smaller than a tile with 16 points, the TransFusion training shape
SINGLE_LEVEL = [(3, 8, 700, 4, 37, 61), (2, 4, 300, 4, 8, 8), (1, 1, 40, 16, 3, 2), (24, 8, 10000, 4, 112, 200)]


@pytest.mark.parametrize("N,M,Lq,P,H,W", SINGLE_LEVEL)
def test_single_level_entry_asks_for_the_bytes_of_the_general_one(N, M, Lq, P, H, W):
    """df3d_ms_deform_attn_backward_binned forwards to the implementation behind ..._binned_ml with L = 1, ordered = 0: its two
    size functions return what the general ones return for that shape."""
    lib = _lib()
    one = ctypes.cast(_i64([H, W]), ctypes.c_void_p)
    ws = int(lib.df3d_ms_deform_attn_backward_binned_workspace_bytes(N, M, Lq, P, H, W))
    slab = int(lib.df3d_ms_deform_attn_backward_binned_slab_bytes(N, M, 16, Lq, P, H, W))
    assert ws > 0 and ws == int(lib.df3d_ms_deform_attn_backward_binned_ml_workspace_bytes(N, M, Lq, 1, P, one, 0))
    assert slab > 0 and slab == int(lib.df3d_ms_deform_attn_backward_binned_ml_slab_bytes(N, M, 16, Lq, 1, P, one))


def _single_level_call(N=2, M=8, D=16, Lq=300, P=4, H=37, W=61):
    """df3d_ms_deform_attn_backward_binned with null tensors: only what it decides before it touches the device."""
    lib = _lib()
    rc = int(lib.df3d_ms_deform_attn_backward_binned(*([None] * 6 + [N, M, D, Lq, P, H, W] + [None] * 4 + [0, None, None])))
    return rc, lib.df3d_last_error().decode()


@pytest.mark.parametrize("change,text", [
    (dict(D=32), "ms_deform_attn_backward_binned: head width 32 / 4 points not served"),
    (dict(P=17), "ms_deform_attn_backward_binned: head width 16 / 17 points not served"),
    (dict(H=248, W=248), "ms_deform_attn_backward_binned: 961 tiles x 8 heads exceed the LDS budget"),   # 7688 bins > 7680
    (dict(N=65536), "ms_deform_attn_backward_binned: 65536 maps x 300 queries"),
    (dict(), "ms_deform_attn_backward_binned: null argument"),
], ids=["D32", "P17", "bins7688", "N65536", "null"])
def test_single_level_entry_keeps_its_own_refusals(change, text):
    rc, err = _single_level_call(**change)
    assert rc != 0 and err == text, (rc, err)


def test_single_level_entry_returns_ok_for_no_maps():
    assert _single_level_call(N=0)[0] == 0                                         # DF3D_OK, before any argument is read


def test_python_plan_agrees_with_the_library_under_the_switch():
    import torch
    from dualfusion import _lib as L, ops
    assert not torch.are_deterministic_algorithms_enabled()
    saved = os.environ.get("DF3D_MSDA_BWD")
    for name, c, default, ordered, word in CASES:
        args = (c["N"], c["S"], c["M"], c["D"], c["Lq"], c["L"], c["P"], c["maps"], c["starts"])
        for env, mode in ((None, DEFAULT), ("binned", DEFAULT), ("atomic", ATOMIC), ("sorted", SORTED)):
            with _Env("DF3D_MSDA_BWD", env):
                want = _plan(c, mode)
                if want == P_REFUSED:
                    with pytest.raises(L.Df3dError) as e:
                        ops.msda_backward_plan(*args)
                    assert word in str(e.value)
                else:
                    assert ops.msda_backward_plan(*args) == NAMES[want], (name, env)
        with _Env("DF3D_MSDA_BWD", "atomic"):                                      # an explicit mode wins over the variable
            assert ops.msda_backward_plan(*args, mode="binned") == NAMES[default]
    assert os.environ.get("DF3D_MSDA_BWD") == saved                                # restored
    with _Env("DF3D_MSDA_BWD", None):
        assert ops.msda_backward_mode() == "binned"
    with _Env("DF3D_MSDA_BWD", "fastest"):
        with pytest.raises(L.Df3dError):
            ops.msda_backward_mode()


def test_deterministic_algorithms_select_the_ordered_path():
    import warnings
    import torch
    from dualfusion import _lib as L, ops
    served, refused = CASES[1][1], CASES[3][1]
    a = lambda c: (c["N"], c["S"], c["M"], c["D"], c["Lq"], c["L"], c["P"], c["maps"], c["starts"])
    with _Env("DF3D_MSDA_BWD", None):
        try:
            torch.use_deterministic_algorithms(True)
            assert ops.msda_backward_mode() == "sorted" and ops.msda_backward_plan(*a(served)) == "sorted"
            with pytest.raises(L.Df3dError):
                ops.msda_backward_plan(*a(refused))
            torch.use_deterministic_algorithms(True, warn_only=True)
            ops._msda_bwd_warned = False
            with warnings.catch_warnings(record=True) as seen:
                warnings.simplefilter("always")
                assert ops.msda_backward_plan(*a(refused)) == "atomic"
                assert ops.msda_backward_plan(*a(refused)) == "atomic"
            assert len([w for w in seen if "D = 8" in str(w.message)]) == 1      # warned once
        finally:
            torch.use_deterministic_algorithms(False)
        with _Env("DF3D_MSDA_BWD", "binned"):                                      # the variable, when set, decides
            torch.use_deterministic_algorithms(True)
            try:
                assert ops.msda_backward_mode() == "binned"
            finally:
                torch.use_deterministic_algorithms(False)
