"""The MSDA value gradient without global atomics beyond the single-level, 16-channel shape (df3d_ms_deform_attn_backward_binned_ml:
bins of (level, tile, head), heads of 16 / 32 / 64 channels) and its ordered form (DF3D_MSDA_BWD=sorted: the points of a bin
summed in ascending id order, so grad_value is a function of the inputs alone), against the atomic kernels and the oracle's
col2im.  Inputs as in test_msda_backward_binned_against_the_atomic_kernel_and_the_oracle (tests/test_gpu_ops.py): the last third
of the queries on reference point (0, 0), the last sixth of the upstream rows zero, locations = reference + 0.03 randn, softmax
weights over L * P.  Bounds: 2e-5 of scale against the atomic kernel (summation order), 1e-4 against the oracle -- the
project's own, from that test."""
import os

import numpy as np
import pytest

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# (N, Lq, M, D, P, maps)
CASES = [
    (2, 64, 2, 16, 2, [(5, 19), (3, 2)]),                          # two levels, one smaller than a tile
    (2, 300, 8, 32, 4, [(13, 17), (7, 9), (4, 5), (2, 3)]),        # the common 4 x 4 configuration; bins of 1000 points
    (1, 40, 1, 64, 16, [(3, 2)]),                                  # 528 points in the single bin, L * P = 16
    (3, 1600, 8, 32, 4, [(37, 61)]),                               # map not a multiple of the tile, wide head, one level
    (2, 900, 4, 16, 2, [(9, 8), (17, 33)]),                        # largest bin 1223 points
    # one tile, one head: a bin of 14839 points (counted on the CPU) and 320 000 possible ids = two windows of the ordered
    # pass's bit directory (14566 + 273 points); the cases above end in its one-wave ranking and its LDS network (<= 1024 ids)
    (1, 20000, 1, 16, 1, [(8, 8)]),
]
IDS = ["L2_D16_tiny", "L4_P4_D32", "L1_D64_LP16", "L1_D32_37x61", "L2_D16_bin1223", "L1_D16_bin14839"]
NAMES = ("value", "loc", "weight")
ENTRIES = ("df3d_ms_deform_attn_backward", "df3d_ms_deform_attn_backward_binned", "df3d_ms_deform_attn_backward_binned_ml")


class _Env(object):
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get("DF3D_MSDA_BWD")
        os.environ.pop("DF3D_MSDA_BWD", None)
        if self.value is not None:
            os.environ["DF3D_MSDA_BWD"] = self.value

    def __exit__(self, *exc):
        os.environ.pop("DF3D_MSDA_BWD", None)
        if self.old is not None:
            os.environ["DF3D_MSDA_BWD"] = self.old
        return False


class _Spy(object):
    """Which of the library's three backward entries a call went through."""

    def __enter__(self):
        from dualfusion import _lib
        self.lib, self.real, self.seen = _lib.load(), {}, []
        for name in ENTRIES:
            fn = self.real[name] = getattr(self.lib, name)
            setattr(self.lib, name, (lambda *a, _fn=fn, _n=name: (self.seen.append(_n), _fn(*a))[1]))
        return self

    def __exit__(self, *exc):
        for name, fn in self.real.items():
            setattr(self.lib, name, fn)
        return False


def _starts(maps):
    out, run = [], 0
    for h, w in maps:
        out.append(run)
        run += h * w
    return out, run


def _inputs(N, Lq, M, D, P, maps):
    L = len(maps)
    starts, S = _starts(maps)
    gen = torch.Generator().manual_seed(N * 1000 + Lq)
    value = torch.randn(N, S, M, D, generator=gen)
    ref = torch.rand(N, Lq, 1, 1, 1, 2, generator=gen) * 1.2 - 0.1
    ref[:, Lq * 2 // 3:] = 0.0
    loc = (ref + torch.randn(N, Lq, M, L, P, 2, generator=gen) * 0.03).contiguous()
    aw = torch.softmax(torch.randn(N, Lq, M, L * P, generator=gen), -1).view(N, Lq, M, L, P).contiguous()
    go = torch.randn(N, Lq, M * D, generator=gen)
    go[:, Lq * 5 // 6:] = 0.0
    return value, loc, aw, go, starts, S


def _run(dev, maps, starts, value, loc, aw, go, mode):
    from dualfusion import ops
    shp = torch.tensor(maps, dtype=torch.long, device=dev)
    ls = torch.tensor(starts, dtype=torch.long, device=dev)
    with _Env(mode), _Spy() as spy:
        out = [t.cpu() for t in ops.ms_deform_attn_backward(value.to(dev), shp, ls, loc.to(dev), aw.to(dev), go.to(dev))]
    assert len(spy.seen) == 1, spy.seen
    return out, spy.seen[0]


_SHARED = {}


def _shared(i):
    """The case's inputs, its oracle gradients and the atomic kernel's: computed once, read by both tests of the case."""
    if i not in _SHARED:
        N, Lq, M, D, P, maps = CASES[i]
        value, loc, aw, go, starts, S = _inputs(*CASES[i])
        want = orc.ms_deform_attn_backward(value.numpy(), maps, loc.numpy(), aw.numpy(), go.numpy())
        atomic, entry = _run(torch.device("cuda:0"), maps, starts, value, loc, aw, go, "atomic")
        assert entry == "df3d_ms_deform_attn_backward"
        _SHARED[i] = (value, loc, aw, go, starts, S, want, atomic)
    return _SHARED[i]


def _assert_close(got, atomic, want):
    for a, b, w, name in zip(got, atomic, want, NAMES):
        scale = max(1.0, float(np.abs(w).max()))
        d_atomic, d_oracle = float((a - b).abs().max()), float(np.abs(a.numpy() - w).max())
        print("%s: |binned - atomic| %.3e (bound %.3e), |binned - oracle| %.3e (bound %.3e)" % (name, d_atomic, 2e-5 * scale,
                                                                                                 d_oracle, 1e-4 * scale))
        assert d_atomic <= 2e-5 * scale, name                                      # (summation order of the atomics)
        assert d_oracle <= 1e-4 * scale, name


def _assert_no_overflow():
    from dualfusion import ops
    hit, where = ops.split_overflow()
    assert not hit, where


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_binned_value_gradient_for_levels_and_wide_heads(dev, i):
    from dualfusion import ops
    N, Lq, M, D, P, maps = CASES[i]
    value, loc, aw, go, starts, S, want, atomic = _shared(i)
    with _Env(None):
        assert ops.msda_backward_plan(N, S, M, D, Lq, len(maps), P, maps, starts) == "binned"
    got, entry = _run(dev, maps, starts, value, loc, aw, go, None)
    # (no silent fallback to the atomic kernels; one level of 16-channel heads keeps the single-level entry)
    assert entry == ("df3d_ms_deform_attn_backward_binned" if len(maps) == 1 and D == 16 else "df3d_ms_deform_attn_backward_binned_ml")
    _assert_close(got, atomic, want)
    assert torch.equal(got[1], atomic[1]) and torch.equal(got[2], atomic[2])       # the gather half is the same code
    _assert_no_overflow()


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_ordered_value_gradient_is_a_function_of_the_inputs(dev, i):
    from dualfusion import ops
    N, Lq, M, D, P, maps = CASES[i]
    L = len(maps)
    value, loc, aw, go, starts, S, want, atomic = _shared(i)
    with _Env("sorted"):
        assert ops.msda_backward_plan(N, S, M, D, Lq, L, P, maps, starts) == "sorted"
    got, entry = _run(dev, maps, starts, value, loc, aw, go, "sorted")
    assert entry == "df3d_ms_deform_attn_backward_binned_ml", entry
    _assert_close(got, atomic, want)
    again, _ = _run(dev, maps, starts, value, loc, aw, go, "sorted")
    for a, b, name in zip(got, again, NAMES):
        assert torch.equal(a, b), name                                             # two calls: the same bits
    # three identical maps: three identical slices, whichever workgroups served them
    rep = [t[:1].repeat(3, *([1] * (t.dim() - 1))).contiguous() for t in (value, loc, aw, go)]
    same, _ = _run(dev, maps, starts, rep[0], rep[1], rep[2], rep[3], "sorted")
    assert torch.equal(same[0][0], same[0][1]) and torch.equal(same[0][0], same[0][2])
    assert torch.equal(same[0][0], got[0][0])
    # 100 dead queries in front: every live id, workgroup and atomic race shifts; the live ids' order and the 512-point
    # work items do not
    gen = torch.Generator().manual_seed(7)
    loc2 = torch.cat([torch.rand(N, 100, M, L, P, 2, generator=gen) * 1.2 - 0.1, loc], 1).contiguous()
    aw2 = torch.cat([torch.softmax(torch.randn(N, 100, M, L * P, generator=gen), -1).view(N, 100, M, L, P), aw], 1).contiguous()
    go2 = torch.cat([torch.zeros(N, 100, M * D), go], 1).contiguous()
    shifted, _ = _run(dev, maps, starts, value, loc2, aw2, go2, "sorted")
    assert torch.equal(shifted[0], got[0])
    _assert_no_overflow()


def test_ordered_mode_reports_a_shape_outside_the_envelope(dev):
    """Reported, never silent: heads of 8 channels have no binned path, so the ordered mode raises and names the limit."""
    from dualfusion import _lib
    value, loc, aw, go, starts, S = _inputs(1, 16, 2, 8, 2, [(5, 7)])
    with pytest.raises(_lib.Df3dError) as e:
        _run(dev, [(5, 7)], starts, value, loc, aw, go, "sorted")
    assert "D = 8" in str(e.value), e.value
    got, entry = _run(dev, [(5, 7)], starts, value, loc, aw, go, None)            # default mode: the atomic kernels, as before
    assert entry == "df3d_ms_deform_attn_backward"
    _assert_no_overflow()


def test_module_path_reaches_the_binned_kernels(dev):
    """MSDeformAttnFunction.apply(...).backward at the L = 4, D = 32 case: the autograd shell hands over the same gradients."""
    from dualfusion.msda import MSDeformAttnFunction
    N, Lq, M, D, P, maps = CASES[1]
    value, loc, aw, go, starts, S, want, atomic = _shared(1)
    direct, _ = _run(dev, maps, starts, value, loc, aw, go, "sorted")
    leaves = [t.to(dev).requires_grad_(True) for t in (value, loc, aw)]
    shp = torch.tensor(maps, dtype=torch.long, device=dev)
    ls = torch.tensor(starts, dtype=torch.long, device=dev)
    with _Env("sorted"), _Spy() as spy:
        out = MSDeformAttnFunction.apply(leaves[0], shp, ls, leaves[1], leaves[2], 64)
        out.backward(go.to(dev))
    assert spy.seen == ["df3d_ms_deform_attn_backward_binned_ml"], spy.seen
    for leaf, ref, name in zip(leaves, direct, NAMES):
        assert torch.equal(leaf.grad.cpu(), ref), name
    _assert_close([t.grad.cpu() for t in leaves], atomic, want)
    _assert_no_overflow()


# (N, Lq, M, P, H, W), D = 16: a map of one tile row, a map smaller than a tile with 16 points, and two tile rows x three tile
# columns whose last tile is one pixel wide and one pixel high
FORWARDED = [(2, 64, 2, 2, 5, 19), (1, 40, 1, 16, 3, 2), (2, 300, 4, 4, 9, 17)]


@pytest.mark.parametrize("N,Lq,M,P,H,W", FORWARDED, ids=["5x19", "3x2_P16", "9x17"])
def test_single_level_entry_is_the_general_entry_with_one_level(dev, N, Lq, M, P, H, W):
    """df3d_ms_deform_attn_backward_binned forwards to the implementation of ..._binned_ml with level_hw = {H, W}, level_start = {0},
    L = 1, ordered = 0.  Both entries through ctypes on the same operands: the same workspace and slab sizes, the location / weight
    gradients bit for bit (the same kernel), grad_value within the bound of a changed summation order, against both modes of the
    general entry.  A forwarder that swaps H and W, mis-sets level_start or hands over a wrong point count fails here."""
    from dualfusion import _lib, ops
    lib, D = _lib.load(), 16
    value, loc, aw, go, starts, S = _inputs(N, Lq, M, D, P, [(H, W)])
    value, loc, aw, go = [t.to(dev) for t in (value, loc, aw, go)]
    shp = torch.tensor([(H, W)], dtype=torch.long, device=dev)
    ls = torch.zeros((1,), dtype=torch.long, device=dev)
    hw, keep_hw = ops._i64_arr([H, W])
    st, keep_st = ops._i64_arr([0])
    nslab = int(lib.df3d_ms_deform_attn_backward_binned_slab_bytes(N, M, D, Lq, P, H, W))
    assert nslab == int(lib.df3d_ms_deform_attn_backward_binned_ml_slab_bytes(N, M, D, Lq, 1, P, hw))
    nws = int(lib.df3d_ms_deform_attn_backward_binned_workspace_bytes(N, M, Lq, P, H, W))
    assert nws == int(lib.df3d_ms_deform_attn_backward_binned_ml_workspace_bytes(N, M, Lq, 1, P, hw, 0))

    def call(entry, ordered):
        nbytes = nws if not ordered else int(lib.df3d_ms_deform_attn_backward_binned_ml_workspace_bytes(N, M, Lq, 1, P, hw, 1))
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        slabs = torch.empty((nslab // 4,), dtype=torch.float32, device=dev)
        gv, gl, ga = torch.empty_like(value), torch.empty_like(loc), torch.empty_like(aw)
        head = [ops._ptr(t) for t in (value, shp, ls, loc, aw, go)]
        tail = [ops._ptr(gv), ops._ptr(gl), ops._ptr(ga), ops._ptr(ws), nbytes, ops._ptr(slabs), ops._stream()]
        if entry == "df3d_ms_deform_attn_backward_binned":
            rc = lib.df3d_ms_deform_attn_backward_binned(*(head + [N, M, D, Lq, P, H, W] + tail))
        else:
            rc = lib.df3d_ms_deform_attn_backward_binned_ml(*(head + [hw, st, N, M, D, Lq, 1, P, ordered] + tail))
        _lib.check(rc, entry)
        return [t.cpu() for t in (gv, gl, ga)]

    single = call("df3d_ms_deform_attn_backward_binned", 0)
    for ordered in (0, 1):
        general = call("df3d_ms_deform_attn_backward_binned_ml", ordered)
        bound = 2e-5 * max(1.0, float(general[0].abs().max()))
        diff = float((single[0] - general[0]).abs().max())
        print("ordered = %d: |single - general| of grad_value %.3e (bound %.3e)" % (ordered, diff, bound))
        assert diff <= bound, ordered                                              # (summation order of a bin's points)
        assert torch.equal(single[1], general[1]) and torch.equal(single[2], general[2]), ordered
    assert float(single[0].abs().max()) > 0.0
    _assert_no_overflow()
