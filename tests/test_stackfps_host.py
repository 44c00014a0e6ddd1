"""Stacked furthest point sampling without a GPU: the host restatement (tests/stackfps_reference.py) against the batch
restatement and the reference's own outputs (tests/golden/stack_fps.npz), the preconditions the GPU tests rely on (margins,
real ties, every in-kernel variant reached), the block-size formula, and the refusals of the library and the Python layers."""
import ctypes
import inspect
import math

import numpy as np
import pytest
import torch

import stackfps_reference as fr
import stacksa_reference as sr


def test_frames_mode_on_one_segment_is_the_batch_restatement():
    inputs = sr.vsa_inputs()
    pts = inputs["points"]
    clouds = [pts[pts[:, 0] == b][:, 1:4] for b in range(2)]
    clouds.append(sr.voxel_centers(inputs["voxel_coords"][inputs["voxel_coords"][:, 0] == 0][:, 1:4], 1, sr.VSA_VOXEL, sr.VSA_RANGE))
    clouds.append(fr.lattice_cloud(1500, 1))
    for cloud in clouds:
        n = len(cloud)
        m = min(n, 64)
        want = sr.furthest_point_sample(cloud, m)
        got = fr.stack_fps(cloud, [n], [m], fr.FRAMES)
        assert np.array_equal(got, want)
        padded = fr.stack_fps(cloud, [n], [n + 9], fr.FRAMES)          # the cyclic tail is pad_keypoints
        assert np.array_equal(padded, sr.pad_keypoints(sr.furthest_point_sample(cloud, n), n + 9))


def test_the_two_modes_differ_below_1024_lattice_rows_and_agree_from_there():
    small, big = fr.lattice_cloud(600, 5), fr.lattice_cloud(3000, 6, duplicate=True)
    a, b = fr.stack_fps(small, [600], [64], fr.STACK), fr.stack_fps(small, [600], [64], fr.FRAMES)
    assert not np.array_equal(a, b)                     # bs = 1024 against bs = 512: one tie rule for both would fail here
    assert np.array_equal(a[:2], b[:2])
    a, b = fr.stack_fps(big, [3000], [64], fr.STACK), fr.stack_fps(big, [3000], [64], fr.FRAMES)
    assert np.array_equal(a, b)
    for n in (1024, 1025, 5000):
        assert fr.fps_block(n) == 1024


def test_block_formula_is_fps_block_for_every_size():
    n = np.arange(1, (1 << 21) + 1, dtype=np.int64)
    from_bits = np.minimum(1 << (np.floor(np.log2(n.astype(np.float64))).astype(np.int64)), 1024)
    from_log = np.minimum(1 << (np.log(n.astype(np.float64)) / math.log(2.0)).astype(np.int64), 1024)
    exact = np.minimum(1 << (np.frexp(n.astype(np.float64))[1] - 1).astype(np.int64), 1024)   # the bit length
    assert np.array_equal(from_bits, exact) and np.array_equal(from_log, exact)
    for k in (1, 2, 3, 1023, 1024, 1025, (1 << 21) - 1, 1 << 21):
        assert fr.fps_block(k) == fr.fps_block_log(k) == exact[k - 1]


def test_the_gpu_sizes_reach_every_variant():
    sizes = list(fr.SMALL_SIZES) + list(fr.EDGE_SIZES) + [n for n in fr.SEVEN_SIZES if n]
    for mode in (fr.STACK, fr.FRAMES):
        assert {fr.variant(n, mode) for n in sizes} == {"8", "16", "24", "32", "temp"}
        assert {fr.variant(n, mode) for n in fr.SEVEN_SIZES if n} == {"8", "16", "24", "32", "temp"}
        assert [fr.variant(n, mode) for n in fr.EDGE_SIZES] == ["8", "16", "16", "24", "24", "32", "32", "temp"]
    # the thresholds, restated: rows per thread = ceil(n / bs); bs < 1024 only below 1024 rows, where it is 1 row (or 2)
    assert fr.variant(1023, fr.FRAMES) == fr.variant(1023, fr.STACK) == "8" and fr.fps_block(1023) == 512
    assert fr.MAXPT * 1024 == 32768


def test_margins_and_ties_of_the_gpu_cases_on_the_reference_alone():
    """random clouds: every pick at least MARGIN_ULPS ulps ahead of the next distinct value (so the picks do not depend on
    how a correct implementation rounds); lattice clouds: fused and unfused distances agree bit for bit, and real ties occur"""
    for n in fr.SMALL_SIZES:
        for mode_bs in (1024, fr.fps_block(n)):
            assert fr.pick_margins(fr.random_cloud(n, n), fr.small_m(n), mode_bs).min() >= fr.MARGIN_ULPS, n
    for n in fr.EDGE_SIZES:
        assert fr.pick_margins(fr.random_cloud(n, n), 24, 1024).min() >= fr.MARGIN_ULPS, n
    s, cloud = 0, fr.seven_cloud()
    for n, m in zip(fr.SEVEN_SIZES, fr.SEVEN_PICKS):
        if n:
            for mode_bs in (1024, fr.fps_block(n)):
                assert fr.pick_margins(cloud[s:s + n], m, mode_bs).min() >= fr.MARGIN_ULPS, n
        s += n
    for i in range(256):                                                 # the 256-segment launch
        for mode_bs in (1024, 32):
            assert fr.pick_margins(fr.random_cloud(40, 500 + i), 8, mode_bs).min() >= fr.MARGIN_ULPS, i
    assert fr.pick_margins(fr.random_cloud(50, 3), 50, 1024).min() >= fr.MARGIN_ULPS                 # the tails
    assert fr.pick_margins(fr.random_cloud(50, 3), 50, 32).min() >= fr.MARGIN_ULPS
    for i, n in enumerate(fr.FRAME_SIZES):
        assert fr.pick_margins(fr.random_cloud(n, 60 + i), min(n, 64), fr.fps_block(n)).min() >= fr.MARGIN_ULPS, n
    for cloud in (fr.lattice_cloud(600, 5), fr.lattice_cloud(3000, 6, duplicate=True)):
        assert np.abs(cloud).max() < 64 and np.array_equal(cloud * 4, np.round(cloud * 4))
        for c in cloud[:50]:
            assert np.array_equal(fr.dist2_fma(cloud, c), fr.dist2_unfused(cloud, c))
        for mode in (fr.STACK, fr.FRAMES):
            n = len(cloud)
            bs = 1024 if mode == fr.STACK else fr.fps_block(n)
            assert fr.count_tied_picks(cloud, 64, bs) >= 1
            assert np.array_equal(fr.stack_fps(cloud, [n], [64], mode), fr.stack_fps(cloud, [n], [64], mode, dist=fr.dist2_unfused))


def test_fused_distance_is_three_float32_roundings():
    """against exact rational arithmetic on a few hundred random float32 triples"""
    from fractions import Fraction
    rs = np.random.RandomState(0)
    pts = (rs.standard_normal((300, 3)) * rs.choice([1e-3, 1.0, 37.0, 4e3], (300, 1))).astype(np.float32)
    got = fr.dist2_fma(pts, np.zeros(3, np.float32))

    def rnd(fr_):                                       # Fraction -> nearest float32 (ties to even), via exact comparison
        f = np.float32(float(fr_))                      # float() of a Fraction is correctly rounded to float64; then fix up
        lo, hi = np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))
        cands = sorted({float(lo), float(f), float(hi)})
        best = min(cands, key=lambda c: (abs(Fraction(c) - fr_), int(np.float32(c).view(np.int32)) & 1))
        return np.float32(best)
    for p, g in zip(pts, got):
        x, y, z = (Fraction(float(v)) for v in p)
        a = rnd(x * x)
        b = rnd(y * y + Fraction(float(a)))
        c = rnd(z * z + Fraction(float(b)))
        assert c == g


def test_tails_and_empty_segments():
    cloud = fr.random_cloud(50, 3)
    over = fr.stack_fps(cloud, [50], [55], fr.STACK)                   # the loop keeps picking: all minima are 0, row 0 wins
    assert sorted(over[:50]) == list(range(50)) and (over[50:] == 0).all()
    cyc = fr.stack_fps(cloud, [50], [64], fr.FRAMES)
    assert np.array_equal(cyc[50:], cyc[:14]) and sorted(cyc[:50]) == list(range(50))
    idx = np.full(12, -7, np.int32)
    fr.stack_fps(cloud, [0, 20, 0, 30], [4, 3, 0, 2], fr.STACK, idx=idx)
    assert (idx[:4] == -1).all() and idx[4] == 0 and idx[7] == 20 and (idx[9:] == -7).all()
    clipped = fr.stack_fps(cloud, [40, 40], [3, 3], fr.STACK, idx=np.full(5, -7, np.int32))       # 10 rows and 2 slots left
    assert clipped[3] == 40 and (clipped[3:] < 50).all() and (clipped >= 0).all()


def test_sector_fps_and_the_stacked_op_reproduce_the_reference(golden):
    g = golden("stack_fps.npz")
    for name in ("list", "int", "tensor", "lattice"):
        got = fr.stack_fps(g["stack__%s__xyz" % name], g["stack__%s__cnt" % name], g["stack__%s__num" % name], fr.STACK)
        assert np.array_equal(got, g["stack__%s__idx" % name]), name
    points, (K, sectors) = g["sector__points"], g["sector__args"]
    want_points, want_args = fr.sector_case()[0], fr.sector_case()[1:]
    assert np.array_equal(points, want_points) and (int(K), int(sectors)) == want_args
    sampled, _, cnt, num = fr.sector_fps(points, int(K), int(sectors))
    assert np.array_equal(sampled, g["sector__sampled"]) and 0 in cnt and sum(num) == len(sampled) and sum(num) != K
    _, q = fr.sector_of(points, int(sectors))
    assert np.abs(q - np.round(q)).min() > 1e-3


def test_abi_refusals_without_a_gpu():
    from dualfusion import _lib
    lib = _lib.bind(ctypes.CDLL(_lib.LIB_PATH), check=False)
    one = (ctypes.c_float * 64)()
    buf = ctypes.cast(one, ctypes.c_void_p)
    err = lambda: lib.df3d_last_error()
    call = lambda xyz=buf, cnt=buf, N=8, num=buf, B=1, M=4, mode=0, temp=buf, idx=buf: \
        lib.df3d_stack_furthest_point_sample(xyz, cnt, N, num, B, M, mode, temp, idx, None)
    for kw in ("xyz", "cnt", "num", "temp", "idx"):
        assert call(**{kw: None}) == _lib.DF3D_EINVAL and b"null argument" in err()
    assert call(B=1025) == _lib.DF3D_EINVAL and b"at most 1024 a launch" in err()
    assert call(B=-1) == _lib.DF3D_EINVAL and b"negative" in err()
    assert call(mode=2) == _lib.DF3D_EINVAL and b"DF3D_FPS_FRAMES = 1" in err()
    assert call(N=1 << 31) == _lib.DF3D_EINVAL and b"below 2^31" in err()
    assert call(M=1 << 31) == _lib.DF3D_EINVAL and b"below 2^31" in err()
    assert call(B=0) == _lib.DF3D_OK and call(M=0) == _lib.DF3D_OK                          # nothing to do, no launch
    assert len(_lib.SIGNATURES["df3d_stack_furthest_point_sample"][1]) == 10


def test_python_layers_refuse_cpu_tensors():
    from dualfusion import _lib, ops, pfe
    from dualfusion import pointnet2_stack as ps
    xyz, cnt = torch.zeros(5, 3), torch.tensor([5], dtype=torch.int32)
    with pytest.raises(_lib.Df3dError, match="must live on the GPU"):
        ops.stack_furthest_point_sample(xyz, cnt, 2)
    with pytest.raises(_lib.Df3dError, match="must live on the GPU"):
        ps.stack_farthest_point_sample(xyz, cnt, [2])
    with pytest.raises(_lib.Df3dError, match="must live on the GPU"):
        pfe.sector_fps(xyz, 4, 2)
    assert list(inspect.signature(ops.stack_furthest_point_sample).parameters)[:5] == [
        "xyz", "xyz_batch_cnt", "num_sampled", "total", "mode"]
    assert list(inspect.signature(ps.stack_farthest_point_sample).parameters) == ["xyz", "xyz_batch_cnt", "npoint"]
    assert list(inspect.signature(pfe.sector_fps).parameters) == ["points", "num_sampled_points", "num_sectors"]
    assert "read back" in ops.stack_furthest_point_sample.__doc__ and ops.FPS_MODES == {"stack": fr.STACK, "frames": fr.FRAMES}
    assert "NaN" in pfe.VoxelSetAbstraction.get_sampled_points.__doc__


def test_the_shim_has_the_references_sampler_entries():
    from dualfusion import ext
    mod = ext.load("pointnet2_stack_cuda")
    assert list(inspect.signature(mod.stack_farthest_point_sampling_wrapper).parameters) == [
        "xyz", "temp", "xyz_batch_cnt", "idx", "num_sampled_points"]
    assert list(inspect.signature(mod.farthest_point_sampling_wrapper).parameters) == ["B", "N", "npoint", "xyz", "temp", "output"]
    assert "not provided" in mod.__doc__ and "three_nn" in mod.__doc__ and "vector pool" in mod.__doc__
    cnt, num = torch.tensor([5], dtype=torch.int32), torch.tensor([2], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        mod.stack_farthest_point_sampling_wrapper(torch.zeros(5, 3), torch.full((5,), 1e10), cnt, torch.zeros(2, dtype=torch.int32), num)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        mod.farthest_point_sampling_wrapper(1, 5, 2, torch.zeros(1, 5, 3), torch.full((1, 5), 1e10), torch.zeros(1, 2, dtype=torch.int32))
