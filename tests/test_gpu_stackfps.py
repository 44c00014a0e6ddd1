"""Stacked furthest point sampling on the GPU (csrc/pointops.hip: stack_fps_kernel; ops.stack_furthest_point_sample,
pointnet2_stack.stack_farthest_point_sample, the pointnet2_stack_cuda shim, pfe.sector_fps and VoxelSetAbstraction's stacked
keypoint path) against the host restatement (tests/stackfps_reference.py) and the reference's own outputs
(tests/golden/stack_fps.npz, vsa.npz).

Indices are compared with array_equal.  The precondition is asserted on the reference alone, without a GPU
(tests/test_stackfps_host.py): random clouds keep every pick MARGIN_ULPS ulps ahead of the next distinct distance, lattice
clouds have distances that are exact in float32, so no pick depends on how a correct implementation rounds."""
import functools

import numpy as np
import pytest
import torch

import stackfps_reference as fr
import stacksa_reference as sr

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODES = (("stack", fr.STACK), ("frames", fr.FRAMES))


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def counts(c):
    return torch.tensor(list(c), dtype=torch.int32, device=DEV)


def run(xyz, cnt, num, mode, **kw):
    from dualfusion import ops
    return ops.stack_furthest_point_sample(T(xyz), counts(cnt), num, mode=mode, **kw).cpu().numpy()


@functools.lru_cache(maxsize=None)
def want_single(n, m, mode, seed):
    return fr.stack_fps(fr.random_cloud(n, seed), [n], [m], mode)


@pytest.mark.parametrize("n", fr.SMALL_SIZES)
def test_small_segments_both_modes(n):
    for name, mode in MODES:
        got = run(fr.random_cloud(n, n), [n], fr.small_m(n), name)
        assert got.dtype == np.int32 and np.array_equal(got, want_single(n, fr.small_m(n), mode, n)), (n, name)


@pytest.mark.parametrize("n", fr.EDGE_SIZES)
def test_variant_edges(n):
    """8192 | 8193, 16384 | 16385, 24576 | 24577 rows change the rows kept per thread; 32769 rows keep the minima in `temp`"""
    for name, mode in MODES:
        assert np.array_equal(run(fr.random_cloud(n, n), [n], [24], name), want_single(n, 24, mode, n)), (n, name)


@pytest.mark.parametrize("n", [24576, 24577, 32768, 32769])
def test_the_register_variant_of_the_lds_range(n, monkeypatch):
    """24 577 .. 32 768 rows keep their minima in LDS by default (tested above); DF3D_STACK_FPS_LDS=0 (read per call) keeps
    them in registers, and changes nothing on either side of that range"""
    monkeypatch.setenv("DF3D_STACK_FPS_LDS", "0")
    for name, mode in MODES:
        assert np.array_equal(run(fr.random_cloud(n, n), [n], [24], name), want_single(n, 24, mode, n)), (n, name)


@pytest.mark.parametrize("name,mode", MODES)
def test_seven_segments_of_every_variant_in_one_launch(name, mode):
    from dualfusion import ops
    cloud = fr.seven_cloud()
    M = sum(fr.SEVEN_PICKS)
    want = fr.stack_fps(cloud, fr.SEVEN_SIZES, fr.SEVEN_PICKS, mode, idx=np.full(M + 6, -7, np.int32))
    out = torch.full((M + 6,), -7, dtype=torch.int32, device=DEV)
    got = ops.stack_furthest_point_sample(T(cloud), counts(fr.SEVEN_SIZES), counts(fr.SEVEN_PICKS), total=M, mode=name, out=out)
    assert got is out and np.array_equal(out.cpu().numpy(), want) and (want[M:] == -7).all() and (want[:M] >= 0).all()
    # the same through a list (M known on the host) and a device tensor whose sum is read back
    assert np.array_equal(run(cloud, fr.SEVEN_SIZES, list(fr.SEVEN_PICKS), name), want[:M])
    assert np.array_equal(run(cloud, fr.SEVEN_SIZES, counts(fr.SEVEN_PICKS), name), want[:M])
    # segments in the middle of the launch alone: slots before and after theirs stay untouched
    cnt, num = list(fr.SEVEN_SIZES), [0, 0, 0, 5, 0, 0, 2]
    out = torch.full((9,), -7, dtype=torch.int32, device=DEV)
    ops.stack_furthest_point_sample(T(cloud), counts(cnt), counts(num), total=7, mode=name, out=out)
    assert np.array_equal(out.cpu().numpy(), fr.stack_fps(cloud, cnt, num, mode, idx=np.full(9, -7, np.int32)))


@pytest.mark.parametrize("name,mode", MODES)
def test_ties_on_lattice_clouds(name, mode):
    for cloud in (fr.lattice_cloud(600, 5), fr.lattice_cloud(3000, 6, duplicate=True)):
        n = len(cloud)
        assert np.array_equal(run(cloud, [n], [64], name), fr.stack_fps(cloud, [n], [64], mode)), n


def test_tails_and_empty_segments():
    cloud = fr.random_cloud(50, 3)
    got = run(cloud, [50], [55], "stack")                                # the loop keeps picking past the segment's rows
    assert np.array_equal(got, fr.stack_fps(cloud, [50], [55], fr.STACK)) and (got[50:] == 0).all()
    got = run(cloud, [50], [64], "frames")                               # the cyclic tail
    assert np.array_equal(got, fr.stack_fps(cloud, [50], [64], fr.FRAMES)) and np.array_equal(got[50:], got[:14])
    for name, mode in MODES:
        got = run(cloud, [0, 50], [4, 3], name)
        assert np.array_equal(got[:4], [-1] * 4) and np.array_equal(got, fr.stack_fps(cloud, [0, 50], [4, 3], mode))
        # counts that promise more rows and slots than there are: clipped, nothing past either end
        from dualfusion import ops
        out = torch.full((8,), -7, dtype=torch.int32, device=DEV)
        ops.stack_furthest_point_sample(T(cloud), counts([40, 40]), counts([3, 3]), total=5, mode=name, out=out)
        assert np.array_equal(out.cpu().numpy(), fr.stack_fps(cloud, [40, 40], [3, 3], mode, idx=np.full(5, -7, np.int32)).tolist() + [-7] * 3)
    assert run(np.zeros((0, 3), np.float32), [0, 0], [2, 1], "stack").tolist() == [-1, -1, -1]
    assert run(cloud, [50], 0, "stack").shape == (0,)


def test_two_runs_are_bit_equal():
    cloud = fr.seven_cloud()
    for name, _ in MODES:
        a = run(cloud, fr.SEVEN_SIZES, list(fr.SEVEN_PICKS), name)
        assert np.array_equal(a, run(cloud, fr.SEVEN_SIZES, list(fr.SEVEN_PICKS), name))
    lat = fr.lattice_cloud(3000, 6, duplicate=True)
    assert np.array_equal(run(lat, [3000], [200], "frames"), run(lat, [3000], [200], "frames"))


def test_256_segments():
    cloud = np.concatenate([fr.random_cloud(40, 500 + i) for i in range(256)])
    for name, mode in MODES:
        assert np.array_equal(run(cloud, [40] * 256, 8, name), fr.stack_fps(cloud, [40] * 256, [8] * 256, mode)), name


def test_frames_mode_is_the_batch_kernel_called_per_frame():
    from dualfusion import ops
    frames = [fr.random_cloud(n, 60 + i) for i, n in enumerate(fr.FRAME_SIZES)]
    got = run(np.concatenate(frames), fr.FRAME_SIZES, 64, "frames").reshape(3, 64)
    start = 0
    for b, cloud in enumerate(frames):
        n = len(cloud)
        per = ops.furthest_point_sample(T(cloud)[None], min(n, 64))[0].cpu().numpy()
        assert np.array_equal(got[b, :len(per)] - start, per), n
        assert np.array_equal(got[b] - start, sr.pad_keypoints(per, 64))
        start += n


def test_the_shim_and_the_reference_named_function_give_the_ops_results(golden):
    from dualfusion import ext
    from dualfusion import pointnet2_stack as ps
    mod = ext.load("pointnet2_stack_cuda")
    g = golden("stack_fps.npz")
    for name in ("list", "int", "tensor", "lattice"):
        xyz, cnt, num, want = (g["stack__%s__%s" % (name, k)] for k in ("xyz", "cnt", "num", "idx"))
        idx = torch.full((len(want),), -7, dtype=torch.int32, device=DEV)
        temp = torch.full((len(xyz),), 1e10, device=DEV)
        assert mod.stack_farthest_point_sampling_wrapper(T(xyz), temp, T(cnt), idx, T(num)) == 1
        assert np.array_equal(idx.cpu().numpy(), want), name
        assert np.array_equal(run(xyz, cnt, T(num), "stack"), want)
        npoint = {"list": num.tolist(), "int": int(num[0]), "tensor": T(num), "lattice": num.tolist()}[name]
        got = ps.stack_farthest_point_sample(T(xyz), T(cnt), npoint)
        assert got.dtype == torch.int32 and not got.requires_grad and np.array_equal(got.cpu().numpy(), want)
    frames = np.stack([fr.random_cloud(200, 60), fr.random_cloud(200, 77)])
    out = torch.full((2, 16), -7, dtype=torch.int32, device=DEV)
    assert mod.farthest_point_sampling_wrapper(2, 200, 16, T(frames), torch.full((2, 200), 1e10, device=DEV), out) == 1
    from dualfusion import ops
    assert np.array_equal(out.cpu().numpy(), ops.furthest_point_sample(T(frames), 16).cpu().numpy())
    assert np.array_equal(out.cpu().numpy()[0], fr.stack_fps(frames[0], [200], [16], fr.FRAMES))


def test_sector_fps_equals_the_reference(golden):
    from dualfusion import pfe
    g = golden("stack_fps.npz")
    K, sectors = (int(v) for v in g["sector__args"])
    got = pfe.sector_fps(T(g["sector__points"]), K, sectors)
    assert np.array_equal(got.cpu().numpy(), g["sector__sampled"])


# -------------------------------------------------------------------------------------------------------- VoxelSetAbstraction
def _vsa_batch(inputs):
    from dualfusion.spconv import SparseConvTensor
    levels = {}
    for stride, (name, (ind, feats)) in zip((1, 2, 4, 8), inputs["levels"].items()):
        levels[name] = SparseConvTensor(T(feats), T(ind), [s // stride for s in sr.VSA_GRID], 2)
    return {"batch_size": 2, "points": T(inputs["points"]), "voxel_coords": T(inputs["voxel_coords"]),
            "spatial_features": T(inputs["bev"]), "spatial_features_stride": inputs["bev_stride"], "multi_scale_3d_features": levels}


def _vsa(point_source):
    from dualfusion import pfe
    cfg = sr.vsa_cfg(point_source)
    vsa = pfe.VoxelSetAbstraction(cfg, sr.VSA_VOXEL, sr.VSA_RANGE, num_bev_features=sr.VSA_BEV[0], num_rawpoint_features=4)
    vsa.load_state_dict(sr.torch_state(sr.vsa_state(cfg)), strict=True)
    return vsa.to(DEV).eval()


@pytest.mark.parametrize("point_source", ["raw_points", "voxel_centers"])
def test_voxel_set_abstraction_with_the_switch_on_and_off(point_source, golden, monkeypatch):
    from dualfusion import ops
    want = golden("vsa.npz")["vsa__%s__keypoints" % point_source]
    vsa, inputs = _vsa(point_source), sr.vsa_inputs()
    calls, real = [], ops.stack_furthest_point_sample

    def counted(*a, **k):
        calls.append(k.get("mode"))
        return real(*a, **k)
    monkeypatch.setattr(ops, "stack_furthest_point_sample", counted)
    with torch.no_grad():
        monkeypatch.setenv("DF3D_VSA_STACK_FPS", "1")
        on = vsa(_vsa_batch(inputs))
        assert calls == ["frames"]
        monkeypatch.setenv("DF3D_VSA_STACK_FPS", "0")
        off = vsa(_vsa_batch(inputs))
        assert calls == ["frames"]                                       # the switch is read per call
        monkeypatch.delenv("DF3D_VSA_STACK_FPS")
        default = vsa(_vsa_batch(inputs))
    for out in (on, off, default):
        assert np.array_equal(out["point_coords"].cpu().numpy(), want)
    assert np.array_equal(on["point_features"].cpu().numpy(), off["point_features"].cpu().numpy())


def test_the_stacked_forward_makes_no_device_to_host_copy(monkeypatch):
    monkeypatch.setenv("DF3D_VSA_STACK_FPS", "1")
    vsa, batch = _vsa("raw_points"), _vsa_batch(sr.vsa_inputs())
    with torch.no_grad():
        vsa(dict(batch))                                                 # warm-up: allocations, cached constants
        torch.cuda.synchronize()
        probe = torch.ones((1,), device=DEV)
        torch.cuda.set_sync_debug_mode("error")
        try:
            with pytest.raises(RuntimeError):
                probe.item()                                             # the mode is honoured by this build
            out = vsa(dict(batch))
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert bool(torch.isfinite(out["point_features"]).all())


@pytest.mark.parametrize("point_source", ["raw_points", "voxel_centers"])
def test_an_empty_frame_gives_nan_keypoints_on_the_stacked_path(point_source, monkeypatch):
    vsa, inputs = _vsa(point_source), sr.vsa_inputs()
    batch = _vsa_batch(inputs)
    batch["points"] = T(inputs["points"][inputs["points"][:, 0] == 0])
    batch["voxel_coords"] = T(inputs["voxel_coords"][inputs["voxel_coords"][:, 0] == 0])
    monkeypatch.setenv("DF3D_VSA_STACK_FPS", "1")
    kp = vsa.get_sampled_points(batch).cpu().numpy()
    assert kp.shape == (128, 4) and np.isfinite(kp[:64]).all() and np.isnan(kp[64:, 1:]).all() and (kp[64:, 0] == 1).all()
    monkeypatch.setenv("DF3D_VSA_STACK_FPS", "0")
    with pytest.raises(ValueError, match="frame 1 has no points"):
        vsa.get_sampled_points(batch)
