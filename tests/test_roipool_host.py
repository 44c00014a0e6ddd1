"""RoI grid pooling without a GPU: the C entries are declared, exported, bound and report null arguments; the product ops
refuse CPU tensors; VoxelRCNNHead built from the shipped pool settings carries the reference's parameter names and
shapes; the triple-loop query of tests/roipool_reference.py equals a brute-force restatement; the pybind-name shim
installs under pcdet's import path."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import roipool_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["df3d_voxel_query", "df3d_voxel_query_dense", "df3d_group_points_stack", "df3d_group_points_stack_grad_workspace_bytes",
           "df3d_group_points_stack_grad", "df3d_voxel_pool_fused"]


def test_symbols_are_declared_exported_and_bound():
    import __graft_entry__ as ge
    ge._load(os.path.join(ge.PKG, "csrc", "build.py"), "df3d_build").build()
    from dualfusion import _lib
    header = open(os.path.join(ROOT, "include", "df3d_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, header), s
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES, s


def test_null_arguments_and_limits_are_reported_without_a_gpu():
    from dualfusion import _lib
    lib = _lib.bind(ctypes.CDLL(_lib.LIB_PATH), check=False)
    assert lib.df3d_voxel_query(None, None, 1, None, None, 0, None, None, 0, None, 0.5, 4, None, None) == -1
    assert b"voxel_query: null" in lib.df3d_last_error()
    assert lib.df3d_voxel_query_dense(None, 1, None, None, 0, None, None, 0, None, 0.5, 4, None, None) == -1
    assert b"voxel_query_dense: null" in lib.df3d_last_error()
    assert lib.df3d_group_points_stack(None, None, None, None, 1, 0, 4, 4, 0, None, None) == -1
    assert b"group_points_stack: null" in lib.df3d_last_error()
    assert lib.df3d_group_points_stack_grad(None, None, None, None, 1, 0, 4, 0, 4, None, None, 0, None) == -1
    assert b"group_points_stack_grad: null" in lib.df3d_last_error()
    assert lib.df3d_voxel_pool_fused(None, None, 0, 32, None, None, 1, None, None, None, 0, None, 0.5, 16, None, 0, None, None,
                                     None, None) == -1
    assert b"voxel_pool_fused: null" in lib.df3d_last_error()
    # shapes no kernel serves are refused by name of the limit, before anything is launched (M = 0: nothing would be)
    one = (ctypes.c_int * 4)(1, 1, 1, 1)
    buf = ctypes.cast(one, ctypes.c_void_p)
    shape, k1 = _lib.int3((4, 4, 4))
    wide, k2 = _lib.int3((1, 1, 16))
    assert lib.df3d_voxel_query(buf, None, 1, shape, buf, 0, buf, buf, 0, wide, 0.5, 4, buf, None) == -1
    assert b"x query range 16 is above the limit of 15" in lib.df3d_last_error()
    ok, k3 = _lib.int3((1, 1, 1))
    aligned = (ctypes.c_float * 64)()
    ab = ctypes.c_void_p((ctypes.addressof(aligned) + 15) // 16 * 16)
    assert lib.df3d_voxel_pool_fused(ab, buf, 0, 32, buf, None, 1, shape, buf, buf, 0, ok, 0.5, 17, ab, 0, ab, None, None, None) == -1
    assert b"nsample 17 is above the limit of 16" in lib.df3d_last_error()
    assert lib.df3d_voxel_pool_fused(ab, buf, 0, 24, buf, None, 1, shape, buf, buf, 0, ok, 0.5, 16, ab, 0, ab, None, None, None) == -1
    assert b"16, 32 and 64 channels" in lib.df3d_last_error()
    assert lib.df3d_group_points_stack_grad_workspace_bytes(1 << 28, 16, None) == 0          # M * nsample >= 2^31


def test_product_ops_refuse_cpu_tensors():
    from dualfusion import _lib, ops
    from dualfusion import pointnet2_stack as ps
    xyz, new_xyz = torch.zeros(5, 3), torch.zeros(2, 3)
    coords = torch.zeros(2, 4, dtype=torch.int32)
    table = torch.full((1, 2, 2, 2), -1, dtype=torch.int32)
    cnt = torch.tensor([5], dtype=torch.int32)
    with pytest.raises(_lib.Df3dError):
        ops.voxel_query((1, 1, 1), 0.5, 4, xyz, new_xyz, coords, table)
    with pytest.raises(_lib.Df3dError):
        ps.voxel_query((1, 1, 1), 0.5, 4, xyz, new_xyz, coords, table)
    with pytest.raises(_lib.Df3dError):
        ops.group_points_stack(torch.zeros(5, 4), cnt, torch.zeros(2, 4, dtype=torch.int32), torch.tensor([2], dtype=torch.int32))
    with pytest.raises(_lib.Df3dError):
        ops.group_points_stack_backward(torch.zeros(2, 4, 4), torch.zeros(2, 4, dtype=torch.int32),
                                        torch.tensor([2], dtype=torch.int32), cnt, 5)
    grid = ops.GridDirectory(torch.zeros(64, dtype=torch.uint8), None, 1, (2, 2, 2))
    with pytest.raises(_lib.Df3dError):
        ops.voxel_pool_fused(torch.zeros(5, 32), xyz, grid, new_xyz, coords, (1, 1, 1), 0.5, 4, torch.zeros(32, 4))
    assert ops.voxel_pool_fused_supported(32, 16, (4, 4, 4), "max_pool")
    assert ops.voxel_pool_fused_supported(64, 1, (0, 0, 15), "avg_pool", grid)
    assert not ops.voxel_pool_fused_supported(24, 16, (4, 4, 4))
    assert not ops.voxel_pool_fused_supported(32, 17, (4, 4, 4))
    assert not ops.voxel_pool_fused_supported(32, 16, (4, 4, 16))
    assert not ops.voxel_pool_fused_supported(32, 16, (4, 4, 4), "sum_pool")
    assert not ops.voxel_pool_fused_supported(32, 16, (4, 4, 4), "max_pool", table)        # the dense table: composed path


def test_head_from_the_shipped_pool_config_has_the_reference_parameter_names():
    from dualfusion import roi_heads
    from dualfusion.registry import ROI_HEADS
    assert ROI_HEADS.get("VoxelRCNNHead") is roi_heads.VoxelRCNNHead
    cfg = ref.HEAD_CFG
    before = repr(cfg)
    head = roi_heads.VoxelRCNNHead(ref.BACKBONE_CHANNELS, cfg, ref.KITTI_RANGE, ref.KITTI_VOXEL, num_class=1)
    assert repr(cfg) == before                                   # the config is not edited (the reference prepends to MLPS)
    sd = {k: tuple(v.shape) for k, v in head.state_dict().items()}
    cin = {0: 32, 1: 64, 2: 64}
    for k in range(3):
        pre = "roi_grid_pool_layers.%d." % k
        assert sd[pre + "mlps_in.0.0.weight"] == (32, cin[k], 1)
        assert sd[pre + "mlps_in.0.1.running_var"] == (32,)
        assert sd[pre + "mlps_pos.0.0.weight"] == (32, 3, 1, 1)
        assert sd[pre + "mlps_pos.0.1.weight"] == (32,)
        assert sd[pre + "mlps_out.0.0.weight"] == (32, 32, 1)
        assert sd[pre + "mlps_out.0.1.bias"] == (32,)
        assert not any(name.startswith(pre + "groupers") for name in sd)
    assert sd["shared_fc_layer.0.weight"] == (256, 216 * 96)
    assert sd["shared_fc_layer.1.running_mean"] == (256,)
    assert sd["shared_fc_layer.4.weight"] == (256, 256)          # Linear, BN, ReLU, Dropout, Linear
    assert sd["cls_fc_layers.0.weight"] == (256, 256) and sd["cls_fc_layers.4.weight"] == (256, 256)
    assert sd["reg_fc_layers.0.weight"] == (256, 256) and sd["reg_fc_layers.5.weight"] == (256,)
    assert sd["cls_pred_layer.weight"] == (1, 256) and sd["cls_pred_layer.bias"] == (1,)
    assert sd["reg_pred_layer.weight"] == (7, 256) and sd["reg_pred_layer.bias"] == (7,)
    names = [type(m).__name__ for m in head.shared_fc_layer]
    assert names == ["Linear", "BatchNorm1d", "ReLU", "Dropout", "Linear", "BatchNorm1d", "ReLU"]
    layer = head.roi_grid_pool_layers[1]
    assert (layer.groupers[0].max_range, layer.groupers[0].radius, layer.groupers[0].nsample) == ([4, 4, 4], 0.8, 16)
    assert float(layer.mlps_pos[0][1].weight.detach().min()) == 1.0 and float(layer.mlps_out[0][1].bias.detach().abs().max()) == 0.0
    with pytest.raises(KeyError, match="rois"):
        head({"batch_size": 1})


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_triple_loop_query_equals_brute_force(seed):
    fx = ref.base_fixture(seed)
    assert 1300 < len(fx["indices"]) < 1600
    for rng, radius, nsample in ref.SETTINGS:
        idx, found = ref.voxel_query(fx["table"], fx["xyz"], fx["new_xyz"], fx["new_coords"], rng, radius, nsample)
        brute = ref.voxel_query_brute(fx["indices"], fx["xyz"], fx["new_xyz"], fx["new_coords"], fx["shape"], rng, radius, nsample)
        assert np.array_equal(idx, brute)
        assert ref.near_boundary(fx["table"], fx["xyz"], fx["new_xyz"], fx["new_coords"], rng, radius) == 0
    # the fixture exercises what it is meant to: overfull balls, empty balls, centres outside the grid
    idx, found = ref.voxel_query(fx["table"], fx["xyz"], fx["new_xyz"], fx["new_coords"], (4, 4, 4), 0.8, 16)
    assert (found > 16).sum() >= 10 and (found == 0).sum() >= 40
    c = fx["new_coords"][:, 1:]
    assert ((c < 0) | (c >= np.asarray(fx["shape"]))).any(1).sum() >= 30


def test_reference_grouping_and_gradient_agree_with_loops():
    rs = np.random.RandomState(3)
    feat_cnt, idx_cnt = [7, 5], [3, 4]
    features = rs.standard_normal((12, 3)).astype(np.float32)
    idx = np.concatenate([rs.randint(0, 7, (3, 4)), rs.randint(0, 5, (4, 4))]).astype(np.int32)
    out = ref.group_points_stack(features, feat_cnt, idx, idx_cnt)
    grad_out = rs.standard_normal(out.shape).astype(np.float32)
    grad, mag, refs = ref.group_points_stack_grad(grad_out, idx, idx_cnt, feat_cnt, 12)
    want = np.zeros((12, 3))
    for m in range(7):
        start = 0 if m < 3 else 7
        for s in range(4):
            for c in range(3):
                assert out[m, c, s] == features[start + idx[m, s], c]
                want[start + idx[m, s], c] += float(grad_out[m, c, s])
    assert np.allclose(grad, want, rtol=0, atol=1e-12) and refs.sum() == 28 and (mag >= np.abs(grad) - 1e-12).all()


def test_shim_installs_under_the_pcdet_import_path():
    from dualfusion import ext
    path = "pcdet.ops.pointnet2.pointnet2_stack.pointnet2_stack_cuda"
    assert ext.ALIASES["pointnet2_stack_cuda"] == (path,)
    saved = dict(sys.modules)
    try:
        for k in [k for k in sys.modules if k.split(".")[0] == "pcdet"]:
            del sys.modules[k]
        assert path in ext.install()
        import importlib
        mod = importlib.import_module(path)
        assert mod is ext.load("pointnet2_stack_cuda")
        for name in ("voxel_query_wrapper", "group_points_wrapper", "group_points_grad_wrapper"):
            assert callable(getattr(mod, name)), name
        with pytest.raises(RuntimeError):                            # CPU tensors: a RuntimeError like pybind's
            mod.voxel_query_wrapper(2, 2, 2, 2, 4, 0.5, 1, 1, 1, torch.zeros(2, 3), torch.zeros(5, 3),
                                    torch.zeros(2, 4, dtype=torch.int32), torch.full((1, 2, 2, 2), -1, dtype=torch.int32),
                                    torch.zeros(2, 4, dtype=torch.int32))
        with pytest.raises(RuntimeError):
            mod.group_points_wrapper(1, 2, 4, 4, torch.zeros(5, 4), torch.tensor([5], dtype=torch.int32),
                                     torch.zeros(2, 4, dtype=torch.int32), torch.tensor([2], dtype=torch.int32),
                                     torch.zeros(2, 4, 4))
        with pytest.raises(RuntimeError):
            mod.group_points_grad_wrapper(1, 2, 4, 5, 4, torch.zeros(2, 4, 4), torch.zeros(2, 4, dtype=torch.int32),
                                          torch.tensor([2], dtype=torch.int32), torch.tensor([5], dtype=torch.int32),
                                          torch.zeros(5, 4))
    finally:
        for k in list(sys.modules):
            if k not in saved and k.split(".")[0] == "pcdet":
                del sys.modules[k]
        sys.modules.update({k: v for k, v in saved.items() if k.split(".")[0] == "pcdet"})
