"""The PV-RCNN point branch without a GPU: the C entries are declared, exported, bound and report null arguments and limits; the
refusals are made by name; StackSAModuleMSG, VoxelSetAbstraction and PVRCNNHead built from the shipped config carry the
reference's parameter names and shapes; the registries and the pybind-name shim know the new entries; the host restatement
(tests/stacksa_reference.py) equals what the reference's own modules gave (tests/golden/vsa.npz); the switch is read per
call."""
import ctypes
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

import stacksa_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["df3d_ball_query_stack", "df3d_stack_sa_fused_supported", "df3d_stack_sa_fused", "df3d_bev_interpolate",
           "df3d_bev_interpolate_grad_workspace_bytes", "df3d_bev_interpolate_grad"]


def test_symbols_are_declared_exported_and_bound():
    import __graft_entry__ as ge
    build = ge._load(os.path.join(ge.PKG, "csrc", "build.py"), "df3d_build")
    assert "stackpool.hip" in build.SOURCES
    build.build()
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
    assert lib.df3d_ball_query_stack(None, None, 0, None, None, 0, 1, 0.5, 16, None, None) == -1
    assert b"ball_query_stack: null" in lib.df3d_last_error()
    assert lib.df3d_stack_sa_fused(None, None, None, 0, None, None, 0, 1, 0.5, 16, 16, 16, None, None, None, None, None, None, None) == -1
    assert b"stack_sa_fused: null" in lib.df3d_last_error()
    assert lib.df3d_bev_interpolate(None, 0, None, 1, 8, 4, 4, 0.0, 0.0, 0.1, 0.1, 8.0, None, None) == -1
    assert b"bev_interpolate: null" in lib.df3d_last_error()
    assert lib.df3d_bev_interpolate_grad(None, None, 0, 1, 8, 4, 4, 0.0, 0.0, 0.1, 0.1, 8.0, None, None, 0, None) == -1
    assert b"bev_interpolate_grad: null" in lib.df3d_last_error()
    # limits are refused by name before anything is launched (M = 0: nothing would be)
    aligned = (ctypes.c_float * 64)()
    buf = ctypes.c_void_p((ctypes.addressof(aligned) + 15) // 16 * 16)
    assert lib.df3d_ball_query_stack(buf, buf, 0, buf, buf, 0, 1, 0.5, 65, buf, None) == -1
    assert b"nsample 65 is above the limit of 64" in lib.df3d_last_error()
    assert lib.df3d_ball_query_stack(buf, buf, 0, buf, buf, 0, 256, 0.5, 16, buf, None) == -1
    assert b"B = 256 outside 1..255" in lib.df3d_last_error()
    assert lib.df3d_ball_query_stack(buf, buf, 0, buf, buf, 0, 255, 0.5, 64, buf, None) == 0
    assert lib.df3d_stack_sa_fused(buf, buf, buf, 0, buf, buf, 0, 1, 0.5, 16, 24, 16, buf, buf, buf, buf, None, None, None) == -1
    assert b"serves 16, 32 and 64 channels and 16 or 32 samples" in lib.df3d_last_error()
    assert lib.df3d_stack_sa_fused(buf, buf, buf, 0, buf, buf, 0, 1, 0.5, 16, 64, 32, buf, buf, buf, buf, None, None, None) == 0
    assert lib.df3d_bev_interpolate(buf, 0, buf, 1, 8, 4, 4, 0.0, 0.0, 0.0, 0.1, 8.0, buf, None) == -1
    assert b"voxel size and stride must be positive" in lib.df3d_last_error()
    assert lib.df3d_bev_interpolate_grad_workspace_bytes(1 << 29, None) == 0                      # 4 * M >= 2^31
    for c1 in (16, 32, 64):
        for c2 in (16, 32, 64):
            assert lib.df3d_stack_sa_fused_supported(c1, c2, 16) == 1 and lib.df3d_stack_sa_fused_supported(c1, c2, 32) == 1
    assert lib.df3d_stack_sa_fused_supported(16, 16, 8) == 0 and lib.df3d_stack_sa_fused_supported(128, 64, 16) == 0


def test_refusals_by_name():
    from dualfusion import _lib, ops, pfe, roi_heads
    from dualfusion import pointnet2_stack as ps
    xyz, cnt = torch.zeros(5, 3), torch.tensor([5], dtype=torch.int32)
    new_xyz, new_cnt = torch.zeros(2, 3), torch.tensor([2], dtype=torch.int32)
    with pytest.raises(_lib.Df3dError, match="nsample 65 is above the limit of 64"):
        ps.ball_query_stack(0.5, 65, xyz, cnt, new_xyz, new_cnt)
    with pytest.raises(_lib.Df3dError, match="B = 256 is above the limit of 255"):
        ops.ball_query_stack(0.5, 16, xyz, torch.zeros(256, dtype=torch.int32), new_xyz, torch.zeros(256, dtype=torch.int32))
    with pytest.raises(_lib.Df3dError, match="must live on the GPU"):                            # no CPU fallback
        ps.ball_query_stack(0.5, 16, xyz, cnt, new_xyz, new_cnt)
    with pytest.raises(_lib.Df3dError, match="must live on the GPU"):
        ops.stack_sa_fused(None, xyz, cnt, new_xyz, new_cnt, 0.5, 16, torch.zeros(16, 4), torch.zeros(16, 16), torch.zeros(16))
    with pytest.raises(_lib.Df3dError, match="must live on the GPU"):
        ops.bev_interpolate(torch.zeros(2, 4), torch.zeros(1, 8, 4, 4), sr.VSA_RANGE, sr.VSA_VOXEL, 8)
    with pytest.raises(_lib.Df3dError, match="use the composed path"):
        ops.stack_sa_fused(None, xyz, cnt, new_xyz, new_cnt, 0.5, 16, torch.zeros(24, 4), torch.zeros(16, 24), torch.zeros(16))
    assert ops.stack_sa_fused_supported(16, 16, 16) and ops.stack_sa_fused_supported(64, 32, 32)
    assert not ops.stack_sa_fused_supported(128, 64, 16) and not ops.stack_sa_fused_supported(16, 16, 8)
    assert not ops.stack_sa_fused_supported(16, 16, 16, "avg_pool")                                # avg_pool: composed only
    with pytest.raises(NotImplementedError, match="VectorPoolAggregationModuleMSG"):
        ps.build_local_aggregation_module(16, {"NAME": "VectorPoolAggregationModuleMSG"})
    with pytest.raises(NotImplementedError, match="SPC"):
        pfe.VoxelSetAbstraction(dict(sr.SHIPPED_PFE, SAMPLE_METHOD="SPC"), sr.SHIPPED_PFE["VOXEL_SIZE"],
                                sr.SHIPPED_PFE["POINT_CLOUD_RANGE"], num_bev_features=256, num_rawpoint_features=4)
    sa = dict(sr.SHIPPED_PFE["SA_LAYER"])
    sa["x_conv3"] = dict(sa["x_conv3"], FILTER_NEIGHBOR_WITH_ROI=True)
    with pytest.raises(NotImplementedError, match="FILTER_NEIGHBOR_WITH_ROI"):
        pfe.VoxelSetAbstraction(dict(sr.SHIPPED_PFE, SA_LAYER=sa), sr.SHIPPED_PFE["VOXEL_SIZE"], sr.SHIPPED_PFE["POINT_CLOUD_RANGE"],
                                num_bev_features=256, num_rawpoint_features=4)
    head = roi_heads.PVRCNNHead(32, sr.head_cfg(), num_class=1).eval()
    h = sr.head_inputs()
    bd = {"batch_size": 2, "rois": torch.from_numpy(h["rois"]), "point_coords": torch.from_numpy(h["point_coords"]),
          "point_features": torch.from_numpy(h["point_features"])}
    with pytest.raises(KeyError, match="point_cls_scores"):
        head(bd)
    with pytest.raises(NotImplementedError, match="NMS_PRE_MAXSIZE = 9000"):                      # the TRAIN proposals stay refused
        head.proposal_layer({"batch_size": 1, "batch_box_preds": torch.zeros(1, 4, 7), "batch_cls_preds": torch.zeros(1, 4, 1)},
                            sr.SHIPPED_HEAD["NMS_CONFIG"]["TRAIN"])


def test_state_dicts_of_the_shipped_config():
    from dualfusion import pfe, roi_heads
    from dualfusion import pointnet2_stack as ps
    layer = ps.StackSAModuleMSG(radii=[0.8, 1.2], nsamples=[16, 32], mlps=[[32, 32, 32], [32, 32, 32]])
    sd = {k: tuple(v.shape) for k, v in layer.state_dict().items()}
    for k in range(2):
        assert sd["mlps.%d.0.weight" % k] == (32, 35, 1, 1) and sd["mlps.%d.3.weight" % k] == (32, 32, 1, 1)
        assert sd["mlps.%d.1.running_var" % k] == (32,) and sd["mlps.%d.4.bias" % k] == (32,)
        assert sd["mlps.%d.4.num_batches_tracked" % k] == ()
    assert len(sd) == 2 * 12 and not any("groupers" in k for k in sd)
    assert isinstance(layer.mlps[0][0], torch.nn.Conv2d) and isinstance(layer.mlps[0][1], torch.nn.BatchNorm2d)
    assert (layer.groupers[1].radius, layer.groupers[1].nsample, layer.groupers[1].use_xyz) == (1.2, 32, True)
    assert float(layer.mlps[0][1].weight.detach().min()) == 1.0 and float(layer.mlps[1][4].bias.detach().abs().max()) == 0.0
    cfg = sr.SHIPPED_PFE
    before = repr(cfg)
    vsa = pfe.VoxelSetAbstraction(cfg, cfg["VOXEL_SIZE"], cfg["POINT_CLOUD_RANGE"], num_bev_features=256, num_rawpoint_features=4)
    assert repr(cfg) == before                                   # the config is not edited (the reference prepends to MLPS)
    assert vsa.num_point_features_before_fusion == 256 + 32 * 2 + 64 + 128 + 128 == 640 and vsa.num_point_features == 128
    sd = {k: tuple(v.shape) for k, v in vsa.state_dict().items()}
    assert sd["SA_rawpoints.mlps.0.0.weight"] == (16, 4, 1, 1) and sd["SA_rawpoints.mlps.1.3.weight"] == (16, 16, 1, 1)
    for k, (cin, c) in enumerate(((16, 16), (32, 32), (64, 64), (64, 64))):
        assert sd["SA_layers.%d.mlps.0.0.weight" % k] == (c, cin + 3, 1, 1) and sd["SA_layers.%d.mlps.1.4.running_mean" % k] == (c,)
    assert sd["vsa_point_feature_fusion.0.weight"] == (128, 640) and sd["vsa_point_feature_fusion.1.running_var"] == (128,)
    assert "vsa_point_feature_fusion.0.bias" not in sd
    assert vsa.SA_layer_names == ["x_conv1", "x_conv2", "x_conv3", "x_conv4"] and vsa.downsample_times_map["x_conv4"] == 8
    head = roi_heads.PVRCNNHead(128, sr.SHIPPED_HEAD, num_class=1)
    sd = {k: tuple(v.shape) for k, v in head.state_dict().items()}
    assert sd["roi_grid_pool_layer.mlps.0.0.weight"] == (64, 131, 1, 1) and sd["roi_grid_pool_layer.mlps.1.3.weight"] == (64, 64, 1, 1)
    assert sd["shared_fc_layer.0.weight"] == (256, 216 * 128, 1) and sd["shared_fc_layer.1.running_mean"] == (256,)
    assert sd["shared_fc_layer.4.weight"] == (256, 256, 1)       # Conv1d, BN, ReLU, Dropout, Conv1d
    assert [type(m).__name__ for m in head.shared_fc_layer] == ["Conv1d", "BatchNorm1d", "ReLU", "Dropout", "Conv1d", "BatchNorm1d", "ReLU"]
    assert [type(m).__name__ for m in head.cls_layers] == ["Conv1d", "BatchNorm1d", "ReLU", "Dropout", "Conv1d", "BatchNorm1d", "ReLU", "Conv1d"]
    assert sd["cls_layers.7.weight"] == (1, 256, 1) and sd["cls_layers.7.bias"] == (1,)
    assert sd["reg_layers.7.weight"] == (7, 256, 1) and sd["reg_layers.7.bias"] == (7,)
    assert float(head.reg_layers[-1].weight.detach().std()) < 2e-3 < float(head.cls_layers[-1].weight.detach().std())
    assert isinstance(head, roi_heads.RoIHeadTemplate) and issubclass(roi_heads.VoxelRCNNHead, roi_heads.RoIHeadTemplate)
    assert roi_heads.PVRCNNHead.get_loss is roi_heads.VoxelRCNNHead.get_loss is roi_heads.RoIHeadTemplate.get_loss
    assert roi_heads.PVRCNNHead.forward_train is roi_heads.VoxelRCNNHead.forward_train


def test_state_dict_names_equal_the_reference_modules(golden):
    """the names and shapes the reference's own VoxelSetAbstraction and PVRCNNHead had when the fixture was made"""
    from dualfusion import pfe, roi_heads
    g = golden("vsa.npz")
    cfg = sr.vsa_cfg()
    vsa = pfe.VoxelSetAbstraction(cfg, sr.VSA_VOXEL, sr.VSA_RANGE, num_bev_features=sr.VSA_BEV[0], num_rawpoint_features=4)
    assert ["%s %s" % (k, tuple(v.shape)) for k, v in sorted(vsa.state_dict().items())] == g["vsa__sd_shapes"].tolist()
    head = roi_heads.PVRCNNHead(32, sr.head_cfg(), num_class=1)
    assert ["%s %s" % (k, tuple(v.shape)) for k, v in sorted(head.state_dict().items())] == g["head__sd_shapes"].tolist()
    vsa.load_state_dict(sr.torch_state(sr.vsa_state(cfg)), strict=True)


def test_registries_and_the_shim():
    from dualfusion import ext, pfe, roi_heads
    from dualfusion import registry as R
    assert R.PFE.get("VoxelSetAbstraction") is pfe.VoxelSetAbstraction
    assert R.ROI_HEADS.get("PVRCNNHead") is roi_heads.PVRCNNHead and R.ROI_HEADS.get("VoxelRCNNHead") is roi_heads.VoxelRCNNHead
    saved = dict(sys.modules)
    try:
        for k in [k for k in sys.modules if k.split(".")[0] == "pcdet"]:
            del sys.modules[k]
        for n in ("pcdet", "pcdet.models", "pcdet.models.backbones_3d", "pcdet.models.backbones_3d.pfe", "pcdet.models.roi_heads"):
            sys.modules[n] = types.ModuleType(n)
            sys.modules[n].__path__ = []
        sys.modules["pcdet"].models = sys.modules["pcdet.models"]
        sys.modules["pcdet.models"].backbones_3d = sys.modules["pcdet.models.backbones_3d"]
        sys.modules["pcdet.models"].roi_heads = sys.modules["pcdet.models.roi_heads"]
        sys.modules["pcdet.models.backbones_3d"].pfe = sys.modules["pcdet.models.backbones_3d.pfe"]
        sys.modules["pcdet.models.backbones_3d"].__all__ = {}
        sys.modules["pcdet.models.backbones_3d.pfe"].__all__ = {"VoxelSetAbstraction": object}
        sys.modules["pcdet.models.roi_heads"].__all__ = {}
        done = R.late_register()
        assert "pcdet.models.backbones_3d.pfe" in done and "pcdet.roi_heads" in done
        assert sys.modules["pcdet.models.backbones_3d.pfe"].__all__["VoxelSetAbstraction"] is pfe.VoxelSetAbstraction
        assert sys.modules["pcdet.models.roi_heads"].__all__["PVRCNNHead"] is roi_heads.PVRCNNHead
    finally:
        for k in list(sys.modules):
            if k not in saved and k.split(".")[0] == "pcdet":
                del sys.modules[k]
        sys.modules.update({k: v for k, v in saved.items() if k.split(".")[0] == "pcdet"})
    mod = ext.load("pointnet2_stack_cuda")
    assert callable(mod.ball_query_wrapper) and "ball query" in mod.__doc__ and "not provided" in mod.__doc__
    import inspect
    assert list(inspect.signature(mod.ball_query_wrapper).parameters) == [
        "B", "M", "radius", "nsample", "new_xyz_tensor", "new_xyz_batch_cnt_tensor", "xyz_tensor", "xyz_batch_cnt_tensor", "idx_tensor"]
    with pytest.raises(RuntimeError, match="CUDA tensor"):           # CPU tensors: a RuntimeError like pybind's
        mod.ball_query_wrapper(1, 2, 0.5, 4, torch.zeros(2, 3), torch.tensor([2], dtype=torch.int32), torch.zeros(5, 3),
                               torch.tensor([5], dtype=torch.int32), torch.zeros(2, 4, dtype=torch.int32))


def test_ball_query_restatement_equals_brute_force_and_covers_its_cases():
    fx = sr.ball_fixture()
    assert sr.near_boundary(fx["radius"], fx["xyz"], fx["xyz_cnt"], fx["new_xyz"], fx["new_cnt"]) == 0
    for ns in (16, 32):
        idx, found = sr.ball_query_kernel(fx["radius"], ns, fx["xyz"], fx["xyz_cnt"], fx["new_xyz"], fx["new_cnt"])
        starts, frames = sr.frame_starts(fx["xyz_cnt"]), sr.frame_of_rows(fx["new_cnt"])
        for m in range(len(idx)):                                # the reference's loop, row by row in float64-free float32
            want, cnt = np.zeros(ns, np.int32), 0
            for k in range(fx["xyz_cnt"][frames[m]]):
                d = fx["new_xyz"][m] - fx["xyz"][starts[frames[m]] + k]
                d2 = np.float32(np.float32(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
                if d2 < np.float32(np.float32(fx["radius"]) * np.float32(fx["radius"])):
                    if cnt == 0:
                        want[:] = k
                    want[cnt] = k
                    cnt += 1
                    if cnt >= ns:
                        break
            if cnt == 0:
                want[0] = -1
            assert np.array_equal(idx[m], want), m
        assert (found[5:8] == 0).all()                           # the frame with no rows: only empty balls
        assert found[fx["far"]] == 0 and found[fx["dense"]] > ns # nearest rows in the neighbouring frame; an overfull ball
        assert ((found > 0) & (found < ns)).sum() >= 3
    big = sr.big_ball_fixture()
    assert sr.near_boundary(big["radius"], big["xyz"], big["xyz_cnt"], big["new_xyz"], big["new_cnt"]) == 0
    _, found = sr.ball_query_kernel(big["radius"], 16, big["xyz"], big["xyz_cnt"], big["new_xyz"], big["new_cnt"])
    assert (found > 16).sum() >= 20 and (found < 16).sum() >= 10


def test_restatement_equals_the_reference_outputs(golden):
    g = golden("vsa.npz")
    inputs = sr.vsa_inputs()
    for tag in ("raw_points", "voxel_centers"):
        cfg = sr.vsa_cfg(tag)
        kp, before, fused = sr.vsa_forward(sr.torch_state(sr.vsa_state(cfg)), cfg, inputs)
        assert np.array_equal(kp, g["vsa__%s__keypoints" % tag])
        assert np.abs(fused.numpy() - g["vsa__%s__point_features" % tag]).max() < 1e-10 * np.abs(g["vsa__%s__point_features" % tag]).max()
        if tag == "raw_points":
            assert np.abs(before.numpy() - g["vsa__raw_points__before_fusion"]).max() < 1e-10 * np.abs(g["vsa__raw_points__before_fusion"]).max()
    # frame 1 has 50 points for 64 keypoints: the sampled order repeats
    kp = g["vsa__raw_points__keypoints"]
    assert np.array_equal(kp[64:64 + 14, 1:], kp[64 + 50:, 1:]) and len(np.unique(kp[:64], axis=0)) == 64
    assert np.array_equal(sr.pad_keypoints(np.arange(5), 12), [0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 0, 1])
    h, cfg = sr.head_inputs(), sr.head_cfg()
    pooled = sr.pvrcnn_grid_pool(sr.torch_state(sr.head_pool_state(cfg)), cfg["ROI_GRID_POOL"], h["rois"], h["point_coords"],
                                 h["point_features"], h["point_cls_scores"])
    assert np.abs(pooled.numpy() - g["head__pooled"]).max() < 1e-10 * np.abs(g["head__pooled"]).max()
    assert (h["rois"][1, 2] == 0).all()                          # the padding RoI: 216 grid points at the origin


def test_bilinear_restatement_weights_come_from_the_clamped_corners():
    """voxel_set_abstraction.py:27-40: outside the map floor(x) and floor(x) + 1 clamp to the same column and the weights cancel"""
    im = torch.arange(7 * 5 * 2, dtype=torch.float64).view(7, 5, 2)
    x = torch.tensor([1.25, -0.5, 2.0, 4.5], dtype=torch.float64)
    y = torch.tensor([2.5, 3.0, 7.25, 1.0], dtype=torch.float64)
    out = sr.bilinear_sample(im, x, y)
    assert torch.allclose(out[0], 0.75 * 0.5 * im[2, 1] + 0.75 * 0.5 * im[3, 1] + 0.25 * 0.5 * im[2, 2] + 0.25 * 0.5 * im[3, 2])
    assert torch.equal(out[1], torch.zeros(2, dtype=torch.float64)) and torch.equal(out[2], torch.zeros(2, dtype=torch.float64))
    assert torch.equal(out[3], torch.zeros(2, dtype=torch.float64))


def test_the_switch_is_read_per_call(monkeypatch):
    from dualfusion import pointnet2_stack as ps
    monkeypatch.delenv("DF3D_STACK_SA_FUSED", raising=False)
    assert ps.stack_sa_fused_enabled()
    monkeypatch.setenv("DF3D_STACK_SA_FUSED", "0")
    assert not ps.stack_sa_fused_enabled()
    monkeypatch.setenv("DF3D_STACK_SA_FUSED", "1")
    assert ps.stack_sa_fused_enabled()
    layer = ps.StackSAModuleMSG(radii=[0.8], nsamples=[16], mlps=[[16, 16, 16]]).eval()
    with torch.no_grad():
        assert not layer.takes_fused(0, torch.zeros(4, 3))       # host tensors never take the kernel
