"""The Voxel-RCNN tail without a GPU: parameter names and shapes of AnchorHeadSingle, BaseBEVBackbone and HeightCompression
against the shipped car config; anchors and shift tables bit-equal to the reference's (tests/golden/vr_tail.npz); the float64
restatement of tests/vrtail_reference.py against the golden within float32 rounding; every refusal; the retained KeyError;
registry lookups; argument errors of the two C entry points."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import vrtail_reference as vt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["df3d_anchor_proposals_workspace_bytes", "df3d_anchor_proposals", "df3d_roi_decode_select_workspace_bytes",
           "df3d_roi_decode_select"]
KITTI_RANGE = [0, -40, -3, 70.4, 40, 1]
KITTI_GRID = np.array([1408, 1600, 40])
BEV_CFG = {"NAME": "BaseBEVBackbone", "LAYER_NUMS": [5, 5], "LAYER_STRIDES": [1, 2], "NUM_FILTERS": [64, 128],
           "UPSAMPLE_STRIDES": [1, 2], "NUM_UPSAMPLE_FILTERS": [128, 128]}


@pytest.fixture(scope="module")
def g(golden):
    return golden("vr_tail.npz")


def build_head(name, **edit):
    from dualfusion import dense_heads
    cfg = copy.deepcopy(vt.head_cfg(name))
    cfg.update(edit)
    grid, rng = vt.case_geometry(name)
    c = vt.CASES[name]
    return dense_heads.AnchorHeadSingle(cfg, 16, c["C"], [s["class_name"] for s in c["sets"]], grid, rng)


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
    assert "proposals.hip" in ge._load(os.path.join(ge.PKG, "csrc", "build.py"), "df3d_build").SOURCES


def test_argument_errors_are_reported_without_a_gpu():
    from dualfusion import _lib, ops
    lib = _lib.bind(ctypes.CDLL(_lib.LIB_PATH), check=False)
    byref = ctypes.byref
    assert lib.df3d_anchor_proposals(None, 0, None, 0, None, 0, None, None, None, None, None, None, None, None, 0, None) == -1
    assert b"anchor_proposals: null config" in lib.df3d_last_error()
    table = [[-1.0, 3.9, 1.6, 1.56, 0.0], [-1.0, 3.9, 1.6, 1.56, 1.57]]
    cfg = ops.anchor_cfg(2, 25, 22, 1, 2, [0, 0], table, 1, 0.78539, 0.0, 0.7, 256, 32)
    assert lib.df3d_anchor_proposals_workspace_bytes(byref(cfg)) > 0
    assert lib.df3d_anchor_proposals(None, 2, None, 14, None, 4, None, None, byref(cfg), None, None, None, None, None, 0, None) == -1
    assert b"anchor_proposals: null input" in lib.df3d_last_error()
    one = (ctypes.c_float * 64)()
    buf = ctypes.cast(one, ctypes.c_void_p)
    call = lambda c, ld_cls=2, ld_box=14, ws=1 << 30: lib.df3d_anchor_proposals(buf, ld_cls, buf, ld_box, buf, 4, buf, buf, byref(c), buf,
                                                                                 buf, buf, buf, buf, ws, None)
    assert call(cfg, ld_cls=1) == -1 and b"row stride is smaller" in lib.df3d_last_error()
    assert call(cfg, ld_box=13) == -1 and b"row stride is smaller" in lib.df3d_last_error()
    assert call(cfg, ws=16) == -1 and b"workspace 16 <" in lib.df3d_last_error()
    big = ops.anchor_cfg(2, 25, 22, 1, 2, [0, 0], table, 1, 0.78539, 0.0, 0.7, 9000, 512)
    assert lib.df3d_anchor_proposals_workspace_bytes(byref(big)) == 0
    assert call(big) == -1 and b"NMS_PRE_MAXSIZE <= 4096 (got 9000)" in lib.df3d_last_error()
    bad_set = ops.anchor_cfg(2, 25, 22, 1, 2, [0, 1], table, 1, 0.78539, 0.0, 0.7, 256, 32)
    assert call(bad_set) == -1 and b"names set 1 of 1" in lib.df3d_last_error()
    many = ops.anchor_cfg(256, 25, 22, 1, 2, [0, 0], table, 1, 0.78539, 0.0, 0.7, 256, 32)
    assert call(many) == -1 and b"at most 255 frames" in lib.df3d_last_error()
    wide = ops.anchor_cfg(1, 4096, 2048, 1, 2, [0, 0], table, 1, 0.78539, 0.0, 0.7, 256, 32)
    assert call(wide) == -1 and b"at most 2^22 anchors per frame" in lib.df3d_last_error()
    with pytest.raises(NotImplementedError, match="at most 32 anchors"):
        ops.anchor_cfg(1, 4, 4, 1, 2, [0] * 33, [table[0]] * 33, 1, 0.0, 0.0, 0.7, 256, 32)

    assert lib.df3d_roi_decode_select(None, None, 1, None, 7, None, None, None, None, None, None, None, None, 0, None) == -1
    assert b"roi_decode_select: null config" in lib.df3d_last_error()
    rc = ops._RoiDecodeCfg(3, 32, 1, 0.3, 0.1, 4096, 100, 0)
    assert lib.df3d_roi_decode_select_workspace_bytes(byref(rc)) > 0
    assert lib.df3d_roi_decode_select(None, None, 1, None, 7, None, byref(rc), None, None, None, None, None, None, 0, None) == -1
    assert b"roi_decode_select: null input" in lib.df3d_last_error()
    rcall = lambda c, ld_reg=7, ws=1 << 30: lib.df3d_roi_decode_select(buf, buf, 1, buf, ld_reg, None, byref(c), buf, buf, buf, buf, buf,
                                                                       buf, ws, None)
    assert rcall(rc, ld_reg=6) == -1 and b"row stride is smaller" in lib.df3d_last_error()
    assert rcall(rc, ws=16) == -1 and b"workspace 16 <" in lib.df3d_last_error()
    assert rcall(ops._RoiDecodeCfg(3, 4097, 1, 0.3, 0.1, 4096, 100, 0)) == -1 and b"RoIs per frame <= 4096 (got 4097)" in lib.df3d_last_error()
    assert rcall(ops._RoiDecodeCfg(3, 32, 1, 0.3, 0.1, 9000, 100, 0)) == -1 and b"NMS_PRE_MAXSIZE <= 4096 (got 9000)" in lib.df3d_last_error()
    # the product ops refuse CPU tensors
    with pytest.raises(_lib.Df3dError):
        ops.anchor_proposals(torch.zeros(8, 2), torch.zeros(8, 14), None, torch.zeros(1, 4), torch.zeros(1, 2), 1, 2, 4, 1, [0, 0],
                             table, 0.7, 256, 32)
    with pytest.raises(_lib.Df3dError):
        ops.roi_decode_select(torch.zeros(1, 4, 7), torch.zeros(4, 1), torch.zeros(4, 7), None, 0.3, 0.1, 4096, 100)


def test_parameter_names_and_shapes_of_the_car_config():
    from dualfusion import dense_heads
    from dualfusion.registry import BACKBONES_2D, DENSE_HEADS, DETECTORS_PCDET, MAP_TO_BEV, late_register
    from dualfusion import vr_detector
    assert DENSE_HEADS.get("AnchorHeadSingle") is dense_heads.AnchorHeadSingle
    assert BACKBONES_2D.get("BaseBEVBackbone") is dense_heads.BaseBEVBackbone
    assert MAP_TO_BEV.get("HeightCompression") is dense_heads.HeightCompression
    assert DETECTORS_PCDET.get("VoxelRCNN") is vr_detector.VoxelRCNN
    late_register()                                                # pcdet absent: nothing to mirror into, no error
    bev = dense_heads.BaseBEVBackbone(BEV_CFG, 256)
    sd = {k: tuple(v.shape) for k, v in bev.state_dict().items()}
    assert bev.num_bev_features == 256
    assert sd["blocks.0.1.weight"] == (64, 256, 3, 3) and sd["blocks.0.2.running_var"] == (64,)
    assert sd["blocks.0.16.weight"] == (64, 64, 3, 3) and "blocks.0.19.weight" not in sd           # pad, conv, bn, relu + 5 x 3
    assert sd["blocks.1.1.weight"] == (128, 64, 3, 3) and sd["blocks.1.17.weight"] == (128,)
    assert sd["deblocks.0.0.weight"] == (64, 128, 1, 1) and sd["deblocks.1.0.weight"] == (128, 128, 2, 2)
    assert sd["deblocks.1.1.bias"] == (128,)
    assert bev.blocks[0][2].eps == 1e-3 and bev.blocks[0][2].momentum == 0.01 and isinstance(bev.blocks[0][0], torch.nn.ZeroPad2d)
    assert bev.blocks[0][1].bias is None and bev.deblocks[1][0].bias is None and bev.blocks[1][1].stride == (2, 2)
    with torch.no_grad():
        out = bev.eval()({"spatial_features": torch.zeros(1, 256, 8, 6)})
    assert tuple(out["spatial_features_2d"].shape) == (1, 256, 8, 6)
    hc = dense_heads.HeightCompression({"NAME": "HeightCompression", "NUM_BEV_FEATURES": 256})
    assert hc.num_bev_features == 256 and len(hc.state_dict()) == 0

    class Dense(object):
        def dense(self):
            return torch.arange(2 * 3 * 2 * 4 * 5, dtype=torch.float32).view(2, 3, 2, 4, 5)
    bd = hc({"encoded_spconv_tensor": Dense(), "encoded_spconv_tensor_stride": 8})
    assert tuple(bd["spatial_features"].shape) == (2, 6, 4, 5) and bd["spatial_features_stride"] == 8
    assert torch.equal(bd["spatial_features"][1, 3], Dense().dense()[1, 1, 1])

    cfg = copy.deepcopy(vt.head_cfg("car"))
    head = dense_heads.AnchorHeadSingle(cfg, 256, 1, ["Car"], KITTI_GRID, KITTI_RANGE)
    assert cfg == vt.head_cfg("car")
    sd = {k: tuple(v.shape) for k, v in head.state_dict().items()}
    assert sd == {"conv_cls.weight": (2, 256, 1, 1), "conv_cls.bias": (2,), "conv_box.weight": (14, 256, 1, 1), "conv_box.bias": (14,),
                  "conv_dir_cls.weight": (4, 256, 1, 1), "conv_dir_cls.bias": (4,)}
    assert tuple(head.anchors.shape) == (1, 200, 176, 1, 2, 7) and head.num_anchors_per_location == 2
    assert np.allclose(head.conv_cls.bias.detach().numpy(), -np.log(99.0)) and float(head.conv_box.weight.std()) < 2e-3
    no_dir = dense_heads.AnchorHeadSingle(vt.head_cfg("nodir"), 256, 1, ["Car"], KITTI_GRID, KITTI_RANGE)
    assert no_dir.conv_dir_cls is None and sorted(no_dir.state_dict()) == ["conv_box.bias", "conv_box.weight", "conv_cls.bias",
                                                                           "conv_cls.weight"]
    with pytest.raises(NotImplementedError, match="eval mode only"):
        head.train()({"spatial_features_2d": torch.zeros(1, 256, 200, 176), "batch_size": 1})


@pytest.mark.parametrize("name", ["car", "small", "multi"])
def test_anchors_and_shift_tables_are_bit_equal_to_the_reference(g, name):
    head = build_head(name)
    want = g[name + "_anchors"]
    assert head.anchors.dtype == torch.float32 and tuple(head.anchors.shape) == want.shape
    assert np.array_equal(head.anchors.numpy().view(np.uint32), want.view(np.uint32))
    t, c = head.tables, vt.CASES[name]
    A = t.num_anchors_per_location
    assert A == 2 * len(c["sets"]) and (t.H, t.W) == (c["H"], c["W"])
    flat = want.reshape(c["H"], c["W"], A, 7)
    for a in range(A):
        s = t.anchor_set[a]
        assert s == a // 2
        assert np.array_equal(t.x_shifts[s].numpy(), flat[0, :, a, 0]) and np.array_equal(t.y_shifts[s].numpy(), flat[:, 0, a, 1])
        assert np.array_equal(t.table[a].numpy(), flat[3, 2, a, 2:])
    if name == "multi":                                            # align_center moves the pedestrian set by half a cell
        assert not np.array_equal(t.x_shifts[0].numpy(), t.x_shifts[1].numpy()) and np.array_equal(t.x_shifts[0].numpy(), t.x_shifts[2].numpy())


def bound(want):
    return 8 * vt.U32 * np.abs(want).max()


@pytest.mark.parametrize("name", ["car", "small", "multi", "nodir"])
def test_float64_restatement_against_the_reference(g, name):
    c = vt.CASES[name]
    src = "car" if name == "nodir" else name
    cls, box, dirs = g[src + "_cls"], g[src + "_box"], g[src + "_dir"] if c["NB"] else None
    anchors = g[src + "_anchors"].reshape(-1, 7)
    dense, dist = vt.dense_decode(box, dirs, anchors, vt.DIR_OFFSET, vt.DIR_LIMIT_OFFSET)
    want = g[name + "_dense"]
    if dist is not None:                                           # an anchor whose floor argument rounds the other way is off by
        ok = dist >= vt.FLOOR_MARGIN                               # a period: compared where the margin holds (all selected ones do)
        assert ok.mean() > 0.99
        assert np.abs(dense - want)[ok].max() <= bound(want)
    else:
        assert np.abs(dense - want).max() <= bound(want)
    ref = vt.proposals(cls, box, dirs, anchors, c["pre"], c["post"], c["thresh"], vt.DIR_OFFSET, vt.DIR_LIMIT_OFFSET)
    assert ref["min_gap"] > 0 and ref["close"] == 0 and (dirs is None or ref["floor_dist"] >= vt.FLOOR_MARGIN)
    assert np.abs(ref["rois"] - g[name + "_rois"]).max() <= bound(g[name + "_rois"])
    assert np.array_equal(ref["roi_scores"].astype(np.float32), g[name + "_roi_scores"])
    assert np.array_equal(ref["roi_labels"], g[name + "_roi_labels"])
    picked = np.where(ref["index"][..., None] >= 0, want[np.arange(c["B"])[:, None], np.maximum(ref["index"], 0)], 0)
    assert np.array_equal(picked, g[name + "_rois"])               # the same anchors, slot by slot; zeros and label 1 after them
    assert (g[name + "_roi_labels"][ref["index"] < 0] == 1).all()


@pytest.mark.parametrize("name,raw", [("car", False), ("car", True), ("multi", False)])
def test_float64_roi_decode_and_selection_against_the_reference(g, name, raw):
    rois, rcnn_cls, rcnn_reg = g[name + "_rois"], g[name + "_rcnn_cls"], g[name + "_rcnn_reg"]
    box_preds = vt.roi_decode(rois, rcnn_reg)
    assert np.abs(box_preds - g[name + "_box_preds"]).max() <= bound(g[name + "_box_preds"])
    labels = g[name + "_roi_labels"] if vt.CASES[name]["C"] > 1 else None
    fin = vt.final_select(box_preds, rcnn_cls, labels, vt.FINAL["score_thresh"], vt.FINAL["thresh"], vt.FINAL["pre"],
                          vt.FINAL["post"], raw_score=raw)
    tag = name + ("_raw" if raw else "")
    assert fin["min_gap"] > 0 and fin["close"] == 0 and fin["thresh_dist"] >= 1e-4
    assert np.array_equal(fin["counts"], g[tag + "_final_counts"])
    assert np.array_equal(fin["labels"], g[tag + "_final_labels"])
    assert np.abs(fin["boxes"] - g[tag + "_final_boxes"]).max() <= bound(g[tag + "_final_boxes"])
    assert np.abs(fin["scores"] - g[tag + "_final_scores"]).max() <= bound(g[tag + "_final_scores"])
    picked = np.where(fin["index"][..., None] >= 0, g[name + "_box_preds"][np.arange(len(rois))[:, None], np.maximum(fin["index"], 0)], 0)
    assert np.array_equal(picked, g[tag + "_final_boxes"])
    if name == "car":
        assert fin["counts"][1] == 0                               # the frame where nothing passes SCORE_THRESH
        zero = np.abs(rois).sum(-1) == 0                           # zero-padded RoIs are decoded and may be selected
        assert zero[2].sum() == 16 and zero[2][fin["index"][2][fin["index"][2] >= 0]].any()


def test_limits_are_refused_by_name():
    from dualfusion import dense_heads, roi_heads, vr_detector
    sets = vt.CASES["multi"]["sets"]
    with pytest.raises(NotImplementedError, match="USE_MULTIHEAD"):
        build_head("car", USE_MULTIHEAD=True)
    with pytest.raises(NotImplementedError, match="encode_angle_by_sincos"):
        build_head("car", TARGET_ASSIGNER_CONFIG={"BOX_CODER": "ResidualCoder", "BOX_CODER_CONFIG": {"encode_angle_by_sincos": True}})
    with pytest.raises(NotImplementedError, match="PreviousResidualDecoder"):
        build_head("car", TARGET_ASSIGNER_CONFIG={"BOX_CODER": "PreviousResidualDecoder"})
    with pytest.raises(NotImplementedError, match="anchor_bottom_heights"):
        build_head("car", ANCHOR_GENERATOR_CONFIG=[dict(vt.CAR, anchor_bottom_heights=[-1.78, -1.0])])
    with pytest.raises(NotImplementedError, match="feature-map sizes differ"):
        build_head("multi", ANCHOR_GENERATOR_CONFIG=[sets[0], dict(sets[1], feature_map_stride=4)])
    check = roi_heads.VoxelRCNNHead.check_nms_config
    with pytest.raises(NotImplementedError, match="MULTI_CLASSES_NMS"):
        check(dict(vt.nms_cfg("car"), MULTI_CLASSES_NMS=True), "proposal_layer")
    with pytest.raises(NotImplementedError, match="NMS_PRE_MAXSIZE = 9000 exceeds 4096"):
        check({"NMS_TYPE": "nms_gpu", "MULTI_CLASSES_NMS": False, "NMS_PRE_MAXSIZE": 9000, "NMS_POST_MAXSIZE": 512,
               "NMS_THRESH": 0.8}, "proposal_layer")
    assert check(vt.nms_cfg("car"), "proposal_layer") == (256, 32, 0.7)
    multi = vt.post_cfg()
    multi["NMS_CONFIG"]["MULTI_CLASSES_NMS"] = True
    with pytest.raises(NotImplementedError, match="MULTI_CLASSES_NMS"):
        vr_detector.post_processing({"batch_size": 1}, multi)
    with pytest.raises(NotImplementedError, match="RoIs per frame exceed 4096"):
        vr_detector.final_selection({"batch_size": 1, "rois": torch.zeros(1, 4097, 7)}, vt.post_cfg())


def test_head_without_rois_or_dense_outputs_keeps_its_key_error():
    import roipool_reference as rp
    from dualfusion import roi_heads
    cfg = dict(rp.HEAD_CFG)                                        # no NMS_CONFIG: read only when proposals are made
    assert "NMS_CONFIG" not in cfg
    head = roi_heads.VoxelRCNNHead(rp.BACKBONE_CHANNELS, cfg, rp.KITTI_RANGE, rp.KITTI_VOXEL, num_class=1).eval()
    with pytest.raises(KeyError, match="rois"):
        head({"batch_size": 1})
    with pytest.raises(KeyError, match="rois.*NMS_CONFIG"):       # dense outputs, but nothing to make proposals with
        head({"batch_size": 1, "batch_box_preds": torch.zeros(1, 4, 7), "batch_cls_preds": torch.zeros(1, 4, 1)})
    given = {"batch_size": 1, "rois": torch.zeros(1, 2, 7)}
    assert head.proposal_layer(given, vt.nms_cfg("car")) is given and sorted(given) == ["batch_size", "rois"]


def test_composed_decode_on_the_cpu_matches_the_reference_bit_for_bit(g, monkeypatch):
    """The composed mode is the reference's own sequence of torch operations: on the same device it gives the same bits."""
    monkeypatch.setenv("DF3D_VR_TAIL_FUSED", "0")
    for name in ("car", "multi", "nodir"):
        c = vt.CASES[name]
        src = "car" if name == "nodir" else name
        head = build_head(name).eval()
        view = lambda v: torch.from_numpy(v).view(c["B"], c["H"], c["W"], -1)
        with torch.no_grad():
            cls_preds, box_preds = head.generate_predicted_boxes(c["B"], view(g[src + "_cls"]), view(g[src + "_box"]),
                                                                 view(g[src + "_dir"]) if c["NB"] else None)
        assert np.array_equal(box_preds.numpy(), g[name + "_dense"])
        assert np.array_equal(cls_preds.numpy(), g[src + "_cls"])
    from dualfusion import roi_heads
    import roipool_reference as rp
    rh = roi_heads.VoxelRCNNHead(rp.BACKBONE_CHANNELS, rp.HEAD_CFG, rp.KITTI_RANGE, rp.KITTI_VOXEL, num_class=1).eval()
    with torch.no_grad():
        _, got = rh.generate_predicted_boxes(3, torch.from_numpy(g["car_rois"]), torch.from_numpy(g["car_rcnn_cls"]),
                                             torch.from_numpy(g["car_rcnn_reg"]))
    assert np.array_equal(got.numpy(), g["car_box_preds"])


def test_detector_builds_the_chain_from_the_car_config():
    import roipool_reference as rp
    from dualfusion import backbones, dense_heads, roi_heads, vr_detector
    roi_cfg = dict(rp.HEAD_CFG, NMS_CONFIG={"TEST": vt.nms_cfg("car")})
    cfg = {"NAME": "VoxelRCNN", "BACKBONE_3D": {"NAME": "VoxelBackBone8x"},
           "MAP_TO_BEV": {"NAME": "HeightCompression", "NUM_BEV_FEATURES": 256}, "BACKBONE_2D": BEV_CFG,
           "DENSE_HEAD": vt.head_cfg("car"), "ROI_HEAD": roi_cfg, "POST_PROCESSING": vt.post_cfg()}
    model = vr_detector.VoxelRCNN(cfg, 1, ["Car"], KITTI_GRID, KITTI_RANGE, [0.05, 0.05, 0.1])
    kinds = [type(m) for m in model.module_list]
    assert kinds == [backbones.VoxelBackBone8x, dense_heads.HeightCompression, dense_heads.BaseBEVBackbone,
                     dense_heads.AnchorHeadSingle, roi_heads.VoxelRCNNHead]
    names = set(k.split(".")[0] for k in model.state_dict())
    assert names == {"backbone_3d", "backbone_2d", "dense_head", "roi_head"}
    assert model.dense_head.conv_cls.in_channels == 256 and model.roi_head.post_process_cfg is cfg["POST_PROCESSING"]
    with pytest.raises(NotImplementedError, match="eval mode only"):
        model.train()({})
    with pytest.raises(KeyError, match="NoSuchHead"):
        vr_detector.VoxelRCNN(dict(cfg, DENSE_HEAD=dict(vt.head_cfg("car"), NAME="NoSuchHead")), 1, ["Car"], KITTI_GRID, KITTI_RANGE,
                              [0.05, 0.05, 0.1])
