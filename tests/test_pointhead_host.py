"""The PV-RCNN point head and detector without a GPU: the entry points of csrc/pointhead.hip are declared, exported and bound;
their argument errors and caps; the refusals of PointHeadSimple and PVRCNN; the registry entries and the pybind-name shim; the
float32 restatement of tests/pointhead_reference.py against the reference's results (tests/golden/point_head.npz) and against
a float64 brute force; the margins (near_face == 0) and the coverage of every fixture, checked on the reference alone; the
composed path on the CPU; the PVRCNN detector built from a config shaped like the shipped one."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import pointhead_reference as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["df3d_points_in_boxes", "df3d_point_head_targets", "df3d_point_cls_loss_workspace_bytes", "df3d_point_cls_loss",
           "df3d_point_cls_loss_grad"]
UPSTREAM = 2.5          # tests/golden/make_golden_pointhead.py


@pytest.fixture(scope="module")
def g(golden):
    return golden("point_head.npz")


@pytest.fixture(scope="module")
def cases():
    return {name: pr.target_case(name) for name in pr.TARGET_CASES}


def test_symbols_are_declared_exported_and_bound():
    import __graft_entry__ as ge
    build = ge._load(os.path.join(ge.PKG, "csrc", "build.py"), "df3d_build")
    build.build()
    from dualfusion import _lib, dense_heads, ops, vr_detector
    header = open(os.path.join(ROOT, "include", "df3d_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, header), s
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES, s
    assert "pointhead.hip" in build.SOURCES
    macros = dict(re.findall(r"#define (DF3D_POINT_HEAD_\w+) (\d+)", header))
    assert int(macros["DF3D_POINT_HEAD_MAX_GT"]) == ops.POINT_HEAD_MAX_GT >= 130
    assert int(macros["DF3D_POINT_HEAD_GT_CHUNK"]) == ops.POINT_HEAD_GT_CHUNK == 128
    for name in ("points_in_boxes", "point_head_targets", "point_cls_loss"):
        assert callable(getattr(ops, name)), name
    for name in ("PointHeadSimple", "composed_point_targets", "composed_point_cls_loss", "point_head_fused"):
        assert callable(getattr(dense_heads, name)), name
    assert callable(vr_detector.PVRCNN)
    # the focal term is shared: one definition, in loss_terms.h, used by both loss files
    csrc = os.path.join(ROOT, "3d-dual-fusion_amd", "csrc")
    text = {f: open(os.path.join(csrc, f)).read() for f in ("loss_terms.h", "anchorloss.hip", "pointhead.hip")}
    define = r"void focal\(double x, double tt"
    assert len(re.findall(define, text["loss_terms.h"])) == 1
    for f in ("anchorloss.hip", "pointhead.hip"):
        assert not re.search(define, text[f]) and "focal(" in text[f] and '#include "loss_terms.h"' in text[f], f


def test_argument_errors_and_caps_are_reported_without_a_gpu():
    from dualfusion import _lib, ops
    lib = _lib.bind(ctypes.CDLL(_lib.LIB_PATH), check=False)
    one = (ctypes.c_float * 64)()
    buf = ctypes.cast(one, ctypes.c_void_p)
    err = lambda: lib.df3d_last_error()
    assert lib.df3d_points_in_boxes(buf, buf, 70000, 4, 4, buf, None) == -1 and b"points_in_boxes: 0..65535 frames" in err()
    assert lib.df3d_points_in_boxes(buf, None, 1, 4, 4, buf, None) == -1 and b"points_in_boxes: null pointer" in err()
    assert lib.df3d_points_in_boxes(buf, buf, 1, 4, 0, buf, None) == 0                                   # nothing to do, no launch
    tg = lambda P=8, B=2, G=5, C=3, extra=buf, points=buf: lib.df3d_point_head_targets(points, P, buf, B, G, extra, C, buf, None, None)
    assert tg(G=ops.POINT_HEAD_MAX_GT + 1) == -1 and b"0..1024 ground-truth rows per frame" in err()
    assert tg(P=(1 << 24) + 1) == -1 and b"points (got" in err()
    assert tg(C=0) == -1 and b"num_class >= 1" in err()
    assert tg(extra=None) == -1 and b"null extra_width" in err()
    assert tg(points=None) == -1 and b"null pointer" in err()
    assert tg(P=0) == 0
    need = lib.df3d_point_cls_loss_workspace_bytes(513)
    assert need >= 3 * 2 * 8 and lib.df3d_point_cls_loss_workspace_bytes(-1) == 0
    loss = lambda P=513, C=3, ld=3, ws=need, out=buf: lib.df3d_point_cls_loss(buf, ld, buf, P, C, 1.0, out, buf, buf, buf, ws, None)
    assert loss(ws=need - 1) == -1 and b"workspace" in err()
    assert loss(ld=2) == -1 and b"ld >= num_class" in err()
    assert loss(C=65, ld=65) == -1 and b"1..64 classes" in err()
    assert loss(out=None) == -1 and b"null output" in err()
    grad = lambda P=513, C=3, ld=3, up=buf: lib.df3d_point_cls_loss_grad(buf, buf, up, P, C, 1.0, buf, ld, None)
    assert grad(ld=2) == -1 and b"ld_grad >= num_class" in err()
    assert grad(up=None) == -1 and b"null pointer" in err()
    assert grad(P=0) == 0

    # the Python layer: CPU tensors, shapes and the ground-truth cap, each by name
    pts, gt = torch.zeros((4, 4)), torch.zeros((1, 3, 8))
    with pytest.raises(_lib.Df3dError, match="must live on the GPU"):
        ops.point_head_targets(pts, gt, pr.EXTRA, 3)
    with pytest.raises(_lib.Df3dError, match="must live on the GPU"):
        ops.points_in_boxes(torch.zeros((1, 3, 7)), torch.zeros((1, 4, 3)))
    with pytest.raises(_lib.Df3dError, match="must live on the GPU"):
        ops.point_cls_loss(torch.zeros((4, 3)), torch.zeros((4,), dtype=torch.int64))


def test_the_shim_and_the_registries():
    from dualfusion import _lib, dense_heads, ext, registry, vr_detector
    assert "roiaware_pool3d_cuda" in ext.PCDET_NAMES
    assert ext.ALIASES["roiaware_pool3d_cuda"] == ("pcdet.ops.roiaware_pool3d.roiaware_pool3d_cuda",)
    mod = ext.load("roiaware_pool3d_cuda")
    assert callable(mod.points_in_boxes_gpu) and "not provided" in mod.__doc__
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        mod.points_in_boxes_gpu(torch.zeros((1, 3, 7)), torch.zeros((1, 4, 3)), torch.zeros((1, 4), dtype=torch.int32))
    assert "pcdet.ops.roiaware_pool3d.roiaware_pool3d_cuda" in [p for paths in ext.ALIASES.values() for p in paths]
    registry.late_register()
    assert registry.DENSE_HEADS.get("PointHeadSimple") is dense_heads.PointHeadSimple
    assert registry.DETECTORS_PCDET.get("PVRCNN") is vr_detector.PVRCNN
    assert registry.DETECTORS_PCDET.get("VoxelRCNN") is vr_detector.VoxelRCNN
    for name in ("AuxPointHeadSimple", "PointHeadBox", "PointIntraPartOffsetHead"):
        assert registry.DENSE_HEADS.get(name) is None, name


def test_fixtures_are_margin_clean_and_cover_every_case(cases):
    """on the reference alone: no pair near a face, every label value, every crafted row"""
    for name, (points, gt, extra) in cases.items():
        assert pr.near_face(points, gt, extra) == 0, name
    points, gt, extra = cases["main"]
    assert points.shape == (514, 4) and gt.shape == (2, 5, 8) and not gt[:, 3:].any() and np.abs(gt[:, :3, 3:6]).min() > 0
    assert [int((points[:, 0] == b).sum()) for b in range(3)] == [300, 213, 1]
    labels, idx, d = pr.assign_targets(points, gt, extra, 3, detail=True)
    assert sorted(np.unique(labels)) == [-1, 0, 1, 2, 3]
    rows = pr.MAIN_ROWS
    k = rows["on_face"]                                          # |z - cz| = dz / 2 exactly: inside
    assert tuple(points[k, 1:]) == pr.ON_FACE and abs(points[k, 3] - gt[0, 0, 2]) == gt[0, 0, 5] / 2 and idx[k] == 0 and labels[k] == 1
    k = rows["in_both"]                                          # two boxes of different class: the lower index wins
    assert d["plain"][k, 0] and d["plain"][k, 1] and gt[0, 0, 7] != gt[0, 1, 7] and idx[k] == 0 and labels[k] == gt[0, 0, 7]
    for k in (rows["padding_hit"], rows["padding_hit_frame1"]):  # an enlarged padding row and nothing else: ignored
        assert not d["plain"][k].any() and not d["ext"][k, :3].any() and d["ext"][k, 3:].all() and labels[k] == -1 and idx[k] == -1
    k = rows["ext_only"]
    assert not d["plain"][k].any() and d["ext"][k, 2] and labels[k] == -1
    k = rows["stray"]                                            # frame 2 of B = 2, at the centre of a box of frame 0
    assert points[k, 0] == 2 and labels[k] == 0 and idx[k] == -1
    assert pr.assign_targets(np.concatenate([[[0.0]], points[k:k + 1, 1:]], axis=1), gt, extra, 3)[0][0] == 1
    inside, outside = int((labels > 0).sum()), int((labels == 0).sum())
    assert inside >= 20 and outside >= 100 and int((labels == -1).sum()) >= 8
    assert np.array_equal(np.unique(pr.assign_targets(points, gt, extra, 1)[0]), [-1, 0, 1])

    mixed, perm = pr.interleaved(points)
    assert np.array_equal(mixed, cases["interleaved"][0]) and (np.diff(mixed[:, 0]) < 0).sum() > 50     # no stacked order
    assert np.array_equal(pr.assign_targets(mixed, gt, extra, 3)[0], labels[perm])

    points, gt, extra = cases["empty_frame"]
    assert gt.shape[0] == 3 and not (points[:, 0] == 1).any() and (points[:, 0] == 2).sum() == 214
    assert (pr.assign_targets(points, gt, extra, 3)[0][points[:, 0] == 2] > 0).any()

    points, gt, extra = cases["no_gt"]
    assert gt.shape == (2, 0, 8) and not pr.assign_targets(points, gt, extra, 3)[0].any()

    points, gt, extra = cases["chunk"]
    labels, idx = pr.assign_targets(points, gt, extra, 3)
    assert gt.shape == (1, 130, 8) and idx[0] == 129 and idx[1] == 128 and (idx >= 128).sum() >= 2 and labels[0] == gt[0, 129, 7]
    assert sorted(np.unique(labels)) == [-1, 0, 1, 2, 3] and ((idx >= 0) & (idx < 128)).sum() >= 10

    points, gt, extra = cases["negative_extra"]
    assert min(extra) < 0
    rows = pr.fg_without_ext_rows(points, gt, extra)             # the reference writes the class over the ignore flag
    labels, idx = pr.assign_targets(points, gt, extra, 3)
    assert len(rows) >= 3 and (labels[rows] > 0).all() and (labels == -1).any()


def test_restatement_equals_the_reference_and_the_float64_brute_force(g, cases):
    for name, (points, gt, extra) in cases.items():
        for num_class in (1, 3):
            labels, idx = pr.assign_targets(points, gt, extra, num_class)
            assert labels.dtype == np.int64 and idx.dtype == np.int32
            assert np.array_equal(labels, g["%s_labels_c%d" % (name, num_class)]), (name, num_class)
            want = pr.assign_targets_f64(points, gt, extra, num_class)
            assert np.array_equal(labels, want[0]) and np.array_equal(idx, want[1]), (name, num_class)
        if gt.shape[1]:                                          # points_in_boxes on the frames' own rows
            for b in range(gt.shape[0]):
                rows = points[:, 0] == b
                got = pr.points_in_boxes(gt[b:b + 1, :, :7], points[rows][None, :, 1:4])[0]
                assert np.array_equal(got, pr.assign_targets(points, gt, extra, 1)[1][rows]), (name, b)


def test_loss_restatement_equals_the_reference(g):
    for name in pr.LOSS_CASES:
        preds, labels = pr.loss_case(name)
        assert preds.shape[0] == 513 and preds.max() == 40 and preds.min() == -40
        loss, pos, grad = pr.loss_and_grad(preds, labels, pr.LOSS_WEIGHT, torch.float32, UPSTREAM)
        assert loss == float(g[name + "_loss"]) and pos == float(g[name + "_pos_num"]) == (labels > 0).sum(), name
        assert np.array_equal(grad, g[name + "_grad"].astype(np.float64)), name
        want = pr.loss_and_grad(preds, labels, pr.LOSS_WEIGHT, torch.float64, UPSTREAM)
        assert pr.rel_err(loss, want[0]) <= 1e-6 and pr.rel_err(grad, want[2]) <= 1e-5, name
    labels = pr.loss_case("c3")[1]
    assert sorted(np.unique(labels)) == [-1, 0, 1, 2, 3]
    assert sorted(np.unique(pr.loss_case("no_positive")[1])) == [-1, 0] and (pr.loss_case("all_ignored")[1] == -1).all()
    assert float(g["no_positive_pos_num"]) == 0 and float(g["no_positive_loss"]) > 0                  # the normaliser clamps to 1
    assert float(g["all_ignored_loss"]) == 0 and not g["all_ignored_grad"].any()


def test_composed_path_on_the_cpu(g, cases, monkeypatch):
    from dualfusion import _lib, dense_heads
    for name, (points, gt, extra) in cases.items():
        for num_class in (1, 3):
            labels, idx = dense_heads.composed_point_targets(torch.from_numpy(points), torch.from_numpy(gt), extra, num_class)
            want = pr.assign_targets(points, gt, extra, num_class)
            assert labels.dtype == torch.int64 and np.array_equal(labels.numpy(), want[0]) and np.array_equal(idx.numpy(), want[1]), name
    for name in pr.LOSS_CASES:
        preds, labels = pr.loss_case(name)
        x = torch.from_numpy(preds).requires_grad_(True)
        loss, pos = dense_heads.composed_point_cls_loss(x, torch.from_numpy(labels), pr.LOSS_WEIGHT)
        (UPSTREAM * loss[0]).backward()
        assert float(loss.detach()[0]) == float(g[name + "_loss"]) and float(pos[0]) == float(g[name + "_pos_num"]), name
        assert np.array_equal(x.grad.numpy(), g[name + "_grad"]), name

    # the head: parameter names, scores, the composed mode trains on the CPU, the fused mode refuses it
    torch.manual_seed(3)
    head = dense_heads.PointHeadSimple(num_class=3, input_channels=40, model_cfg=pr.point_head_cfg(before_fusion=False))
    assert sorted(k for k, _ in head.named_parameters()) == sorted(
        "cls_layers.%s" % k for k in ("0.weight", "1.weight", "1.bias", "3.weight", "4.weight", "4.bias", "6.weight", "6.bias"))
    points, gt, extra = cases["main"]
    batch = {"batch_size": 2, "point_features": torch.randn(514, 40), "point_coords": torch.from_numpy(points), "gt_boxes": torch.from_numpy(gt)}
    with pytest.raises(_lib.Df3dError, match="point_features must live on the GPU"):
        head(dict(batch))
    monkeypatch.setenv("DF3D_POINT_HEAD_FUSED", "0")
    head.train()
    out = head(batch)
    r = head.forward_ret_dict
    assert out is batch and sorted(r) == ["point_cls_labels", "point_cls_preds"] and tuple(r["point_cls_preds"].shape) == (514, 3)
    assert np.array_equal(r["point_cls_labels"].numpy(), pr.assign_targets(points, gt, extra, 3)[0])
    assert torch.equal(batch["point_cls_scores"], torch.sigmoid(r["point_cls_preds"]).max(dim=-1)[0]) and batch["point_cls_scores"].shape == (514,)
    loss, tb = head.get_loss({"kept": 1})
    assert sorted(tb) == ["kept", "point_loss_cls", "point_pos_num"] and not tb["point_loss_cls"].requires_grad
    assert float(tb["point_pos_num"]) == (r["point_cls_labels"] > 0).sum()
    loss.backward()
    assert all(p.grad is not None and bool(p.grad.abs().sum() > 0) for p in head.parameters())
    head.eval()
    head(batch)
    assert sorted(head.forward_ret_dict) == ["point_cls_preds"]
    with pytest.raises(KeyError, match="training-mode forward"):
        head.get_loss()


def test_refusals_of_the_head_and_the_detector():
    from dualfusion import dense_heads, synth, vr_detector
    from dualfusion.roi_heads import VoxelRCNNHead
    import stacksa_reference as sr
    cfg = pr.point_head_cfg()
    cfg.pop("CLS_FC")
    with pytest.raises(KeyError, match="CLS_FC"):
        dense_heads.PointHeadSimple(num_class=1, input_channels=8, model_cfg=cfg)
    for drop, text in (("TARGET_CONFIG", "GT_EXTRA_WIDTH"), ("LOSS_CONFIG", "point_cls_weight")):
        cfg = pr.point_head_cfg()
        cfg.pop(drop)
        head = dense_heads.PointHeadSimple(num_class=1, input_channels=8, model_cfg=cfg)       # an eval-only config builds
        with pytest.raises(KeyError, match=text):
            head._training_setup()
    geometry = (np.array([1408, 1600, 40]), synth.KITTI_RANGE, synth.KITTI_VOXEL)
    for edit, text in ((("DENSE_HEAD_3D", {"NAME": "MMDet3DHead"}), "DENSE_HEAD_3D"), (("BACKBONE_3D", "SEG_LOSS"), "SEG_LOSS"),
                       (("BACKBONE_3D", "AUX_PTS_LOSS"), "AUX_PTS_LOSS"), (("BACKBONE_3D", "AUX_CNS_LOSS"), "AUX_CNS_LOSS")):
        cfg = pr.pv_rcnn_cfg()
        if edit[0] == "BACKBONE_3D":
            cfg["BACKBONE_3D"] = dict(cfg["BACKBONE_3D"], **{edit[1]: True})
        else:
            cfg[edit[0]] = edit[1]
        with pytest.raises(NotImplementedError, match=text):
            vr_detector.PVRCNN(cfg, 1, ["Car"], *geometry)
    for key in ("PFE", "POINT_HEAD"):
        cfg = pr.pv_rcnn_cfg()
        cfg.pop(key)
        with pytest.raises(KeyError, match=key):
            vr_detector.PVRCNN(cfg, 1, ["Car"], *geometry)
    cfg = pr.pv_rcnn_cfg()
    cfg["POINT_HEAD"] = dict(cfg["POINT_HEAD"], NAME="PointHeadBox")
    with pytest.raises(KeyError, match="PointHeadBox is not in"):
        vr_detector.PVRCNN(cfg, 1, ["Car"], *geometry)
    # the shipped TRAIN proposals stay refused: 9000 candidates are past the cap of the top-k select and the NMS
    with pytest.raises(NotImplementedError, match="NMS_PRE_MAXSIZE = 9000 exceeds 4096"):
        VoxelRCNNHead.check_nms_config(sr.SHIPPED_HEAD["NMS_CONFIG"]["TRAIN"], "PVRCNNHead.proposal_layer")


def test_pvrcnn_builds_from_a_config_shaped_like_the_shipped_one():
    from dualfusion import synth, vr_detector
    model = vr_detector.PVRCNN(pr.pv_rcnn_cfg(), 1, ["Car"], np.array([1408, 1600, 40]), synth.KITTI_RANGE, synth.KITTI_VOXEL)
    kinds = [type(m).__name__ for m in model.module_list]
    assert kinds == ["VoxelBackBone8x", "HeightCompression", "VoxelSetAbstraction", "BaseBEVBackbone", "AnchorHeadSingle",
                     "PointHeadSimple", "PVRCNNHead"]
    assert [n for n, _ in model.named_children()] == ["backbone_3d", "map_to_bev_module", "pfe", "backbone_2d", "dense_head",
                                                      "point_head", "roi_head"]
    # detector3d_template.py:100-173: the channel hand-offs
    pfe = model.pfe
    assert pfe.num_point_features_before_fusion == 256 + 2 * 64 + 2 * 16 and pfe.num_point_features == 32
    assert model.point_head.cls_layers[0].in_features == pfe.num_point_features_before_fusion
    assert model.roi_head.roi_grid_pool_layer.mlps[0][0].in_channels == pfe.num_point_features + 3
    assert model.backbone_2d.blocks[0][1].in_channels == 256 and model.dense_head.conv_cls.in_channels == 256
    assert model.point_head.num_class == 1 and model.roi_head.num_class == 1 and model.roi_head.post_process_cfg["SCORE_THRESH"] == 0.3
    cfg = pr.pv_rcnn_cfg()
    cfg["POINT_HEAD"] = pr.point_head_cfg(before_fusion=False)
    model = vr_detector.PVRCNN(cfg, 3, ["Car", "Pedestrian", "Cyclist"], np.array([1408, 1600, 40]), synth.KITTI_RANGE, synth.KITTI_VOXEL)
    assert model.point_head.cls_layers[0].in_features == 32 and model.point_head.cls_layers[6].out_features == 3
    cfg["POINT_HEAD"] = pr.point_head_cfg(agnostic=True)
    model = vr_detector.PVRCNN(cfg, 3, ["Car", "Pedestrian", "Cyclist"], np.array([1408, 1600, 40]), synth.KITTI_RANGE, synth.KITTI_VOXEL)
    assert model.point_head.cls_layers[6].out_features == 1


def test_the_anchor_head_keeps_its_training_refusal_and_shares_the_prediction_keys(monkeypatch):
    """AnchorHeadSingle.forward behaves as before (eval only); the helper it now shares writes the same keys from the
    detached rows of a forward_train pass"""
    import anchorloss_reference as al
    import vrtail_reference as vt
    from dualfusion import dense_heads
    grid, rng = vt.case_geometry("small")
    c = vt.CASES["small"]
    torch.manual_seed(0)
    head = dense_heads.AnchorHeadSingle(al.train_head_cfg("small"), 16, 1, ["Car"], grid, rng)
    x = torch.randn(c["B"], 16, c["H"], c["W"])
    head.train()
    with pytest.raises(NotImplementedError, match="eval mode only"):
        head({"spatial_features_2d": x})
    with pytest.raises(KeyError, match="follows forward_train"):
        head.write_train_predictions({})
    monkeypatch.setenv("DF3D_ANCHOR_LOSS_FUSED", "0")
    gt = torch.zeros((c["B"], 2, 8))
    gt[:, 0] = torch.tensor([rng[0] + 5.0, rng[1] + 5.0, -1.0, 3.9, 1.6, 1.56, 0.3, 1.0])
    train = head.forward_train({"spatial_features_2d": x, "gt_boxes": gt, "batch_size": c["B"]})
    for mode, keys in (("1", ["dense_anchor_tables", "dense_box_rows", "dense_cls_rows", "dense_dir_rows"]),
                       ("0", ["batch_box_preds", "batch_cls_preds", "cls_preds_normalized"])):
        monkeypatch.setenv("DF3D_VR_TAIL_FUSED", mode)
        out = {}
        assert head.write_train_predictions(out) is out and sorted(out) == keys
        assert all(not v.requires_grad for v in out.values() if isinstance(v, torch.Tensor))
        head.eval()
        with torch.no_grad():
            want = head({"spatial_features_2d": x})
        head.train()
        for k in keys:
            if isinstance(out[k], torch.Tensor):
                assert torch.allclose(out[k], want[k], atol=1e-5), k
    assert head.forward_ret_dict["rows"].requires_grad and train["gt_boxes"] is gt
