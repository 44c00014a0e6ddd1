"""The Voxel-RCNN second-stage training path without a GPU: the entry points of csrc/roiloss.hip are declared, exported and
bound; their argument errors and limits; every new refusal, and the four refusals that stay; the float64 restatement of
tests/roiloss_reference.py against the reference's results (tests/golden/roi_loss.npz): indices, labels, masks and counts
exact, values within float32 rounding; the margins and the coverage of the fixture; the composed losses on the CPU against
the fixture's losses and gradients; ProposalTargetLayer's own draws are reproducible from a seeded generator."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import roiloss_reference as rl
import vrtail_reference as vt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["df3d_roi_targets_workspace_bytes", "df3d_roi_targets", "df3d_rcnn_loss_workspace_bytes", "df3d_rcnn_loss",
           "df3d_rcnn_loss_grad"]
LEVELS = {"x_a": 8, "x_b": 16}
TARGET_KEYS = ("rois", "gt_of_rois", "gt_of_rois_src", "gt_iou_of_rois", "roi_scores", "roi_labels", "reg_valid_mask", "rcnn_cls_labels")


@pytest.fixture(scope="module")
def g(golden):
    return golden("roi_loss.npz")


@pytest.fixture(scope="module")
def restated(g):
    return {name: rl.restate(name, g) for name in rl.CASES}


def head_cfg(**edit):
    layer = lambda c: {"MLPS": [[c, 8]], "QUERY_RANGES": [[2, 2, 2]], "POOL_RADIUS": [0.8], "NSAMPLE": [8], "POOL_METHOD": "max_pool"}
    cfg = {"CLASS_AGNOSTIC": True, "SHARED_FC": [16], "CLS_FC": [8], "REG_FC": [8], "DP_RATIO": 0.0,
           "ROI_GRID_POOL": {"FEATURES_SOURCE": list(LEVELS), "GRID_SIZE": 2, "POOL_LAYERS": {n: layer(c) for n, c in LEVELS.items()}},
           "TARGET_CONFIG": rl.sampler_cfg("iou"), "LOSS_CONFIG": copy.deepcopy(rl.LOSS_CFG)}
    cfg.update(edit)
    return cfg


def build_head(**edit):
    from dualfusion import roi_heads
    return roi_heads.VoxelRCNNHead(dict(LEVELS), head_cfg(**edit), [0, -40, -3, 70.4, 40, 1], [0.05, 0.05, 0.1])


def test_symbols_are_declared_exported_and_bound():
    import __graft_entry__ as ge
    build = ge._load(os.path.join(ge.PKG, "csrc", "build.py"), "df3d_build")
    build.build()
    from dualfusion import _lib, ops, roi_heads
    header = open(os.path.join(ROOT, "include", "df3d_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, header), s
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES, s
    assert "roiloss.hip" in build.SOURCES
    macros = dict(re.findall(r"#define (DF3D_ROI_\w+) (\d+)", header))
    assert int(macros["DF3D_ROI_MAX_ROIS"]) == ops.ROI_MAX_ROIS == ops.TAIL_MAX_CANDIDATES == 4096
    assert int(macros["DF3D_ROI_MAX_SAMPLES"]) == ops.ROI_MAX_SAMPLES >= 512
    assert int(macros["DF3D_ROI_MAX_GT"]) == ops.ROI_MAX_GT >= ops.ANCHOR_MAX_GT
    assert {k: int(macros["DF3D_ROI_SCORE_" + k.upper()]) for k in ops.ROI_SCORE_TYPES} == ops.ROI_SCORE_TYPES
    for name in ("roi_targets", "RcnnLossSpec", "rcnn_loss", "roi_target_cfg"):
        assert callable(getattr(ops, name)), name
    for name in ("ProposalTargetLayer", "composed_roi_targets", "composed_rcnn_losses", "roi_loss_fused"):
        assert callable(getattr(roi_heads, name)), name
    for name in ("assign_targets", "forward_train", "get_loss"):
        assert callable(getattr(roi_heads.VoxelRCNNHead, name)), name


def test_argument_errors_and_limits_are_reported_without_a_gpu():
    from dualfusion import _lib, ops
    lib = _lib.bind(ctypes.CDLL(_lib.LIB_PATH), check=False)
    byref = ctypes.byref
    one = (ctypes.c_float * 64)()
    buf = ctypes.cast(one, ctypes.c_void_p)
    err = lambda: lib.df3d_last_error()
    nulls = lambda n: [None] * n

    assert lib.df3d_roi_targets(*nulls(6), None, *nulls(10), None, 0, None) == -1 and b"roi_targets: null config" in err()
    mk = lambda B=2, R=100, G=8, **k: ops.roi_target_cfg(B, R, G, dict(rl.sampler_cfg("iou"), **k))
    call = lambda cfg, ws=1 << 20: lib.df3d_roi_targets(*[buf] * 6, byref(cfg), *[buf] * 10, buf, ws, None)
    cfg = mk()
    assert (cfg.roi_per_image, cfg.fg_per_image, cfg.sample_by_class, cfg.cls_score_type) == (16, 8, 1, 0)
    assert mk(ROI_PER_IMAGE=5).fg_per_image == 2 and mk(ROI_PER_IMAGE=7).fg_per_image == 4              # numpy rounds half to even
    need = lib.df3d_roi_targets_workspace_bytes(byref(cfg))
    assert need >= 4 * 2 * 100 * 4
    assert call(cfg, need - 1) == -1 and b"workspace" in err()
    assert lib.df3d_roi_targets(None, *[buf] * 5, byref(cfg), *[buf] * 10, buf, need, None) == -1 and b"null input" in err()
    for edit, text in ((dict(num_rois=4097), b"1..4096 RoIs"), (dict(roi_per_image=1025), b"1..1024 sampled"), (dict(max_gt=1025), b"1..1024 ground-truth"),
                       (dict(batch=0), b"frames"), (dict(fg_per_image=17), b"fg_per_image"), (dict(hard_bg_ratio=1.5), b"hard_bg_ratio"),
                       (dict(cls_score_type=2), b"unknown cls_score_type"), (dict(cls_fg_thresh=0.2), b"cls_fg_thresh")):
        bad = mk()
        for k, v in edit.items():
            setattr(bad, k, v)
        assert call(bad) == -1 and text in err(), (edit, err())
    assert lib.df3d_roi_targets_workspace_bytes(None) == 0

    spec = ops.RcnnLossSpec(1.0, 1.0, 1.0, [1.0] * 7)
    lcfg = spec.cfg(96)
    lneed = lib.df3d_rcnn_loss_workspace_bytes(byref(lcfg))
    assert lneed >= 5 * 8
    loss = lambda c, ld_cls=1, ld_reg=7, ws=lneed: lib.df3d_rcnn_loss(buf, ld_cls, buf, ld_reg, *[buf] * 5, byref(c), buf, buf, buf, ws, None)
    assert lib.df3d_rcnn_loss(buf, 1, buf, 7, *[buf] * 5, None, buf, buf, buf, lneed, None) == -1 and b"rcnn_loss: null config" in err()
    assert loss(lcfg, ld_reg=6) == -1 and b"row stride" in err()
    assert loss(lcfg, ws=8) == -1 and b"workspace" in err()
    assert loss(spec.cfg(0)) == -1 and b"bad row count" in err()
    assert lib.df3d_rcnn_loss_grad(buf, 1, buf, 7, *[buf] * 5, byref(lcfg), None, buf, buf, 1, buf, 7, None) == -1 and b"null gradient" in err()
    assert lib.df3d_rcnn_loss_grad(buf, 1, buf, 7, *[buf] * 5, byref(lcfg), buf, buf, buf, 1, buf, 6, None) == -1 and b"gradient row stride" in err()


def test_new_refusals_name_the_key():
    from dualfusion import _lib, ops, roi_heads
    with pytest.raises(NotImplementedError, match="CLS_LOSS CrossEntropy"):
        build_head(LOSS_CONFIG=dict(rl.LOSS_CFG, CLS_LOSS="CrossEntropy"))._training_setup()
    with pytest.raises(NotImplementedError, match="REG_LOSS l1"):
        build_head(LOSS_CONFIG=dict(rl.LOSS_CFG, REG_LOSS="l1"))._training_setup()
    with pytest.raises(KeyError, match="LOSS_CONFIG"):
        build_head(LOSS_CONFIG=None)._training_setup()
    with pytest.raises(NotImplementedError, match="CLS_SCORE_TYPE 'raw_roi_iou'"):
        roi_heads.ProposalTargetLayer(dict(rl.sampler_cfg("iou"), CLS_SCORE_TYPE="raw_roi_iou"))
    with pytest.raises(NotImplementedError, match="CLS_SCORE_TYPE 'raw_roi_iou'"):
        ops.roi_target_cfg(2, 100, 8, dict(rl.sampler_cfg("iou"), CLS_SCORE_TYPE="raw_roi_iou"))
    for B, R, G, m, text in ((2, 4097, 8, 16, "4097 RoIs per frame exceed 4096"), (2, 100, 8, 1025, "ROI_PER_IMAGE = 1025 exceeds 1024"),
                             (2, 100, 1025, 16, "1025 ground-truth rows per frame exceed 1024")):
        with pytest.raises(NotImplementedError, match=text):
            ops.roi_target_cfg(B, R, G, dict(rl.sampler_cfg("iou"), ROI_PER_IMAGE=m))
    with pytest.raises(KeyError, match="HARD_BG_RATIO"):
        ops.roi_target_cfg(2, 100, 8, {k: v for k, v in rl.sampler_cfg("iou").items() if k != "HARD_BG_RATIO"})
    with pytest.raises(NotImplementedError, match="wider than 7"):
        ops.RcnnLossSpec(1.0, 1.0, 1.0, [1.0] * 9)
    layer = roi_heads.ProposalTargetLayer(rl.sampler_cfg("iou"))
    wide = {"rois": torch.zeros(2, 10, 9), "roi_scores": torch.zeros(2, 10), "roi_labels": torch.ones(2, 10, dtype=torch.long),
            "gt_boxes": torch.zeros(2, 3, 10)}
    with pytest.raises(NotImplementedError, match="wider than 7"):
        layer(wide)
    big = {"rois": torch.zeros(1, 4097, 7), "roi_scores": torch.zeros(1, 4097), "roi_labels": torch.ones(1, 4097, dtype=torch.long),
           "gt_boxes": torch.zeros(1, 3, 8)}
    with pytest.raises(NotImplementedError, match="exceed the caps 4096"):
        layer(big)
    head = build_head().train()
    with pytest.raises(NotImplementedError, match="wider than 7"):
        head.forward_train({"batch_size": 2, "rois": torch.zeros(2, 10, 9), "gt_boxes": torch.zeros(2, 3, 10)})
    with pytest.raises(KeyError, match="rois"):
        head.forward_train({"batch_size": 2, "gt_boxes": torch.zeros(2, 3, 8)})
    with pytest.raises(NotImplementedError, match="wider than 7"):
        roi_heads.composed_rcnn_losses(torch.zeros(4, 1), torch.zeros(4, 9), {}, head.loss_spec)
    # the fused mode has no CPU path: a missing device is an error, never a quiet change of formulation
    small = {"batch_size": 2, "rois": torch.zeros(2, 10, 7), "roi_scores": torch.zeros(2, 10), "roi_labels": torch.ones(2, 10, dtype=torch.long),
             "gt_boxes": torch.zeros(2, 3, 8)}
    with pytest.raises(_lib.Df3dError, match="no CPU fallback"):
        layer(small)


def test_the_four_pinned_refusals_still_fire():
    from dualfusion import dense_heads, roi_heads, vr_detector
    import roipool_reference as rp
    grid, rng = np.array([1408, 1600, 40]), [0, -40, -3, 70.4, 40, 1]
    with pytest.raises(NotImplementedError, match="NMS_PRE_MAXSIZE = 9000 exceeds 4096"):
        roi_heads.VoxelRCNNHead.check_nms_config({"NMS_TYPE": "nms_gpu", "MULTI_CLASSES_NMS": False, "NMS_PRE_MAXSIZE": 9000,
                                                  "NMS_POST_MAXSIZE": 512, "NMS_THRESH": 0.8}, "proposal_layer")
    head = build_head(NMS_CONFIG={"TRAIN": {"NMS_TYPE": "nms_gpu", "MULTI_CLASSES_NMS": False, "NMS_PRE_MAXSIZE": 9000,
                                            "NMS_POST_MAXSIZE": 512, "NMS_THRESH": 0.8}}).train()
    with pytest.raises(NotImplementedError, match="NMS_PRE_MAXSIZE = 9000 exceeds 4096"):                 # forward_train stays inside the cap
        head.forward_train({"batch_size": 1, "batch_box_preds": torch.zeros(1, 4, 7), "batch_cls_preds": torch.zeros(1, 4, 1),
                            "gt_boxes": torch.zeros(1, 2, 8)})
    with pytest.raises(KeyError, match="rois"):                                                          # forward as it was
        build_head().eval()({"batch_size": 1})
    anchor = dense_heads.AnchorHeadSingle(copy.deepcopy(vt.head_cfg("car")), 16, 1, ["Car"], grid, rng).train()
    with pytest.raises(NotImplementedError, match="eval mode only"):
        anchor({"spatial_features_2d": torch.zeros(1, 16, 200, 176), "batch_size": 1})
    bev = {"NAME": "BaseBEVBackbone", "LAYER_NUMS": [1], "LAYER_STRIDES": [1], "NUM_FILTERS": [16], "UPSAMPLE_STRIDES": [1],
           "NUM_UPSAMPLE_FILTERS": [16]}
    cfg = {"NAME": "VoxelRCNN", "BACKBONE_3D": {"NAME": "VoxelBackBone8x"}, "MAP_TO_BEV": {"NAME": "HeightCompression", "NUM_BEV_FEATURES": 256},
           "BACKBONE_2D": bev, "DENSE_HEAD": vt.head_cfg("car"), "ROI_HEAD": dict(rp.HEAD_CFG, NMS_CONFIG={"TEST": vt.nms_cfg("car")}),
           "POST_PROCESSING": vt.post_cfg()}
    model = vr_detector.VoxelRCNN(cfg, 1, ["Car"], grid, rng, [0.05, 0.05, 0.1]).train()
    with pytest.raises(NotImplementedError, match="eval mode only"):
        model({"batch_size": 1})


def test_switch_is_read_per_call(monkeypatch):
    from dualfusion import roi_heads
    monkeypatch.delenv("DF3D_ROI_LOSS_FUSED", raising=False)
    assert roi_heads.roi_loss_fused() is True
    monkeypatch.setenv("DF3D_ROI_LOSS_FUSED", "0")
    assert roi_heads.roi_loss_fused() is False


def bound(want):
    return 8 * vt.U32 * np.abs(want).max()


@pytest.mark.parametrize("name", list(rl.CASES))
def test_float64_restatement_against_the_reference(g, restated, name):
    t, l = restated[name]
    c = rl.CASES[name]
    assert g[name + "_rois"].shape == (rl.B, c["R"], 7) and g[name + "_t_rois"].shape == (rl.B, rl.M, 7) and g[name + "_gt"].shape[1] <= 8
    # indices (through the gathered rows), labels, masks, counts: exact
    rows = g[name + "_rois"][np.arange(rl.B)[:, None], t["inds"]]
    assert np.array_equal(rows, g[name + "_t_rois"])
    assert np.array_equal(t["roi_labels"], g[name + "_t_roi_labels"])
    assert np.array_equal(t["roi_scores"].astype(np.float32), g[name + "_t_roi_scores"])
    assert np.array_equal(t["reg_valid_mask"], g[name + "_t_reg_valid_mask"])
    assert np.array_equal(t["cls_labels_cls"], g[name + "_t_cls_labels_cls"])
    assert np.array_equal(t["gt_of_rois_src"].astype(np.float32), g[name + "_t_gt_of_rois_src"])
    assert np.array_equal(t["counts"], np.asarray(rl.frame_plan(c["R"])))
    hard = np.isin(t["cls_labels_roi_iou"], (0.0, 1.0))
    assert np.array_equal(t["cls_labels_roi_iou"][hard], g[name + "_t_cls_labels_roi_iou"][hard]) and (~hard).any()
    # values: a handful of float32 roundings of the largest magnitude
    for key, want in (("gt_iou_of_rois", t["gt_iou_of_rois"]), ("gt_of_rois", t["gt_of_rois"]), ("cls_labels_roi_iou", t["cls_labels_roi_iou"])):
        assert np.abs(g[name + "_t_" + key] - want).max() <= bound(want), key
    assert np.abs(g[name + "_t_rcnn_cls_labels"] - t["rcnn_cls_labels"]).max() <= bound(t["rcnn_cls_labels"])
    # float32 sums over up to 96 x 8 terms in the reference: 64 roundings of the largest
    assert np.abs(g[name + "_loss"] - l["loss"]).max() <= 64 * vt.U32 * np.abs(l["loss"]).max()
    for key in ("grad_cls", "grad_reg"):
        assert g[name + "_" + key].shape == l[key].shape
        assert np.abs(g[name + "_" + key] - l[key]).max() <= 64 * vt.U32 * np.abs(l[key]).max(), key
    assert not l["grad_reg"][t["reg_valid_mask"].reshape(-1) == 0].any()
    assert not l["grad_cls"][t["rcnn_cls_labels"].reshape(-1) < 0].any()


def test_the_two_evaluations_of_the_overlap_agree(g):
    """the vectorised clipping of the restatement against Sutherland-Hodgman, pair by pair, on the fixture's boxes"""
    rois, gt = g["iou_rois"][0].astype(np.float64), g["iou_gt"][0, [0, 1, 3, 4, 5]].astype(np.float64)
    i, j = np.repeat(np.arange(len(rois)), len(gt)), np.tile(np.arange(len(gt)), len(rois))
    fast = rl.bev_overlap_pairs(rois[i], gt[j, :7])
    slow = np.array([rl.bev_overlap_clip(rois[a], gt[b, :7]) for a, b in zip(i, j)])
    assert (slow > 0.5).sum() > 20 and (slow == 0).sum() > 20
    assert np.abs(fast - slow).max() <= 1e-12 * max(1.0, slow.max())


def test_fixture_margins_and_coverage(g, restated):
    import make_golden_roiloss as gen
    seen = dict(scores=set(), by_class=set())
    for name in rl.CASES:
        t, l = restated[name]
        assert t["thresh_dist"] >= rl.THRESH_MARGIN and t["gap"] >= rl.GAP_MARGIN and t["heading_dist"] >= rl.HEADING_MARGIN, name
        assert l["beta_dist"] >= rl.BETA_MARGIN and l["corner_dist"] >= rl.BETA_MARGIN and l["flip_gap"] >= rl.GAP_MARGIN, name
        assert l["logit_max"] <= rl.LOGIT_MAX and rl.keys_distinct(g[name + "_u_fg"])
        assert gen.covered(name, rl.coverage(name, g, t, l)), name
        seen["scores"].add(rl.CASES[name]["score"])
        seen["by_class"].add(rl.CASES[name]["by_class"])
        for u in (g[name + "_u_fg"], g[name + "_u_slot"]):
            assert u.dtype == np.float32 and u.min() >= 0 and u.max() < 1
    assert seen == dict(scores={"roi_iou", "cls"}, by_class={True, False})
    assert sorted(rl.CASES[n]["R"] for n in rl.CASES) == [100, 100, 300] and 100 % 64 and 300 % 256
    for k in g.files:
        assert g[k].nbytes < 400 * 1024, k


@pytest.mark.parametrize("name", list(rl.CASES))
def test_composed_losses_on_the_cpu_match_the_reference(g, restated, monkeypatch, name):
    """composed_rcnn_losses from the fixture's targets: the reference's formulation in float32 on the CPU, through get_loss"""
    from dualfusion import roi_heads
    monkeypatch.setenv("DF3D_ROI_LOSS_FUSED", "0")
    t, l = restated[name]
    head = build_head().train()
    ret = {k: torch.from_numpy(np.ascontiguousarray(g[name + "_t_" + k])) for k in TARGET_KEYS}
    ret["rcnn_cls"] = torch.from_numpy(g[name + "_rcnn_cls"].copy()).requires_grad_(True)
    ret["rcnn_reg"] = torch.from_numpy(g[name + "_rcnn_reg"].copy()).requires_grad_(True)
    head.forward_ret_dict = ret
    loss, tb = head.get_loss()
    assert sorted(tb) == ["rcnn_loss", "rcnn_loss_cls", "rcnn_loss_corner", "rcnn_loss_reg"]
    assert all(isinstance(v, torch.Tensor) and not v.requires_grad for v in tb.values())
    loss.backward()
    got = np.array([float(tb[k]) for k in ("rcnn_loss_cls", "rcnn_loss_reg", "rcnn_loss_corner")])
    assert np.abs(got - l["loss"]).max() <= 64 * vt.U32 * np.abs(l["loss"]).max()
    assert abs(float(loss.detach()) - l["loss"].sum()) <= 64 * vt.U32 * l["loss"].sum()
    assert np.abs(got - g[name + "_loss"]).max() <= 64 * vt.U32 * np.abs(l["loss"]).max()
    for key in ("rcnn_cls", "rcnn_reg"):
        want = l["grad_" + key[5:]]
        assert np.abs(ret[key].grad.numpy() - want).max() <= 64 * vt.U32 * np.abs(want).max(), key
        assert np.abs(ret[key].grad.numpy() - g[name + "_grad_" + key[5:]]).max() <= 64 * vt.U32 * np.abs(want).max(), key


def test_composed_targets_on_the_cpu_match_the_reference(g, restated):
    """the composed assignment is plain torch: it also runs here, and gives the reference's indices, labels and masks"""
    from dualfusion import roi_heads
    name = "iou"
    t, _ = restated[name]
    tens = lambda k: torch.from_numpy(np.ascontiguousarray(g[name + "_" + k]))
    out = roi_heads.composed_roi_targets(tens("rois"), tens("roi_scores"), tens("roi_labels"), tens("gt"), tens("u_fg"), tens("u_slot"),
                                         rl.sampler_cfg(name))
    assert np.array_equal(out["roi_inds"].numpy(), t["inds"]) and np.array_equal(out["counts"].numpy(), t["counts"])
    for k in ("rois", "roi_labels", "roi_scores", "reg_valid_mask", "gt_of_rois_src"):
        assert np.array_equal(out[k].numpy(), g[name + "_t_" + k]), k
    for k in ("gt_iou_of_rois", "gt_of_rois", "rcnn_cls_labels"):
        assert np.abs(out[k].numpy() - t[k]).max() <= bound(t[k]), k


def test_proposal_target_layer_draws_are_reproducible():
    from dualfusion import roi_heads
    layer = roi_heads.ProposalTargetLayer(rl.sampler_cfg("iou"), generator=torch.Generator().manual_seed(5))
    a = layer.draws(3, 50, torch.device("cpu"))
    b = layer.draws(3, 50, torch.device("cpu"))
    layer.generator.manual_seed(5)
    c = layer.draws(3, 50, torch.device("cpu"))
    assert tuple(a[0].shape) == (3, 50) and tuple(a[1].shape) == (3, rl.M) and a[0].dtype == torch.float32
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1]) and not torch.equal(a[0], b[0])
    assert float(a[0].min()) >= 0 and float(a[0].max()) < 1
    with pytest.raises(ValueError, match="both u_fg and u_slot"):
        layer({"rois": torch.zeros(1, 4, 7), "roi_scores": torch.zeros(1, 4), "roi_labels": torch.ones(1, 4, dtype=torch.long),
               "gt_boxes": torch.zeros(1, 2, 8)}, u_fg=torch.zeros(1, 4))
