"""The Voxel-RCNN first-stage training path without a GPU: the entry points of csrc/anchorloss.hip are declared, exported and
bound; their argument errors and limits; every refusal of the target assigner; the float64 restatement of
tests/anchorloss_reference.py against the reference's results (tests/golden/anchor_loss.npz): labels exact, values within
float32 rounding; the margins and the coverage of the fixture; `forward` in training mode still refuses next to
`forward_train`."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import anchorloss_reference as al
import vrtail_reference as vt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["df3d_anchor_assign_workspace_bytes", "df3d_anchor_assign", "df3d_anchor_loss_workspace_bytes", "df3d_anchor_loss",
           "df3d_anchor_loss_grad"]
TABLE = [[-1.0, 3.9, 1.6, 1.56, 0.0], [-1.0, 3.9, 1.6, 1.56, 1.57]]


@pytest.fixture(scope="module")
def g(golden):
    return golden("anchor_loss.npz")


@pytest.fixture(scope="module")
def restated(g):
    return {name: al.restate(name, g) for name in vt.CASES}


def build_head(name, **edit):
    from dualfusion import dense_heads
    cfg = copy.deepcopy(al.train_head_cfg(name))
    cfg.update(edit)
    grid, rng = vt.case_geometry(name)
    return dense_heads.AnchorHeadSingle(cfg, 16, vt.CASES[name]["C"], al.TRAIN[name]["class_names"], grid, rng)


def test_symbols_are_declared_exported_and_bound():
    import __graft_entry__ as ge
    build = ge._load(os.path.join(ge.PKG, "csrc", "build.py"), "df3d_build")
    build.build()
    from dualfusion import _lib, ops
    header = open(os.path.join(ROOT, "include", "df3d_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, header), s
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES, s
    assert "anchorloss.hip" in build.SOURCES
    macros = dict(re.findall(r"#define (DF3D_ANCHOR_\w+) (\d+)", header))
    assert int(macros["DF3D_ANCHOR_MAX_GT"]) == ops.ANCHOR_MAX_GT == 1024
    assert int(macros["DF3D_ANCHOR_GT_CHUNK"]) == ops.ANCHOR_GT_CHUNK


def test_argument_errors_and_limits_are_reported_without_a_gpu():
    from dualfusion import _lib, ops
    lib = _lib.bind(ctypes.CDLL(_lib.LIB_PATH), check=False)
    byref = ctypes.byref
    one = (ctypes.c_float * 64)()
    buf = ctypes.cast(one, ctypes.c_void_p)
    err = lambda: lib.df3d_last_error()

    # ---- df3d_anchor_assign
    assert lib.df3d_anchor_assign(None, None, None, None, None, None, None, None, None, None, 0, None) == -1
    assert b"anchor_assign: null config" in err()
    mk = lambda B=2, H=25, W=22, M=15, sets=(0, 0), cls=(1,): ops.anchor_assign_cfg(B, H, W, M, list(sets), TABLE, list(cls), [0.6] * len(cls),
                                                                                   [0.45] * len(cls))
    cfg = mk()
    assert lib.df3d_anchor_assign_workspace_bytes(byref(cfg)) > 0
    assert lib.df3d_anchor_assign(None, None, None, byref(cfg), None, None, None, None, None, None, 0, None) == -1
    assert b"anchor_assign: null input" in err()
    assert lib.df3d_anchor_assign(buf, buf, buf, byref(cfg), None, None, None, None, None, None, 0, None) == -1
    assert b"anchor_assign: null output" in err()
    call = lambda c, ws=1 << 30: lib.df3d_anchor_assign(buf, buf, buf, byref(c), buf, buf, buf, None, None, buf, ws, None)
    assert call(cfg, ws=16) == -1 and b"workspace 16 <" in err()
    assert call(mk(B=256)) == -1 and b"at most 255 frames" in err()
    assert call(mk(H=4096, W=2048)) == -1 and b"at most 2^22 anchors per frame" in err()
    assert call(mk(M=1025)) == -1 and b"1..1024 ground-truth rows per frame (got M = 1025)" in err()
    assert lib.df3d_anchor_assign_workspace_bytes(byref(mk(M=1025))) == 0
    assert call(mk(M=0)) == -1 and b"ground-truth rows" in err()
    assert call(mk(sets=(0, 1))) == -1 and b"names set 1 of 1" in err()
    assert call(mk(cls=(0,))) == -1 and b"serves class 0" in err()
    many = mk()
    many.anchors.num_anchors = 33
    assert call(many) == -1 and b"1..32 anchors per location (DF3D_MAX_ANCHORS)" in err()
    with pytest.raises(NotImplementedError, match="at most 32 anchors"):
        ops.anchor_assign_cfg(1, 4, 4, 8, [0] * 33, [TABLE[0]] * 33, [1], [0.6], [0.45])
    with pytest.raises(ValueError, match="one class id and one pair of thresholds"):
        ops.anchor_assign_cfg(1, 4, 4, 8, [0, 0], TABLE, [1], [0.6, 0.5], [0.45])

    # ---- df3d_anchor_loss / df3d_anchor_loss_grad
    lk = lambda B=2, H=25, W=22, M=15, C=1, NB=2, beta=1.0 / 9.0: ops.anchor_loss_cfg(B, H, W, M, C, NB, [0, 0], TABLE, 1, 1.0, 2.0, 0.2,
                                                                                   [1.0] * 7, 0.78539, beta)
    loss = lambda c, ld_cls=2, ld_box=14, ld_dir=4, dirs=buf, ws=1 << 30, out=buf: lib.df3d_anchor_loss(
        buf, ld_cls, buf, ld_box, dirs, ld_dir, buf, buf, buf, buf, buf, buf, byref(c) if c is not None else None, out, buf, ws, None)
    grad = lambda c, ld_g=(2, 14, 4), up=buf, gdir=buf: lib.df3d_anchor_loss_grad(
        buf, 2, buf, 14, buf, 4, buf, buf, buf, buf, buf, buf, byref(c), up, buf, ld_g[0], buf, ld_g[1], gdir, ld_g[2], None)
    assert loss(None) == -1 and b"anchor_loss: null config" in err()
    cfg = lk()
    assert lib.df3d_anchor_loss_workspace_bytes(byref(cfg)) >= 3 * 8 * ((2 * 25 * 22 * 2 + 255) // 256)
    assert lib.df3d_anchor_loss(None, 2, None, 14, None, 4, None, None, None, None, None, None, byref(cfg), None, None, 0, None) == -1
    assert b"anchor_loss: null input" in err()
    assert loss(cfg, out=None) == -1 and b"anchor_loss: null output" in err()
    assert loss(cfg, ld_cls=1) == -1 and b"row stride is smaller" in err()
    assert loss(cfg, ld_box=13) == -1 and b"row stride is smaller" in err()
    assert loss(cfg, ld_dir=3) == -1 and b"direction map needs" in err()
    assert loss(lk(NB=0)) == -1 and b"direction map needs num_dir_bins > 0" in err()
    assert loss(cfg, ws=16) == -1 and b"workspace 16 <" in err()
    assert loss(lk(B=256)) == -1 and b"anchor_loss: at most 255 frames" in err()
    assert loss(lk(H=4096, W=2048)) == -1 and b"at most 2^22 anchors per frame" in err()
    assert loss(lk(M=2000)) == -1 and b"got M = 2000" in err()
    assert loss(lk(C=0)) == -1 and b"bad class / direction-bin count" in err()
    assert loss(lk(beta=0.0)) == -1 and b"beta >= 1e-5" in err()
    assert grad(cfg, up=None) == -1 and b"anchor_loss_grad: null gradient" in err()
    assert grad(cfg, gdir=None) == -1 and b"anchor_loss_grad: null gradient" in err()
    assert grad(cfg, ld_g=(2, 13, 4)) == -1 and b"gradient row stride is smaller" in err()
    assert grad(lk(B=256)) == -1 and b"anchor_loss_grad: at most 255 frames" in err()
    with pytest.raises(ValueError, match="code_weights must have 7"):
        ops.anchor_loss_cfg(1, 4, 4, 8, 1, 2, [0, 0], TABLE, 1, 1.0, 2.0, 0.2, [1.0] * 8)

    # ---- the product ops refuse CPU tensors and wrong shapes
    with pytest.raises(_lib.Df3dError):
        ops.anchor_assign(torch.zeros(1, 4), torch.zeros(1, 2), torch.zeros(1, 3, 8), 2, 4, [0, 0], TABLE, [1], [0.6], [0.45])


def test_refusals_name_the_key():
    from dualfusion import dense_heads
    base = al.train_head_cfg("car")

    def assigner(target=None, **top):
        cfg = copy.deepcopy(base)
        cfg["TARGET_ASSIGNER_CONFIG"].update(target or {})
        cfg.update(top)
        return dense_heads.AxisAlignedTargetAssigner(cfg, ["Car"], dense_heads.ResidualCoder())

    a = assigner()
    assert a.set_class == [1] and a.matched_thresholds == [0.6] and a.unmatched_thresholds == [0.45] and a.box_coder.code_size == 7
    with pytest.raises(NotImplementedError, match="POS_FRACTION"):
        assigner({"POS_FRACTION": 0.5})
    with pytest.raises(NotImplementedError, match="POS_FRACTION"):
        assigner({"POS_FRACTION": 0.0})
    with pytest.raises(NotImplementedError, match="MATCH_HEIGHT"):
        assigner({"MATCH_HEIGHT": True})
    with pytest.raises(NotImplementedError, match="MATCH_HEIGHT"):
        dense_heads.AxisAlignedTargetAssigner(base, ["Car"], dense_heads.ResidualCoder(), match_height=True)
    with pytest.raises(NotImplementedError, match="NORM_BY_NUM_EXAMPLES"):
        assigner({"NORM_BY_NUM_EXAMPLES": True})
    with pytest.raises(NotImplementedError, match="NAME: ATSS"):
        assigner({"NAME": "ATSS"})
    with pytest.raises(NotImplementedError, match="USE_MULTIHEAD"):
        assigner(USE_MULTIHEAD=True)
    with pytest.raises(ValueError, match="not one of class_names"):
        dense_heads.AxisAlignedTargetAssigner(base, ["Van"], dense_heads.ResidualCoder())
    with pytest.raises(TypeError, match="AnchorTables"):
        a.assign_targets([torch.zeros(4, 7)], torch.zeros(1, 2, 8))
    head = build_head("car", LOSS_CONFIG={"REG_LOSS_TYPE": "WeightedL1Loss", "LOSS_WEIGHTS": dict(al.LOSS_WEIGHTS)})
    with pytest.raises(NotImplementedError, match="REG_LOSS_TYPE"):
        head._training_setup()
    cfg = al.train_head_cfg("car")
    del cfg["LOSS_CONFIG"]
    grid, rng = vt.case_geometry("car")
    with pytest.raises(KeyError, match="LOSS_CONFIG"):
        dense_heads.AnchorHeadSingle(cfg, 16, 1, ["Car"], grid, rng)._training_setup()


def test_forward_in_training_mode_still_refuses_next_to_forward_train():
    head = build_head("car").train()
    assert head.forward_ret_dict == {} and callable(head.forward_train) and callable(head.get_loss)
    with pytest.raises(NotImplementedError, match="eval mode only") as e:
        head({"spatial_features_2d": torch.zeros(1, 16, 25, 22), "batch_size": 1})
    assert "forward_train" in str(e.value)
    from dualfusion import dense_heads
    assert dense_heads.anchor_loss_fused() is True


def test_switch_is_read_per_call(monkeypatch):
    from dualfusion import dense_heads
    monkeypatch.setenv("DF3D_ANCHOR_LOSS_FUSED", "0")
    assert dense_heads.anchor_loss_fused() is False
    monkeypatch.setenv("DF3D_ANCHOR_LOSS_FUSED", "1")
    assert dense_heads.anchor_loss_fused() is True


def bound(want):
    return 8 * vt.U32 * np.abs(want).max()


@pytest.mark.parametrize("name", ["car", "small", "multi", "nodir"])
def test_float64_restatement_against_the_reference(g, restated, name):
    a, l = restated[name]
    c, src = vt.CASES[name], al.source(name)
    assert a["labels"].dtype == np.int32 and np.array_equal(a["labels"], g[name + "_labels"])
    assert np.array_equal(a["weights"], g[name + "_weights"])
    assert np.array_equal(a["gt_ids"] >= 0, a["labels"] > 0)          # (thresholds are ordered: an id exactly at the positives)
    gt = g[src + "_gt"]
    for b in range(c["B"]):                                           # the ids name rows of the frame's class
        pos = a["labels"][b] > 0
        assert np.array_equal(gt[b, a["gt_ids"][b][pos], 7].astype(np.int32), a["labels"][b][pos])
    assert np.abs(a["targets"] - g[name + "_targets"]).max() <= bound(g[name + "_targets"])
    want = g[name + "_loss"]
    # a float32 sum of n terms: n roundings at the most; the reference sums [B, N, C] maps
    n_terms = a["labels"].size * c["C"]
    assert np.abs(l["loss"] - want).max() <= n_terms * vt.U32 * np.abs(want).max()
    # grad_box: below beta the gradient is diff / beta, and the float32 diff of code 6 is sin cos - cos sin of an O(1) target
    # held in float32: ~4 roundings of magnitude <= pi, times 1 / beta = 9 -> 64 roundings of the largest gradient
    # grad_cls / grad_dir: float32 autograd chains of about a dozen operations (pow, log1p, exp, products), each one rounding
    # of a term that can exceed the result: 32 roundings of the largest gradient
    for k, ulps in (("grad_cls", 32), ("grad_box", 64)) + ((("grad_dir", 32),) if c["NB"] else ()):
        assert np.abs(l[k] - g[name + "_" + k]).max() <= ulps * vt.U32 * np.abs(g[name + "_" + k]).max(), k
    if not c["NB"]:
        assert l["grad_dir"] is None and want[2] == 0 and name + "_grad_dir" not in g


def test_fixture_margins_and_coverage(g, restated):
    for name in vt.CASES:
        a, l = restated[name]
        assert a["thresh_dist"] >= al.THRESH_MARGIN and a["argmax_ties"] == 0 and a["positive_gap"] >= al.GAP_MARGIN
        assert a["gt_gap_bad"] == 0 and l["beta_dist"] >= al.BETA_MARGIN
        assert not vt.CASES[name]["NB"] or l["floor_dist"] >= al.FLOOR_MARGIN
        assert a["num_pos"][-1] == 0 and (a["labels"][-1] == 0).all()         # the empty frame
        assert a["labels"].shape[1] <= 1100
    car, multi = restated["car"][0], restated["multi"][0]
    assert car["forced_below"] > 0 and multi["forced_only"] > 0 and car["ignored"] > 0 and car["unmatched_gt"] > 0
    assert restated["car"][1]["bins"] == {0, 1}
    gt = g["car_gt"]
    zero = np.abs(gt[..., :7]).sum(-1) == 0
    assert zero[2].all() and not zero[1].any()                                  # an empty frame, a frame that fills all M rows
    n0 = al.valid_count(gt[0])
    assert zero[0, :n0].sum() == 1 and n0 == gt.shape[1] - 2                    # an interior all-zero row
    assert (gt[1, :, 7] == 2).sum() == 1 and gt[1, 1, 0] > 20                   # a class without anchors, a GT outside the range
    assert set(np.unique(restated["multi"][0]["labels"])) == {-1, 0, 1, 2, 3}
    assert al.valid_count(np.zeros((4, 8), np.float32)) == 1
    for k, v in g.items():
        assert v.nbytes < 400 * 1024, k


def test_composed_assignment_and_losses_on_the_cpu_match_the_reference(g, monkeypatch):
    """The composed mode is the reference's formulation in torch: on the CPU it gives the reference's labels exactly and its
    values within float32 rounding."""
    from dualfusion import dense_heads
    monkeypatch.setenv("DF3D_ANCHOR_LOSS_FUSED", "0")
    for name in ("car", "multi", "nodir"):
        c, src = vt.CASES[name], al.source(name)
        head = build_head(name).train()
        t = head.assign_targets(torch.from_numpy(g[src + "_gt"]))
        assert t["box_cls_labels"].dtype == torch.int32 and t["box_reg_targets"].dtype == torch.float32
        assert np.array_equal(t["box_cls_labels"].numpy(), g[name + "_labels"])
        assert np.array_equal(t["reg_weights"].numpy(), g[name + "_weights"])
        assert np.abs(t["box_reg_targets"].numpy() - g[name + "_targets"]).max() <= bound(g[name + "_targets"])
        assert np.array_equal(t["gt_ids"].numpy(), al.restate(name, g)[0]["gt_ids"])
        view = lambda v: torch.from_numpy(v.copy()).view(c["B"], c["H"], c["W"], -1).requires_grad_(True)
        ret = {"cls_preds": view(g[src + "_cls"]), "box_preds": view(g[src + "_box"])}
        if c["NB"]:
            ret["dir_cls_preds"] = view(g[src + "_dir"])
        ret.update(t)
        head.forward_ret_dict = ret
        loss, tb = head.get_loss()
        loss.backward()
        want = g[name + "_loss"]
        keys = ["rpn_loss_cls", "rpn_loss_loc"] + (["rpn_loss_dir"] if c["NB"] else [])
        assert sorted(tb) == sorted(keys + ["rpn_loss"]) and all(isinstance(v, torch.Tensor) for v in tb.values())
        for j, k in enumerate(keys):
            assert abs(float(tb[k]) - want[j]) <= 64 * vt.U32 * abs(want[j]), (name, k)
        assert abs(float(loss.detach()) - want.sum()) <= 64 * vt.U32 * want.sum()
        for k, p in (("grad_cls", "cls_preds"), ("grad_box", "box_preds"), ("grad_dir", "dir_cls_preds")):
            if p in ret:
                got = ret[p].grad.reshape(g[name + "_" + k].shape).numpy()
                assert np.abs(got - g[name + "_" + k]).max() <= 8 * bound(g[name + "_" + k]), (name, k)
    assert isinstance(head.target_assigner, dense_heads.AxisAlignedTargetAssigner)
