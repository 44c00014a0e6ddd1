"""The proposal targets and the RCNN losses on the device (csrc/roiloss.hip, dualfusion/ops.py, roi_heads.py) against the
reference's results (tests/golden/roi_loss.npz) and the float64 restatement (tests/roiloss_reference.py).

Sampled RoI indices, labels, masks and counts are compared exactly: the fixture's margins (no max IoU within 1e-4 of a
threshold, best and second-best IoU 1e-6 apart, folded heading 1e-3 from a branch point, no |diff| within 1e-4 of beta, no
corner distance within 1e-4 of 1, distinct keys) make a mismatch a bug and not rounding.  Values are judged by the project's
yardstick (tests/test_gpu_vrtail.judge): per tensor, the reference's float32 result against the float64 restatement gives
max error over max magnitude; the device may deviate from the restatement at most 4 x that.  Both numbers are printed.  The
sticky range flag is checked after every test (tests/conftest.py)."""
import copy

import numpy as np
import pytest

import roiloss_reference as rl
import vrtail_reference as vt
from test_gpu_vrtail import dev, judge

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

INPUT_KEYS = ("rois", "roi_scores", "roi_labels", "gt", "u_fg", "u_slot")
TARGET_KEYS = ("rois", "gt_of_rois", "gt_of_rois_src", "gt_iou_of_rois", "roi_scores", "roi_labels", "reg_valid_mask", "rcnn_cls_labels")


@pytest.fixture(scope="module")
def g(golden):
    return golden("roi_loss.npz")


@pytest.fixture(scope="module")
def restated(g):
    """computed once, shared, never modified"""
    return {name: rl.restate(name, g) for name in rl.CASES}


def run_targets(name, g, composed=False, **edit):
    from dualfusion import ops, roi_heads
    args = [dev(g[name + "_" + k]) for k in INPUT_KEYS]
    fn = roi_heads.composed_roi_targets if composed else ops.roi_targets
    out = fn(*args, dict(rl.sampler_cfg(name), **edit))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def check_exact(name, g, t, out):
    assert out["roi_inds"].dtype == np.int32 and out["reg_valid_mask"].dtype == np.int32 and out["counts"].dtype == np.int32
    assert out["roi_labels"].dtype == np.int64 and out["rcnn_cls_labels"].dtype == np.float32
    assert np.array_equal(out["counts"], t["counts"])
    assert np.array_equal(out["roi_inds"], t["inds"])
    assert np.array_equal(out["rois"], g[name + "_t_rois"])                      # the sampled indices, through the gathered rows
    assert np.array_equal(out["roi_labels"], g[name + "_t_roi_labels"]) and np.array_equal(out["roi_scores"], g[name + "_t_roi_scores"])
    assert np.array_equal(out["reg_valid_mask"], g[name + "_t_reg_valid_mask"])
    assert np.array_equal(out["gt_of_rois_src"], g[name + "_t_gt_of_rois_src"])


@pytest.mark.parametrize("name", list(rl.CASES))
def test_targets_on_the_golden_inputs(g, restated, name):
    t, _ = restated[name]
    soft, hard = run_targets(name, g, CLS_SCORE_TYPE="roi_iou"), run_targets(name, g, CLS_SCORE_TYPE="cls")
    for out in (soft, hard):
        check_exact(name, g, t, out)
    assert np.array_equal(hard["rcnn_cls_labels"], g[name + "_t_cls_labels_cls"]) and (hard["rcnn_cls_labels"] == -1).any()
    ends = np.isin(t["cls_labels_roi_iou"], (0.0, 1.0))
    assert np.array_equal(soft["rcnn_cls_labels"][ends], g[name + "_t_cls_labels_roi_iou"][ends])
    judge("targets " + name, [("gt_iou_of_rois", t["gt_iou_of_rois"], g[name + "_t_gt_iou_of_rois"], soft["gt_iou_of_rois"]),
                              ("rcnn_cls_labels (roi_iou)", t["cls_labels_roi_iou"], g[name + "_t_cls_labels_roi_iou"], soft["rcnn_cls_labels"]),
                              ("gt_of_rois", t["gt_of_rois"], g[name + "_t_gt_of_rois"], soft["gt_of_rois"])])


def golden_targets(name, g):
    t = {k: dev(g[name + "_t_" + k]) for k in TARGET_KEYS}
    t["reg_valid_mask"] = t["reg_valid_mask"].to(torch.int32)
    t["rcnn_cls_labels"] = t["rcnn_cls_labels"].float()
    return t


def run_loss(name, g, upstream=(1.0, 1.0, 1.0), composed=False, pad=0):
    """losses + backward on the golden targets and predictions -> losses [3], grad_cls [N, 1], grad_reg [N, 7]; pad > 0: the two
    inputs are column blocks of one wider row buffer"""
    from dualfusion import ops, roi_heads
    w = rl.LOSS_CFG["LOSS_WEIGHTS"]
    spec = ops.RcnnLossSpec(w["rcnn_cls_weight"], w["rcnn_reg_weight"], w["rcnn_corner_weight"], w["code_weights"])
    n = rl.B * rl.M
    wide = torch.full((n, 8 + 3 * pad), 1e30, device="cuda")
    wide[:, pad:pad + 1], wide[:, 2 * pad + 1:2 * pad + 8] = dev(g[name + "_rcnn_cls"]), dev(g[name + "_rcnn_reg"])
    wide.requires_grad_(True)
    cls, reg = wide[:, pad:pad + 1], wide[:, 2 * pad + 1:2 * pad + 8]
    fn = roi_heads.composed_rcnn_losses if composed else ops.rcnn_loss
    losses = fn(cls, reg, golden_targets(name, g), spec)
    (losses * torch.tensor(upstream, device="cuda")).sum().backward()
    torch.cuda.synchronize()
    grad = wide.grad.cpu().numpy()
    return losses.detach().cpu().numpy(), grad[:, pad:pad + 1], grad[:, 2 * pad + 1:2 * pad + 8]


def loss_pairs(name, g, l, got):
    return [("losses", l["loss"], g[name + "_loss"], got[0]), ("grad_cls", l["grad_cls"], g[name + "_grad_cls"], got[1]),
            ("grad_reg", l["grad_reg"], g[name + "_grad_reg"], got[2])]


@pytest.mark.parametrize("name", list(rl.CASES))
def test_losses_and_gradients_on_the_golden_targets(g, restated, name):
    t, l = restated[name]
    got = run_loss(name, g)
    assert got[0].dtype == np.float32 and got[0].shape == (3,) and got[1].shape == (rl.B * rl.M, 1) and got[2].shape == (rl.B * rl.M, 7)
    mask, labels = g[name + "_t_reg_valid_mask"].reshape(-1), g[name + "_t_rcnn_cls_labels"].reshape(-1)
    assert not got[2][mask == 0].any() and got[2][mask > 0].all()               # zeros exactly where nothing contributes
    assert not got[1][labels < 0].any() and got[1][labels >= 0].all()
    judge("loss " + name, loss_pairs(name, g, l, got))
    padded = run_loss(name, g, pad=3)                                            # row views of a wider buffer: the same bits
    assert all(np.array_equal(x, y) for x, y in zip(got, padded))


def test_upstream_gradients_are_honoured(g, restated):
    t, _ = restated["iou"]
    up = (0.5, 2.0, -3.0)
    l = rl.losses(g["iou_rcnn_cls"], g["iou_rcnn_reg"], t["rois"], t["gt_of_rois"], t["gt_of_rois_src"], t["reg_valid_mask"], t["rcnn_cls_labels"],
                  upstream=up)
    _, g_cls, g_reg = run_loss("iou", g, upstream=up)
    # fp64 arithmetic on float32 targets, rounded once: the rounding of a target (2^-24 of its magnitude) enters the quadratic
    # branch divided by beta = 1/9; 64 roundings of the largest entry bound it with room
    for got, want in ((g_cls, l["grad_cls"]), (g_reg, l["grad_reg"])):
        err = np.abs(got - want).max() / np.abs(want).max()
        print("upstream %.3e" % err)
        assert err <= 64 * vt.U32


def test_no_foreground_row_and_no_valid_row():
    """fg_sum = 0 and valid = 0: the normalisers clamp to 1 on the device, the corner loss is 0, every gradient is 0"""
    from dualfusion import ops
    n = 40
    rs = np.random.RandomState(3)
    t = {"rois": dev(rs.uniform(1, 2, (n, 7)).astype(np.float32)), "gt_of_rois": dev(rs.uniform(1, 2, (n, 8)).astype(np.float32)),
         "gt_of_rois_src": dev(rs.uniform(1, 2, (n, 8)).astype(np.float32)), "reg_valid_mask": torch.zeros(n, dtype=torch.int32, device="cuda"),
         "rcnn_cls_labels": torch.full((n,), -1.0, device="cuda")}
    cls, reg = torch.randn(n, 1, device="cuda", requires_grad=True), torch.randn(n, 7, device="cuda", requires_grad=True)
    losses = ops.rcnn_loss(cls, reg, t, ops.RcnnLossSpec(1.0, 1.0, 1.0, [1.0] * 7))
    losses.sum().backward()
    torch.cuda.synchronize()
    assert not losses.detach().cpu().numpy().any() and not cls.grad.cpu().numpy().any() and not reg.grad.cpu().numpy().any()


@pytest.mark.parametrize("name", list(rl.CASES))
def test_fused_and_composed_agree(g, restated, name):
    """the composed formulation on the device as a second implementation: indices, labels, masks and counts exactly, values
    and losses by the yardstick"""
    t, l = restated[name]
    fused, composed = run_targets(name, g), run_targets(name, g, composed=True)
    check_exact(name, g, t, composed)
    key = "cls_labels_" + rl.CASES[name]["score"]
    for what, out in (("fused", fused), ("composed", composed)):
        judge("%s targets %s" % (what, name), [("gt_iou_of_rois", t["gt_iou_of_rois"], g[name + "_t_gt_iou_of_rois"], out["gt_iou_of_rois"]),
                                               ("rcnn_cls_labels", t[key], g[name + "_t_" + key], out["rcnn_cls_labels"]),
                                               ("gt_of_rois", t["gt_of_rois"], g[name + "_t_gt_of_rois"], out["gt_of_rois"])])
    judge("composed loss " + name, loss_pairs(name, g, l, run_loss(name, g, composed=True)))
    judge("fused loss " + name, loss_pairs(name, g, l, run_loss(name, g)))


# ---------------------------------------------------------------------------------------------------- the head
def small_head(seed):
    from dualfusion import roi_heads
    import test_gpu_roipool as rp
    torch.manual_seed(seed)
    cfg = dict(rp.head_cfg(), DP_RATIO=0.0, TARGET_CONFIG=dict(rl.sampler_cfg("iou"), ROI_PER_IMAGE=12), LOSS_CONFIG=copy.deepcopy(rl.LOSS_CFG))
    head = roi_heads.VoxelRCNNHead({n: c for n, _, c in rp.HEAD_LEVELS}, cfg, rp.HEAD_RANGE, rp.HEAD_VOXEL).train()
    with torch.no_grad():                                                        # logits and residuals of a useful size
        head.cls_pred_layer.weight.normal_(0, 0.3)
        head.reg_pred_layer.weight.normal_(0, 0.03)
    return head


def head_inputs(seed, R=40):
    """two frames inside the range of tests/test_gpu_roipool.py's tiny sparse levels: four boxes each, RoIs around them"""
    import roipool_reference as ref
    import test_gpu_roipool as rp
    from dualfusion.spconv import SparseConvTensor
    rs = np.random.RandomState(seed)
    gt = np.zeros((2, 6, 8), np.float32)
    for b in range(2):
        gt[b, :4, 0], gt[b, :4, 1], gt[b, :4, 2] = rs.uniform(0.5, 5.5, 4), rs.uniform(-1.6, 1.6, 4), rs.uniform(0.4, 0.6, 4)
        gt[b, :4, 3:6] = np.array([1.6, 0.8, 0.6]) * rs.uniform(0.8, 1.25, (4, 3))
        gt[b, :4, 6], gt[b, :4, 7] = rs.uniform(-np.pi, np.pi, 4), rs.randint(1, 4, 4)
    src = gt[np.arange(2)[:, None], rs.randint(0, 4, (2, R))]
    scale = rs.choice([0.03, 0.12, 0.3, 2.0], (2, R, 1))
    rois = src[..., :7].copy()
    rois[..., 0:3] += rs.normal(0, 1, (2, R, 3)) * scale * src[..., 3:6]
    rois[..., 3:6] *= np.exp(rs.normal(0, 0.1, (2, R, 3)))
    rois[..., 6] += rs.normal(0, 0.2, (2, R)) + np.pi * (rs.uniform(0, 1, (2, R)) < 0.3)
    rois = rois.astype(np.float32)
    labels = src[..., 7].astype(np.int64)
    fx = rp.fixture(0)
    tensors = {}
    for name, stride, c in rp.HEAD_LEVELS:
        ind = fx["indices"].astype(np.int64)
        ind = np.unique(np.concatenate([ind[:, :1], ind[:, 1:] // stride], 1), axis=0)
        ind = np.ascontiguousarray(ind[np.argsort(ind[:, 0], kind="stable")].astype(np.int32))
        shape = [-(-s // stride) for s in ref.GRID]
        tensors[name] = SparseConvTensor(dev(rs.standard_normal((len(ind), c)).astype(np.float32)), dev(ind), shape, 2)
    u_fg = rs.uniform(0, 1, (2, R)).astype(np.float32)
    u_slot = np.minimum(rs.uniform(0, 1, (2, 12)).astype(np.float32), np.float32(1 - 2.0 ** -24))
    return rois, labels, gt, u_fg, u_slot, tensors, {n: s for n, s, _ in rp.HEAD_LEVELS}


def run_head(head, inputs, mode, monkeypatch):
    """forward_train + get_loss().backward() -> the head's ret dict as numpy, the inputs of the two prediction layers, the
    parameter gradients and the loss parts"""
    rois, labels, gt, u_fg, u_slot, tensors, strides = inputs
    monkeypatch.setenv("DF3D_ROI_LOSS_FUSED", mode)
    hd = copy.deepcopy(head).cuda()
    seen = {}
    hooks = [hd.cls_pred_layer.register_forward_hook(lambda m, i, o: seen.__setitem__("cls", i[0].detach().double().cpu().numpy())),
             hd.reg_pred_layer.register_forward_hook(lambda m, i, o: seen.__setitem__("reg", i[0].detach().double().cpu().numpy()))]
    batch = {"batch_size": 2, "rois": dev(rois), "roi_labels": dev(labels), "gt_boxes": dev(gt), "multi_scale_3d_features": tensors,
             "multi_scale_3d_strides": strides}
    out = hd.forward_train(batch, u_fg=dev(u_fg), u_slot=dev(u_slot))
    assert out is batch and tuple(out["rois"].shape) == (2, 12, 7) and tuple(out["roi_labels"].shape) == (2, 12)
    r = hd.forward_ret_dict
    assert out["rois"] is r["rois"] and tuple(r["rcnn_cls"].shape) == (24, 1) and tuple(r["rcnn_reg"].shape) == (24, 7) and r["rcnn_cls"].requires_grad
    loss, tb = hd.get_loss()
    assert sorted(tb) == ["rcnn_loss", "rcnn_loss_cls", "rcnn_loss_corner", "rcnn_loss_reg"]
    assert all(isinstance(v, torch.Tensor) and v.is_cuda and not v.requires_grad for v in tb.values())
    loss.backward()
    torch.cuda.synchronize()
    for h in hooks:
        h.remove()
    grads = {k: p.grad.cpu().numpy() for k, p in hd.named_parameters() if k.startswith(("cls_pred_layer", "reg_pred_layer"))}
    assert bool(hd.shared_fc_layer[0].weight.grad.abs().sum() > 0)              # the gradient reaches the layers in front
    parts = np.array([float(tb[k]) for k in ("rcnn_loss_cls", "rcnn_loss_reg", "rcnn_loss_corner")])
    return {k: v.detach().cpu().numpy() for k, v in r.items()}, seen, grads, parts, float(loss.detach())


def float64_composition(r, seen):
    """the losses and the gradients of the two prediction layers in float64, from the targets and predictions the device made"""
    l = rl.losses(r["rcnn_cls"], r["rcnn_reg"], r["rois"], r["gt_of_rois"], r["gt_of_rois_src"], r["reg_valid_mask"], r["rcnn_cls_labels"])
    want = {"cls_pred_layer.weight": l["grad_cls"].T @ seen["cls"], "cls_pred_layer.bias": l["grad_cls"].sum(0),
            "reg_pred_layer.weight": l["grad_reg"].T @ seen["reg"], "reg_pred_layer.bias": l["grad_reg"].sum(0)}
    return l, want


def test_parameter_gradients_through_forward_train(monkeypatch):
    """forward_train + get_loss().backward() on a small head with given RoIs, fused and composed.  The yardstick: the composed
    float32 formulation (torch autograd on the device) against the float64 composition on the predictions IT made; the fused
    mode against the float64 composition on its own, at most 4 x the yardstick."""
    for seed in range(16):
        head, inputs = small_head(100 + seed), head_inputs(200 + seed)
        t = rl.targets(inputs[0], np.zeros(inputs[1].shape), inputs[1], inputs[2], inputs[3], inputs[4], dict(rl.sampler_cfg("iou"), ROI_PER_IMAGE=12))
        if not (rl.targets_clean(t) and t["reg_valid_mask"].sum() >= 4 and (t["counts"][:, 0] > 0).all()):
            continue
        composed = run_head(head, inputs, "0", monkeypatch)
        l0, want0 = float64_composition(composed[0], composed[1])
        if rl.loss_clean(l0):
            break
    else:
        raise AssertionError("no clean seed")
    fused = run_head(head, inputs, "1", monkeypatch)
    l1, want1 = float64_composition(fused[0], fused[1])
    assert rl.loss_clean(l1)                                                     # the margins hold on the fused run's predictions too
    failures = []
    for what, (r, _, grads, parts, total), l, want in (("composed", composed, l0, want0), ("fused", fused, l1, want1)):
        assert np.array_equal(r["roi_inds"], t["inds"]) and np.array_equal(r["counts"], t["counts"]), what
        assert np.array_equal(r["reg_valid_mask"], t["reg_valid_mask"]) and np.array_equal(r["rois"], inputs[0][np.arange(2)[:, None], t["inds"]])
        # float32 results of sums over 24 x 8 terms: 64 roundings of the largest
        assert np.abs(parts - l["loss"]).max() <= 64 * vt.U32 * np.abs(l["loss"]).max(), what
        assert abs(total - l["loss"].sum()) <= 64 * vt.U32 * l["loss"].sum()
        assert sorted(grads) == sorted(want)
    for k in sorted(want1):
        y, d = vt.rel_err(composed[2][k], want0[k]), vt.rel_err(fused[2][k], want1[k])
        print("%-24s float32 yardstick (composed) %.3e  fused %.3e" % (k, y, d))
        if not d <= 4 * y:
            failures.append((k, y, d))
    assert not failures, failures


def test_the_caps_of_the_proposal_layer_and_the_sampler():
    """R = 4096 and M = 512 on two frames against the restatement: indices and counts exact (the seed is searched on the host
    until the margins hold)"""
    from dualfusion import ops
    R, m = ops.ROI_MAX_ROIS, 512
    cfg = rl.sampler_cfg("wide", m=m)
    for seed in range(64):
        rois, scores, labels, gt, u_fg, u_slot = rl.make_inputs("wide", 900 + seed, R=R, m=m, plans=[(600, 1000, R - 1600), (100, 200, R - 300)])
        t = rl.targets(rois, scores, labels, gt, u_fg, u_slot, cfg)
        if rl.targets_clean(t) and rl.keys_distinct(u_fg):
            break
    else:
        raise AssertionError("no clean seed")
    out = ops.roi_targets(dev(rois), dev(scores), dev(labels), dev(gt), dev(u_fg), dev(u_slot), cfg)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    assert np.array_equal(out["counts"], t["counts"]) and np.array_equal(out["counts"], [[600, 1000, R - 1600], [100, 200, R - 300]])
    assert np.array_equal(out["roi_inds"], t["inds"]) and out["roi_inds"].max() > 4000
    assert len(np.unique(out["roi_inds"][0, :256])) == 256                       # F = round(0.5 * 512) distinct fg RoIs
    assert np.array_equal(out["rois"], rois[np.arange(2)[:, None], t["inds"]]) and np.array_equal(out["roi_labels"], t["roi_labels"])
    assert np.array_equal(out["reg_valid_mask"], t["reg_valid_mask"]) and np.array_equal(out["rcnn_cls_labels"], t["cls_labels_cls"])
    # one rounding of a float64 value to float32, and a last-place difference of the two float64 evaluations in front of it
    for k in ("gt_iou_of_rois", "gt_of_rois"):
        assert np.abs(out[k] - t[k]).max() <= 2 * vt.U32 * np.abs(t[k]).max(), k


def test_the_modules_own_draws_select_every_foreground_roi_equally_often(g, restated):
    """200 seeded calls on the mixed frame 0 of 'iou' (n_fg = 20, F = 8): every fg RoI's selection count lies within 5 binomial
    standard deviations of 200 * F / n_fg"""
    from dualfusion import roi_heads
    t, _ = restated["iou"]
    n_fg, F, calls = int(t["counts"][0, 0]), 8, 200
    layer = roi_heads.ProposalTargetLayer(rl.sampler_cfg("iou"), generator=torch.Generator(device="cuda").manual_seed(11))
    batch = {"rois": dev(g["iou_rois"][:1]), "roi_scores": dev(g["iou_roi_scores"][:1]), "roi_labels": dev(g["iou_roi_labels"][:1]),
             "gt_boxes": dev(g["iou_gt"][:1])}
    picked = torch.stack([layer(batch)["roi_inds"][0] for _ in range(calls)]).cpu().numpy()
    fg = np.nonzero(t["ious_all"][0] >= 0.55)[0]
    assert len(fg) == n_fg == 20 and np.isin(picked[:, :F], fg).all() and not np.isin(picked[:, F:], fg).any()
    assert all(len(set(row[:F])) == F for row in picked)                         # without replacement
    counts = np.array([(picked[:, :F] == i).sum() for i in fg])
    p = F / n_fg
    sigma = np.sqrt(calls * p * (1 - p))
    print("selection counts", counts.tolist(), "expected %.1f +- %.1f" % (calls * p, sigma))
    assert np.abs(counts - calls * p).max() <= 5 * sigma
    again = roi_heads.ProposalTargetLayer(rl.sampler_cfg("iou"), generator=torch.Generator(device="cuda").manual_seed(11))
    assert np.array_equal(again(batch)["roi_inds"].cpu().numpy()[0], picked[0])  # reproducible from the seed


def test_targets_loss_and_backward_make_the_host_wait_for_nothing(g, restated):
    """Under torch's synchronisation debug mode any read of a device value by the host raises."""
    from dualfusion import ops
    t, _ = restated["iou"]
    args = [dev(g["iou_" + k]) for k in INPUT_KEYS]
    cls, reg = dev(g["iou_rcnn_cls"]).requires_grad_(True), dev(g["iou_rcnn_reg"]).requires_grad_(True)
    up = torch.tensor([1.0, 1.0, 1.0], device="cuda")
    w = rl.LOSS_CFG["LOSS_WEIGHTS"]
    cfg = rl.sampler_cfg("iou")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = ops.roi_targets(*args, cfg)
        spec = ops.RcnnLossSpec(w["rcnn_cls_weight"], w["rcnn_reg_weight"], w["rcnn_corner_weight"], w["code_weights"])
        losses = ops.rcnn_loss(cls, reg, out, spec)
        (losses * up).sum().backward()
        with pytest.raises(RuntimeError, match="synchroniz"):
            out["counts"].tolist()                                              # the mode does see a read
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert np.array_equal(out["roi_inds"].cpu().numpy(), t["inds"])
    assert np.abs(losses.detach().cpu().numpy() - g["iou_loss"]).max() <= 64 * vt.U32 * g["iou_loss"].max()
    assert cls.grad is not None and reg.grad is not None


def test_results_are_bit_identical_from_run_to_run(g):
    first, second = run_targets("wide", g), run_targets("wide", g)
    for k in first:
        assert np.array_equal(first[k].view(np.uint32) if first[k].dtype == np.float32 else first[k],
                              second[k].view(np.uint32) if second[k].dtype == np.float32 else second[k]), k
    a, b = run_loss("wide", g), run_loss("wide", g)
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))
