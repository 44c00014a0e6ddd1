"""The PV-RCNN point head and detector on the device (csrc/pointhead.hip, dualfusion/dense_heads.py PointHeadSimple,
dualfusion/vr_detector.py PVRCNN) against the float32 restatement of tests/pointhead_reference.py and the reference's results
(tests/golden/point_head.npz).

Labels and box indices are compared exactly: every fixture is margin-clean (near_face == 0, asserted on the host), so a
mismatch is a bug and not rounding.  Loss values and gradients are judged by the project's yardstick (test_gpu_vrtail.judge):
the reference's float32 result against the float64 restatement gives max error over max magnitude; the device may deviate from
the restatement at most 4 x that.  Both numbers are printed.

Measured on an MI355X (this file's prints): see DESIGN section 7.18."""
import copy

import numpy as np
import pytest

import pointhead_reference as pr

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
UPSTREAM = 2.5          # tests/golden/make_golden_pointhead.py


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def g(golden):
    return golden("point_head.npz")


@pytest.fixture(scope="module")
def cases():
    return {name: pr.target_case(name) for name in pr.TARGET_CASES}


def fused_only(monkeypatch):
    """DF3D_POINT_HEAD_FUSED=1 -> the list that collects the names of the point-head kernels' wrappers as they are called"""
    from dualfusion import ops
    monkeypatch.setenv("DF3D_POINT_HEAD_FUSED", "1")
    calls = []

    def counted(name, real):
        def call(*a, **k):
            calls.append(name)
            return real(*a, **k)
        return call
    for name in ("point_head_targets", "point_cls_loss"):
        monkeypatch.setattr(ops, name, counted(name, getattr(ops, name)))
    return calls


def composed_only(monkeypatch):
    """DF3D_POINT_HEAD_FUSED=0, and the kernels raise if they are reached anyway"""
    from dualfusion import ops
    monkeypatch.setenv("DF3D_POINT_HEAD_FUSED", "0")

    def refuse(*a, **k):
        raise AssertionError("a point-head kernel was called with DF3D_POINT_HEAD_FUSED=0")
    for name in ("point_head_targets", "point_cls_loss", "points_in_boxes"):
        monkeypatch.setattr(ops, name, refuse)


# ---------------------------------------------------------------------------------------------------------------- targets
@pytest.mark.parametrize("num_class", [1, 3])
@pytest.mark.parametrize("name", pr.TARGET_CASES)
def test_targets_equal_the_restatement_and_the_reference(name, num_class, cases, g):
    from dualfusion import ops
    points, gt, extra = cases[name]
    labels, idx = ops.point_head_targets(dev(points), dev(gt), extra, num_class, want_box_idx=True)
    only = ops.point_head_targets(dev(points), dev(gt), extra, num_class)
    torch.cuda.synchronize()
    want = pr.assign_targets(points, gt, extra, num_class)
    assert labels.dtype == torch.int64 and idx.dtype == torch.int32 and tuple(labels.shape) == (len(points),)
    assert np.array_equal(labels.cpu().numpy(), want[0]) and np.array_equal(idx.cpu().numpy(), want[1])
    assert np.array_equal(labels.cpu().numpy(), g["%s_labels_c%d" % (name, num_class)])
    assert torch.equal(only, labels)
    if name == "main":
        rows = pr.MAIN_ROWS
        got = labels.cpu().numpy()
        assert got[rows["on_face"]] == 1 and got[rows["padding_hit"]] == -1 and got[rows["ext_only"]] == -1 and got[rows["stray"]] == 0
        assert got[rows["in_both"]] == (1 if num_class == 1 else gt[0, 0, 7])
    if name == "chunk":
        assert int(idx[0]) == 129 and int(idx[1]) == 128                        # the second LDS chunk, its last box included
    if name == "interleaved":
        perm = pr.interleaved(cases["main"][0])[1]
        stacked = ops.point_head_targets(dev(cases["main"][0]), dev(gt), extra, num_class)
        assert torch.equal(labels, stacked[torch.from_numpy(perm).cuda()])


@pytest.mark.parametrize("name", ["main", "chunk", "negative_extra"])
def test_points_in_boxes_and_the_shim(name, cases):
    from dualfusion import ext, ops
    shim = ext.load("roiaware_pool3d_cuda")
    points, gt, _ = cases[name]
    for b in range(gt.shape[0]):
        pts = points[points[:, 0] == b][None, :, 1:4]
        boxes = gt[b:b + 1, :, :7]
        want = pr.points_in_boxes(boxes, pts)
        got = ops.points_in_boxes(dev(boxes), dev(pts))
        out = torch.full(want.shape, -7, dtype=torch.int32, device="cuda")
        assert shim.points_in_boxes_gpu(dev(boxes), dev(pts), out) == 1
        torch.cuda.synchronize()
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want) and torch.equal(out, got)
        assert (want >= 0).sum() >= 5 and (want < 0).sum() >= 5
    # two frames in one call: the boxes of frame b test the points of frame b only
    points, gt, _ = cases["main"]
    pts = np.stack([points[:213, 1:4], points[300:513, 1:4]])
    got = ops.points_in_boxes(dev(gt[:, :, :7]), dev(pts))
    assert np.array_equal(got.cpu().numpy(), pr.points_in_boxes(gt[:, :, :7], pts))
    with pytest.raises(RuntimeError, match="contiguous"):
        shim.points_in_boxes_gpu(dev(gt[:, :, :7]), dev(pts).transpose(1, 2).contiguous().transpose(1, 2), got)
    with pytest.raises(NotImplementedError, match="ground-truth rows per frame exceed"):
        ops.point_head_targets(dev(points), torch.zeros((2, ops.POINT_HEAD_MAX_GT + 1, 8), device="cuda"), pr.EXTRA, 3)


# ---------------------------------------------------------------------------------------------------------------- loss
def run_loss(preds, labels, wide=False):
    from dualfusion import ops
    if wide:                                                                    # a column block of a wider row buffer
        buf = torch.full((preds.shape[0], preds.shape[1] + 5), 1e30, device="cuda")
        buf[:, 2:2 + preds.shape[1]] = dev(preds)
        x = buf.requires_grad_(True)
        view = x[:, 2:2 + preds.shape[1]]
    else:
        x = dev(preds).requires_grad_(True)
        view = x
    loss, pos = ops.point_cls_loss(view, dev(labels), pr.LOSS_WEIGHT)
    assert tuple(loss.shape) == (1,) and tuple(pos.shape) == (1,) and loss.is_cuda and not pos.requires_grad
    (UPSTREAM * loss[0]).backward()
    grad = x.grad[:, 2:2 + preds.shape[1]] if wide else x.grad
    if wide:
        assert not x.grad[:, :2].any() and not x.grad[:, 2 + preds.shape[1]:].any()
    return loss.detach().clone(), pos.detach().clone(), grad.clone()


@pytest.mark.parametrize("name", pr.LOSS_CASES)
def test_loss_and_gradient_against_float64(name, g):
    from test_gpu_vrtail import judge
    preds, labels = pr.loss_case(name)
    want = pr.loss_and_grad(preds, labels, pr.LOSS_WEIGHT, torch.float64, UPSTREAM)
    loss, pos, grad = run_loss(preds, labels)
    again = run_loss(preds, labels)
    torch.cuda.synchronize()
    assert torch.equal(loss, again[0]) and torch.equal(pos, again[1]) and torch.equal(grad, again[2])      # bit-equal runs
    assert float(pos) == want[1] == float(g[name + "_pos_num"])
    if name == "all_ignored":
        assert float(loss) == 0.0 and not grad.any()                           # exactly
        return
    if name == "no_positive":
        assert float(pos) == 0.0 and float(loss) > 0                           # the normaliser clamps to 1
    # the yardstick: the reference's own float32 results (the fixture) against the float64 restatement
    judge("point_cls_loss " + name, [("loss", [want[0]], [float(g[name + "_loss"])], [float(loss)]),
                                     ("grad", want[2], g[name + "_grad"], grad.cpu().numpy())])
    wide = run_loss(preds, labels, wide=True)
    assert torch.equal(wide[0], loss) and torch.equal(wide[2], grad)


# ---------------------------------------------------------------------------------------------------------------- head
HEAD_ROWS, HEAD_CHANNELS = 513, 40


def head_batch(num_class, seed=4):
    """513 rows of 40 channels at the first 513 rows of the main case (frames 0 and 1)"""
    points, gt, _ = pr.target_case("main")
    rs = np.random.RandomState(seed)
    feats = rs.standard_normal((HEAD_ROWS, HEAD_CHANNELS)).astype(np.float32)
    return {"batch_size": 2, "point_features": dev(feats), "point_coords": dev(points[:HEAD_ROWS]), "gt_boxes": dev(gt)}, points[:HEAD_ROWS], gt


def run_point_head(head, num_class, mode, monkeypatch):
    """training-mode forward + get_loss().backward() -> labels, preds, the last layer's input, parameter gradients, loss, tb"""
    calls = (composed_only if mode == "0" else fused_only)(monkeypatch)
    hd = copy.deepcopy(head).cuda().train()
    seen = {}
    batch, _, _ = head_batch(num_class)
    feats = batch["point_features"]
    layers = list(hd.cls_layers)
    real = torch.nn.functional.linear

    def spy(x, w, b=None):
        if w is layers[-1].weight:
            seen["last"] = x.detach().double().cpu().numpy()
        return real(x, w, b)
    monkeypatch.setattr(torch.nn.functional, "linear", spy)
    out = hd(batch)
    monkeypatch.setattr(torch.nn.functional, "linear", real)
    r = hd.forward_ret_dict
    assert out is batch and tuple(batch["point_cls_scores"].shape) == (HEAD_ROWS,) and r["point_cls_preds"].requires_grad
    assert torch.equal(batch["point_cls_scores"], torch.sigmoid(r["point_cls_preds"]).max(dim=-1)[0])
    loss, tb = hd.get_loss()
    assert sorted(tb) == ["point_loss_cls", "point_pos_num"]
    assert all(isinstance(v, torch.Tensor) and v.is_cuda and not v.requires_grad for v in tb.values())
    loss.backward()
    torch.cuda.synchronize()
    assert calls is None or calls == ["point_head_targets", "point_cls_loss"]      # fused: one launch of each, no more
    grads = {k: p.grad.cpu().numpy() for k, p in hd.named_parameters()}
    assert all(np.abs(v).sum() > 0 for v in grads.values()), [k for k, v in grads.items() if not np.abs(v).sum() > 0]
    return (r["point_cls_labels"].cpu().numpy(), r["point_cls_preds"].detach().cpu().numpy(), seen["last"], grads, float(loss.detach()),
            {k: float(v) for k, v in tb.items()}, feats)


def float64_composition(preds, labels, last_in):
    """loss and the gradients of the last layer in float64, from the predictions the device made"""
    loss, pos, grad = pr.loss_and_grad(preds, labels, 1.0, torch.float64)
    return loss, pos, {"cls_layers.6.weight": grad.T @ last_in, "cls_layers.6.bias": grad.sum(0)}


@pytest.mark.parametrize("num_class", [1, 3])
def test_head_fused_and_composed(num_class, monkeypatch):
    """PointHeadSimple with CLS_FC [32, 32] on 513 rows of 40 channels.  The yardstick of
    test_gpu_roiloss.test_parameter_gradients_through_forward_train: the composed float32 path (torch autograd on the device)
    against the float64 composition on the predictions IT made; the fused mode against the float64 composition on its own, at
    most 4 x the yardstick."""
    from dualfusion import dense_heads
    torch.manual_seed(20 + num_class)
    head = dense_heads.PointHeadSimple(num_class=num_class, input_channels=HEAD_CHANNELS, model_cfg=pr.point_head_cfg(before_fusion=False))
    _, points, gt = head_batch(num_class)
    want_labels = pr.assign_targets(points, gt, pr.EXTRA, num_class)[0]
    composed = run_point_head(head, num_class, "0", monkeypatch)
    monkeypatch.undo()
    fused = run_point_head(head, num_class, "1", monkeypatch)
    assert np.array_equal(fused[0], composed[0]) and np.array_equal(fused[0], want_labels)               # identical labels
    assert sorted(np.unique(want_labels)) == ([-1, 0, 1] if num_class == 1 else [-1, 0, 1, 2, 3])
    failures = []
    c64, f64 = float64_composition(composed[1], composed[0], composed[2]), float64_composition(fused[1], fused[0], fused[2])
    for what, run, ref in (("composed", composed, c64), ("fused", fused, f64)):
        assert run[5]["point_pos_num"] == ref[1] == (want_labels > 0).sum(), what
        assert abs(run[5]["point_loss_cls"] - run[4]) == 0
    pairs = [("point_loss", pr.rel_err(composed[4], c64[0]), pr.rel_err(fused[4], f64[0]))]
    pairs += [(k, pr.rel_err(composed[3][k], c64[2][k]), pr.rel_err(fused[3][k], f64[2][k])) for k in sorted(f64[2])]
    for k, y, d in pairs:
        print("point head C=%d %-22s float32 yardstick (composed) %.3e  fused %.3e" % (num_class, k, y, d))
        if not d <= 4 * y:
            failures.append((k, y, d))
    assert not failures, failures
    # the layers in front see the same gradient up to float32 rounding of a sum over 513 rows
    for k in ("cls_layers.0.weight", "cls_layers.3.weight"):
        assert pr.rel_err(fused[3][k], composed[3][k]) <= 1e-4, k


def test_head_makes_no_host_synchronisation_in_fused_mode(monkeypatch):
    """forward + get_loss in fused mode under torch's synchronisation debug mode, after showing that the mode raises here"""
    from dualfusion import dense_heads
    fused_only(monkeypatch)
    torch.manual_seed(1)
    head = dense_heads.PointHeadSimple(num_class=3, input_channels=HEAD_CHANNELS, model_cfg=pr.point_head_cfg(before_fusion=False)).cuda().train()
    batch, _, _ = head_batch(3)
    head(dict(batch))                                                           # warm-up: allocations, the first launches
    head.get_loss()[0].backward()
    torch.cuda.synchronize()
    probe = torch.ones((1,), device="cuda")
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.item()                                                        # the mode is honoured by this build
        out = head(dict(batch))
        loss, tb = head.get_loss()
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(torch.isfinite(loss)) and float(tb["point_pos_num"]) > 0 and "point_cls_scores" in out


# ---------------------------------------------------------------------------------------------------------------- detector
@pytest.fixture(scope="module")
def sweeps():
    from dualfusion import ops, synth
    clouds = [synth.kitti_sweep(seed=40 + b)[:, :4].copy() for b in range(2)]
    points = [torch.from_numpy(c).cuda() for c in clouds]
    feats, coords = ops.hard_voxelize_clouds(points, synth.KITTI_VOXEL, synth.KITTI_RANGE, 5, 40000, resident_inputs=False)
    stacked = torch.cat([torch.cat([torch.full((len(p), 1), float(b), device="cuda"), p], dim=1) for b, p in enumerate(points)])
    # ground truth: car-sized boxes centred on points of the sweep, and one zero row of padding
    gt = np.zeros((2, 5, 8), np.float32)
    for b, c in enumerate(clouds):
        rs = np.random.RandomState(b)
        inside = c[(c[:, 0] > 5) & (c[:, 0] < 60) & (np.abs(c[:, 1]) < 30)]
        pick = inside[rs.choice(len(inside), 4, replace=False)]
        gt[b, :4] = np.concatenate([pick[:, :3], np.tile([3.9, 1.6, 1.56], (4, 1)), rs.uniform(-1, 1, (4, 1)), np.ones((4, 1))], axis=1)
    return feats, coords, stacked.contiguous(), dev(gt)


def build_detector():
    from dualfusion import synth, vr_detector
    torch.manual_seed(5)
    return vr_detector.PVRCNN(pr.pv_rcnn_cfg(), 1, ["Car"], np.array([1408, 1600, 40]), synth.KITTI_RANGE, synth.KITTI_VOXEL).cuda()


def test_detector_eval_returns_boxes_and_keypoint_scores(sweeps):
    feats, coords, points, _ = sweeps
    model = build_detector().eval()
    batch = {"voxel_features": feats, "voxel_coords": coords, "points": points, "batch_size": 2}
    with torch.no_grad():
        pred_dicts, recall = model(batch)
        direct = model.point_head({"point_features_before_fusion": batch["point_features_before_fusion"],
                                   "point_features": batch["point_features"]})["point_cls_scores"]
    assert recall == {} and len(pred_dicts) == 2
    for p in pred_dicts:
        boxes, scores, labels = p["pred_boxes"], p["pred_scores"], p["pred_labels"]
        n = scores.shape[0]
        assert 0 < n <= 100 and tuple(boxes.shape) == (n, 7) and labels.shape[0] == n
        assert bool(torch.isfinite(boxes).all()) and bool(torch.isfinite(scores).all())
        assert bool((scores[1:] <= scores[:-1]).all()) and bool((labels == 1).all())
    scores = batch["point_cls_scores"]
    assert tuple(scores.shape) == (2 * 256,) and torch.equal(scores, direct) and bool(((scores > 0) & (scores < 1)).all())
    assert tuple(batch["point_coords"].shape) == (512, 4)


def test_detector_training_step(sweeps, monkeypatch):
    feats, coords, points, gt = sweeps
    model = build_detector().train()
    batch = {"voxel_features": feats, "voxel_coords": coords, "points": points, "batch_size": 2, "gt_boxes": gt}
    ret, tb, disp = model(batch)
    loss = ret["loss"]
    assert sorted(ret) == ["loss"] and disp == {} and loss.requires_grad and bool(torch.isfinite(loss))
    for k in ("rpn_loss", "rpn_loss_cls", "rpn_loss_loc", "rpn_loss_dir", "point_loss_cls", "point_pos_num", "rcnn_loss", "rcnn_loss_cls",
              "rcnn_loss_reg", "rcnn_loss_corner"):
        assert k in tb and isinstance(tb[k], torch.Tensor) and not tb[k].requires_grad, k
    parts = float(tb["rpn_loss"]) + float(tb["point_loss_cls"]) + float(tb["rcnn_loss"])
    print("PVRCNN training step: loss %.6f = rpn %.6f + point %.6f + rcnn %.6f, point_pos_num %d"
          % (float(loss.detach()), float(tb["rpn_loss"]), float(tb["point_loss_cls"]), float(tb["rcnn_loss"]), int(tb["point_pos_num"])))
    assert abs(float(loss.detach()) - parts) <= 4 * 2.0 ** -24 * abs(parts)              # two float32 additions
    assert float(tb["point_pos_num"]) > 0                                       # keypoints inside the ground-truth boxes
    labels = model.point_head.forward_ret_dict["point_cls_labels"]
    keypoints = batch["point_coords"].cpu().numpy()
    want = pr.assign_targets(keypoints, gt.cpu().numpy(), pr.EXTRA, 1)[0]
    # (keypoints are not margin-cleaned: only a pair near a face may differ)
    assert (labels.cpu().numpy() != want).sum() <= pr.near_face(keypoints, gt.cpu().numpy(), pr.EXTRA)
    # the RoIs come from the DETACHED first-stage predictions: no gradient path from them into the dense head
    assert not batch["dense_cls_rows"].requires_grad and not batch["dense_box_rows"].requires_grad
    assert not batch["rois"].requires_grad and tuple(batch["rois"].shape) == (2, 16, 7)
    rcnn_loss = model.roi_head.get_loss()[0]
    head_params = [model.dense_head.conv_cls.weight, model.dense_head.conv_box.weight]
    assert all(v is None for v in torch.autograd.grad(rcnn_loss, head_params, retain_graph=True, allow_unused=True))
    # the point loss alone reaches the VSA's set-abstraction weights: through the point head's input
    sa_weights = [p for n, p in model.pfe.SA_layers.named_parameters() if p.dim() > 1]
    point_loss = model.point_head.get_loss()[0]
    reached = torch.autograd.grad(point_loss, sa_weights, retain_graph=True, allow_unused=True)
    assert sa_weights and all(v is not None and bool(v.abs().sum() > 0) for v in reached)
    loss.backward()
    torch.cuda.synchronize()
    for name, p in model.point_head.named_parameters():
        assert p.grad is not None and bool(p.grad.abs().sum() > 0) and bool(torch.isfinite(p.grad).all()), name
    for p in sa_weights:
        assert p.grad is not None and bool(p.grad.abs().sum() > 0)
    assert bool(model.dense_head.conv_cls.weight.grad.abs().sum() > 0) and bool(model.roi_head.cls_layers[-1].weight.grad.abs().sum() > 0)
    # DETECTOR-level refusal that stays: the shipped TRAIN proposals are past the candidate cap
    import stacksa_reference as sr
    model.roi_head.model_cfg = dict(model.roi_head.model_cfg, NMS_CONFIG=sr.SHIPPED_HEAD["NMS_CONFIG"])
    with pytest.raises(NotImplementedError, match="NMS_PRE_MAXSIZE = 9000 exceeds 4096"):
        model({"voxel_features": feats, "voxel_coords": coords, "points": points, "batch_size": 2, "gt_boxes": gt})
