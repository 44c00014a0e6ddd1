"""Anchor target assignment and the RPN losses on the device (csrc/anchorloss.hip, dualfusion/ops.py, dense_heads.py) against
the reference's results (tests/golden/anchor_loss.npz) and the float64 restatement (tests/anchorloss_reference.py).

Labels, ids and counts are compared exactly: the fixture's margins (no anchor-max IoU within 1e-4 of a threshold, best and
second-best IoU 1e-6 apart where the order decides, direction-bin quotient 1e-3 from an integer, no |diff| within 1e-4 of
beta) make a mismatch a bug and not rounding.  Values are judged by the project's yardstick (tests/test_gpu_vrtail.judge):
per tensor, the reference's float32 result against the float64 restatement gives max error over max magnitude; the device
may deviate from the restatement at most 4 x that.  Both numbers are printed."""
import copy

import numpy as np
import pytest

import anchorloss_reference as al
import vrtail_reference as vt
from test_gpu_vrtail import dev, judge

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g(golden):
    return golden("anchor_loss.npz")


@pytest.fixture(scope="module")
def restated(g):
    """computed once, shared, never modified"""
    return {name: al.restate(name, g) for name in vt.CASES}


def tables(name):
    from dualfusion import dense_heads
    grid, rng = vt.case_geometry(name)
    return dense_heads.AnchorTables(vt.CASES[name]["sets"], grid, rng)


def run_assign(name, gt, dense=True):
    from dualfusion import ops
    t = tables(name)
    x_shifts, y_shifts = t.on("cuda")
    sc, matched, unmatched = al.set_params(name)
    out = ops.anchor_assign(x_shifts, y_shifts, dev(gt), t.H, t.W, t.anchor_set, t.table.tolist(), sc, matched, unmatched, dense=dense)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


@pytest.mark.parametrize("name", ["small", "car", "multi"])
def test_assignment_on_the_golden_ground_truth(g, restated, name):
    a = restated[name][0]
    labels, gt_ids, num_pos, targets, weights = run_assign(name, g[name + "_gt"])
    n = vt.CASES[name]["H"] * vt.CASES[name]["W"] * 2 * len(vt.CASES[name]["sets"])
    assert labels.dtype == np.int32 and gt_ids.dtype == np.int32 and num_pos.dtype == np.int32
    assert labels.shape == (vt.CASES[name]["B"], n) and targets.shape == labels.shape + (7,) and targets.dtype == np.float32
    assert np.array_equal(labels, g[name + "_labels"]) and np.array_equal(labels, a["labels"])
    assert np.array_equal(gt_ids, a["gt_ids"])
    assert np.array_equal(num_pos, a["num_pos"]) and np.array_equal(num_pos, (g[name + "_labels"] > 0).sum(1))
    assert np.array_equal(weights, g[name + "_weights"])
    assert not targets[labels <= 0].any()
    judge("assign " + name, [("box_reg_targets", a["targets"], g[name + "_targets"], targets)])
    lean = run_assign(name, g[name + "_gt"], dense=False)
    assert len(lean) == 3 and all(np.array_equal(x, y) for x, y in zip(lean, (labels, gt_ids, num_pos)))


def test_assignment_with_one_ground_truth_more_than_an_lds_chunk():
    """129 boxes in one frame: the last one goes through a second chunk; exact against the restatement (the seed is searched
    on the host until the margins hold and the last box is some anchor's target)."""
    from dualfusion import ops
    M = ops.ANCHOR_GT_CHUNK + 1
    t = tables("car")
    anchors = t.dense().numpy().reshape(-1, 7)
    _, rng = vt.case_geometry("car")
    sc, matched, unmatched = al.set_params("car")
    for seed in range(64):
        rs = np.random.RandomState(500 + seed)
        gt = np.zeros((2, M, 8), np.float32)
        size = np.asarray(vt.CAR["anchor_sizes"][0]) * rs.uniform(0.8, 1.25, (M, 3))
        gt[0, :, 0], gt[0, :, 1] = rs.uniform(rng[0], rng[3], M), rs.uniform(rng[1], rng[4], M)
        gt[0, :, 2], gt[0, :, 3:6], gt[0, :, 6], gt[0, :, 7] = -1.0, size, rs.uniform(-np.pi, np.pi, M), 1
        gt[1, :5] = gt[0, :5]                                               # a second frame that stops within the first chunk
        a = al.assign(anchors, al.anchor_sets("car"), 2, gt, sc, matched, unmatched)
        if al.assign_clean(a) and (a["gt_ids"][0] == M - 1).any():
            break
    else:
        raise AssertionError("no clean seed")
    labels, gt_ids, num_pos, targets, weights = run_assign("car", gt)
    assert np.array_equal(labels, a["labels"]) and np.array_equal(gt_ids, a["gt_ids"]) and np.array_equal(num_pos, a["num_pos"])
    assert gt_ids.max() == M - 1 and len(np.unique(gt_ids[0])) > 20
    assert np.abs(targets - a["targets"]).max() <= 8 * vt.U32 * np.abs(a["targets"]).max()


def loss_spec(name, g, labels, gt_ids, num_pos, pad=0):
    """-> AnchorLossSpec, the wide row buffer [rows, width] (pad > 0: 1e30 between and around the three blocks), blocks"""
    from dualfusion import ops
    c, src = vt.CASES[name], al.source(name)
    t = tables(name)
    rows = c["B"] * c["H"] * c["W"]
    maps = [g[src + "_cls"].reshape(rows, -1), g[src + "_box"].reshape(rows, -1)] + ([g[src + "_dir"].reshape(rows, -1)] if c["NB"] else [])
    wide = torch.full((rows, sum(m.shape[1] for m in maps) + (len(maps) + 1) * pad), 1e30, device="cuda")
    cols, col = [], pad
    for m in maps:
        wide[:, col:col + m.shape[1]] = dev(m)
        cols.append(col)
        col += m.shape[1] + pad
    blocks = [(c0, c0 + m.shape[1]) for c0, m in zip(cols, maps)]
    if not c["NB"]:
        cols.append(None)
    x_shifts, y_shifts = t.on("cuda")
    w = al.LOSS_WEIGHTS
    spec = ops.AnchorLossSpec(cols, x_shifts, y_shifts, dev(labels), dev(gt_ids), dev(num_pos), dev(g[src + "_gt"]), c["H"], c["W"], c["C"],
                              c["NB"], t.anchor_set, t.table.tolist(), w["cls_weight"], w["loc_weight"], w["dir_weight"],
                              w["code_weights"], dir_offset=vt.DIR_OFFSET)
    return spec, wide, blocks


def run_loss(name, g, a, pad=0, upstream=(1.0, 1.0, 1.0)):
    """ops.anchor_loss + backward on the golden maps -> losses [3], [grad_cls, grad_box(, grad_dir)] as [B, N, channels]"""
    from dualfusion import ops
    c = vt.CASES[name]
    spec, wide, blocks = loss_spec(name, g, g[name + "_labels"], a["gt_ids"], a["num_pos"], pad)
    wide.requires_grad_(True)
    losses = ops.anchor_loss(wide, spec)
    (losses * torch.tensor(upstream, device="cuda")).sum().backward()
    torch.cuda.synchronize()
    grad = wide.grad.cpu().numpy()
    outside = np.ones(grad.shape[1], bool)
    for lo, hi in blocks:
        outside[lo:hi] = False
    assert not grad[:, outside].any()
    return losses.detach().cpu().numpy(), [grad[:, lo:hi].reshape(c["B"], a["labels"].shape[1], -1) for lo, hi in blocks]


def loss_pairs(name, g, l, losses, grads, scale=1.0):
    keys = ["grad_cls", "grad_box"] + (["grad_dir"] if vt.CASES[name]["NB"] else [])
    return [("losses", l["loss"], g[name + "_loss"], losses)] + \
        [(k, l[k], g[name + "_" + k].astype(np.float64) * scale, got) for k, got in zip(keys, grads)]


@pytest.mark.parametrize("name", ["small", "car", "multi", "nodir"])
def test_losses_and_map_gradients_on_the_golden_maps(g, restated, name):
    a, l = restated[name]
    losses, grads = run_loss(name, g, a)
    assert losses.dtype == np.float32 and losses.shape == (3,) and len(grads) == (3 if vt.CASES[name]["NB"] else 2)
    if not vt.CASES[name]["NB"]:
        assert losses[2] == 0
    assert not grads[0][g[name + "_labels"] < 0].any()                        # zeros exactly where nothing contributes
    for got in grads[1:]:
        assert not got[g[name + "_labels"] <= 0].any() and got[g[name + "_labels"] > 0].any()
    judge("loss " + name, loss_pairs(name, g, l, losses, grads))


def test_rows_as_column_blocks_of_a_wider_buffer(g, restated):
    from dualfusion import ops
    a, l = restated["car"]
    plain, plain_grads = run_loss("car", g, a)
    padded, padded_grads = run_loss("car", g, a, pad=5)
    assert np.array_equal(plain, padded) and all(np.array_equal(x, y) for x, y in zip(plain_grads, padded_grads))
    # the gradient entry point writes the blocks of a caller's buffer and nothing else
    spec, wide, blocks = loss_spec("car", g, g["car_labels"], a["gt_ids"], a["num_pos"], pad=5)
    assert wide.stride(0) > sum(hi - lo for lo, hi in blocks)
    into = torch.full_like(wide, 1e30)
    ops.anchor_loss_grad_into(wide, spec, torch.ones(3, device="cuda"), into)
    torch.cuda.synchronize()
    into = into.cpu().numpy()
    outside = np.ones(into.shape[1], bool)
    for (lo, hi), want in zip(blocks, plain_grads):
        outside[lo:hi] = False
        assert np.array_equal(into[:, lo:hi].reshape(want.shape), want)
    assert (into[:, outside] == np.float32(1e30)).all()


def test_upstream_gradients_are_honoured(g, restated):
    a, _ = restated["car"]
    _, one = run_loss("car", g, a)
    _, three = run_loss("car", g, a, upstream=(3.0, 3.0, 3.0))
    for x, y in zip(one, three):
        assert np.abs(y - 3.0 * x.astype(np.float64)).max() <= 2 * vt.U32 * np.abs(y).max()
    up = (0.5, 2.0, -3.0)
    c, src = vt.CASES["car"], "car"
    l = al.losses(g["car_cls"], g["car_box"], g["car_dir"], g["car_anchors"].reshape(-1, 7), a["labels"], a["targets"], c["C"], upstream=up)
    _, mixed = run_loss("car", g, a, upstream=up)
    judge("upstream car", [(k, l[k], g["car_" + k].astype(np.float64) * s, got)
                           for k, s, got in zip(("grad_cls", "grad_box", "grad_dir"), up, mixed)])


# ---------------------------------------------------------------------------------------------------- modules
MOD_C = 16


def build_head(name, seed):
    from dualfusion import dense_heads
    torch.manual_seed(seed)
    c = vt.CASES[name]
    grid, rng = vt.case_geometry(name)
    head = dense_heads.AnchorHeadSingle(copy.deepcopy(al.train_head_cfg(name)), MOD_C, c["C"], al.TRAIN[name]["class_names"], grid, rng).train()
    with torch.no_grad():
        head.conv_cls.weight.normal_(0, 2 / np.sqrt(MOD_C))
        head.conv_cls.bias.zero_()
        head.conv_box.weight.normal_(0, 0.3 / np.sqrt(MOD_C))
        if head.conv_dir_cls is not None:
            head.conv_dir_cls.weight.normal_(0, 1 / np.sqrt(MOD_C))
    return head, torch.randn(c["B"], MOD_C, c["H"], c["W"])


def head_on_cpu(head, x, gt, monkeypatch):
    """the float32 yardstick: the composed formulation on the CPU -> maps [B, N, .] and parameter gradients"""
    monkeypatch.setenv("DF3D_ANCHOR_LOSS_FUSED", "0")
    h = copy.deepcopy(head)
    h.forward_train({"spatial_features_2d": x, "gt_boxes": torch.from_numpy(gt)})
    loss, _ = h.get_loss()
    loss.backward()
    r = h.forward_ret_dict
    B = x.shape[0]
    maps = [r[k].detach().reshape(B, r["box_cls_labels"].shape[1], -1).numpy() for k in ("cls_preds", "box_preds", "dir_cls_preds") if k in r]
    return maps, {k: p.grad.numpy() for k, p in h.named_parameters()}, float(loss.detach())


def float64_parameter_gradients(name, head, x, gt, maps):
    c = vt.CASES[name]
    anchors = head.anchors.numpy().reshape(-1, 7)
    sc, matched, unmatched = al.set_params(name)
    a = al.assign(anchors, al.anchor_sets(name), head.num_anchors_per_location, gt, sc, matched, unmatched)
    l = al.losses(maps[0], maps[1], maps[2] if len(maps) > 2 else None, anchors, a["labels"], a["targets"], c["C"])
    X = x.permute(0, 2, 3, 1).reshape(-1, MOD_C).numpy().astype(np.float64)
    want = {}
    for conv, k in (("conv_cls", "grad_cls"), ("conv_box", "grad_box"), ("conv_dir_cls", "grad_dir")):
        if l[k] is not None:
            G = l[k].reshape(X.shape[0], -1)
            want[conv + ".weight"] = (G.T @ X).reshape(-1, MOD_C, 1, 1)
            want[conv + ".bias"] = G.sum(0)
    return a, l, want


def clean_head(name, g, monkeypatch):
    """first seed whose module-made maps keep the margins of the losses"""
    gt = g[al.source(name) + "_gt"]
    for seed in range(32):
        head, x = build_head(name, seed)
        maps, yard, yard_loss = head_on_cpu(head, x, gt, monkeypatch)
        a, l, want = float64_parameter_gradients(name, head, x, gt, maps)
        if al.loss_clean(l, vt.CASES[name]["NB"] > 0):
            return head, x, gt, a, l, want, yard
    raise AssertionError("no clean seed")


@pytest.mark.parametrize("name", ["car", "multi"])
def test_parameter_gradients_through_forward_train(g, monkeypatch, name):
    """conv_cls / conv_box / conv_dir_cls gradients of forward_train + get_loss().backward(), fused and composed.  The
    yardstick: the float32 composition on the CPU against the float64 composition on ITS maps; the device against the
    float64 composition on the maps the device made (its 1x1 convolution rounds differently), at most 4 x the yardstick."""
    head, x, gt, a, l_cpu, want_cpu, yard = clean_head(name, g, monkeypatch)
    c = vt.CASES[name]
    failures = []
    for mode in ("1", "0"):
        monkeypatch.setenv("DF3D_ANCHOR_LOSS_FUSED", mode)
        hd = copy.deepcopy(head).cuda()
        data = {"spatial_features_2d": x.cuda(), "gt_boxes": dev(gt), "batch_size": c["B"]}
        out = hd.forward_train(data)
        assert out is data and "rois" not in out
        r = hd.forward_ret_dict
        assert tuple(r["cls_preds"].shape) == (c["B"], c["H"], c["W"], hd.conv_cls.out_channels) and r["cls_preds"].requires_grad
        assert tuple(r["box_preds"].shape) == (c["B"], c["H"], c["W"], hd.conv_box.out_channels)
        assert tuple(r["dir_cls_preds"].shape) == (c["B"], c["H"], c["W"], hd.conv_dir_cls.out_channels)
        assert r["box_cls_labels"].dtype == torch.int32 and ("box_reg_targets" in r) == (mode == "0")
        loss, tb = hd.get_loss()
        assert sorted(tb) == ["rpn_loss", "rpn_loss_cls", "rpn_loss_dir", "rpn_loss_loc"]
        assert all(isinstance(v, torch.Tensor) and v.is_cuda and not v.requires_grad for v in tb.values())
        loss.backward()
        torch.cuda.synchronize()
        assert np.array_equal(r["box_cls_labels"].cpu().numpy(), a["labels"]), mode
        assert np.array_equal(r["gt_ids"].cpu().numpy(), a["gt_ids"]) and np.array_equal(r["num_pos"].cpu().numpy(), a["num_pos"])
        maps = [r[k].detach().reshape(c["B"], a["labels"].shape[1], -1).cpu().numpy() for k in ("cls_preds", "box_preds", "dir_cls_preds")]
        _, l, want = float64_parameter_gradients(name, head, x, gt, maps)
        assert al.loss_clean(l, True)                                       # the margins hold on the device's maps too
        grads = {k: p.grad.cpu().numpy() for k, p in hd.named_parameters()}
        assert sorted(grads) == sorted(want)
        parts = np.array([float(tb[k]) for k in ("rpn_loss_cls", "rpn_loss_loc", "rpn_loss_dir")])
        # float32 results of float32 sums over [B, N, C] terms in the composed mode: 64 roundings of the largest
        assert np.abs(parts - l["loss"]).max() <= 64 * vt.U32 * np.abs(l["loss"]).max()
        assert abs(float(loss.detach()) - l["loss"].sum()) <= 64 * vt.U32 * l["loss"].sum()
        for k in sorted(want):
            y, d = vt.rel_err(yard[k], want_cpu[k]), vt.rel_err(grads[k], want[k])
            print("%s %s %-22s float32 yardstick %.3e  device %.3e" % ("fused" if mode == "1" else "composed", name, k, y, d))
            if not d <= 4 * y:
                failures.append((mode, k, y, d))
    assert not failures, failures


@pytest.mark.parametrize("name", ["car", "multi", "nodir"])
def test_fused_and_composed_agree(g, restated, monkeypatch, name):
    """the composed path on the device as a second implementation: labels exactly, losses and map gradients by the yardstick"""
    from dualfusion import dense_heads
    a, l = restated[name]
    c, src = vt.CASES[name], al.source(name)
    fused_losses, fused_grads = run_loss(name, g, a)
    monkeypatch.setenv("DF3D_ANCHOR_LOSS_FUSED", "0")
    grid, rng = vt.case_geometry(name)
    head = dense_heads.AnchorHeadSingle(al.train_head_cfg(name), MOD_C, c["C"], al.TRAIN[name]["class_names"], grid, rng).cuda().train()
    t = head.assign_targets(dev(g[src + "_gt"]))
    fused_labels = run_assign(name, g[src + "_gt"], dense=False)
    assert np.array_equal(t["box_cls_labels"].cpu().numpy(), fused_labels[0])
    assert np.array_equal(t["gt_ids"].cpu().numpy(), fused_labels[1]) and np.array_equal(t["num_pos"].cpu().numpy(), fused_labels[2])
    view = lambda v: dev(v).view(c["B"], c["H"], c["W"], -1).requires_grad_(True)
    ret = {"cls_preds": view(g[src + "_cls"]), "box_preds": view(g[src + "_box"])}
    if c["NB"]:
        ret["dir_cls_preds"] = view(g[src + "_dir"])
    ret.update(t)
    head.forward_ret_dict = ret
    loss, tb = head.get_loss()
    loss.backward()
    composed = np.array([float(tb["rpn_loss_cls"]), float(tb["rpn_loss_loc"]), float(tb.get("rpn_loss_dir", torch.zeros(())))], np.float32)
    grads = [ret[k].grad.reshape(x.shape).cpu().numpy() for k, x in zip(("cls_preds", "box_preds", "dir_cls_preds"), fused_grads)]
    judge("composed " + name, loss_pairs(name, g, l, composed, grads))
    judge("fused " + name, loss_pairs(name, g, l, fused_losses, fused_grads))


def test_assign_loss_and_backward_make_the_host_wait_for_nothing(g, restated):
    """Under torch's synchronisation debug mode any read of a device value by the host raises."""
    from dualfusion import ops
    a, _ = restated["car"]
    t = tables("car")
    x_shifts, y_shifts = t.on("cuda")
    table = t.table.tolist()
    sc, matched, unmatched = al.set_params("car")
    gt = dev(g["car_gt"])
    c = vt.CASES["car"]
    rows = c["B"] * c["H"] * c["W"]
    wide = torch.cat([dev(g["car_" + k].reshape(rows, -1)) for k in ("cls", "box", "dir")], dim=1).requires_grad_(True)
    up = torch.tensor([3.0, 3.0, 3.0], device="cuda")
    w = al.LOSS_WEIGHTS
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        labels, gt_ids, num_pos = ops.anchor_assign(x_shifts, y_shifts, gt, t.H, t.W, t.anchor_set, table, sc, matched, unmatched)
        spec = ops.AnchorLossSpec((0, 2, 16), x_shifts, y_shifts, labels, gt_ids, num_pos, gt, t.H, t.W, 1, 2, t.anchor_set, table,
                                  w["cls_weight"], w["loc_weight"], w["dir_weight"], w["code_weights"], dir_offset=vt.DIR_OFFSET)
        losses = ops.anchor_loss(wide, spec)
        (losses * up).sum().backward()
        with pytest.raises(RuntimeError, match="synchroniz"):
            num_pos.tolist()                                                # the mode does see a read
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert np.array_equal(num_pos.cpu().numpy(), a["num_pos"]) and np.array_equal(labels.cpu().numpy(), g["car_labels"])
    _, three = run_loss("car", g, a, upstream=(3.0, 3.0, 3.0))
    grad = wide.grad.cpu().numpy()
    assert np.array_equal(grad[:, :2].reshape(three[0].shape), three[0]) and np.array_equal(grad[:, 2:16].reshape(three[1].shape), three[1])


def test_results_are_bit_identical_from_run_to_run(g, restated):
    a, _ = restated["car"]
    first, second = run_assign("car", g["car_gt"]), run_assign("car", g["car_gt"])
    for x, y in zip(first, second):
        assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
    l1, g1 = run_loss("car", g, a)
    l2, g2 = run_loss("car", g, a)
    assert np.array_equal(l1.view(np.uint32), l2.view(np.uint32))
    for x, y in zip(g1, g2):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
