"""The Voxel-RCNN tail on the device (csrc/proposals.hip, dualfusion/dense_heads.py, roi_heads.py, vr_detector.py) against
the reference's results (tests/golden/vr_tail.npz) and the float64 restatement (tests/vrtail_reference.py).

Indices, counts, labels and padding are compared exactly: the fixture's margins (distinct scores, floor distance >= 1e-3, no
IoU within 1e-4 of a threshold) make a mismatch a bug and not rounding.  Values are judged by the project's yardstick
(tests/test_gpu_roipool.py): per tensor, the reference's float32 composition on the CPU against the float64 restatement gives
max error over max magnitude; the device may deviate from the restatement at most 4 x that.  Both numbers are printed."""
import copy

import numpy as np
import pytest

import vrtail_reference as vt

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def g(golden):
    return golden("vr_tail.npz")


def judge(what, pairs):
    """pairs: (name, float64 reference, float32 yardstick, device); device error <= 4 x yardstick error, per tensor"""
    failures = []
    for name, want, yard, got in pairs:
        y, d = vt.rel_err(yard, want), vt.rel_err(got, want)
        print("%s %-28s float32 yardstick %.3e  device %.3e" % (what, name, y, d))
        if not d <= 4 * y:
            failures.append((name, y, d))
    assert not failures, failures


def tables(name, g):
    """what AnchorHeadSingle hands the op: shift tables, anchor sets and the per-anchor table of a case"""
    from dualfusion import dense_heads
    grid, rng = vt.case_geometry(name)
    t = dense_heads.AnchorTables(vt.CASES[name]["sets"], grid, rng)
    assert np.array_equal(t.dense().numpy(), g[("car" if name == "nodir" else name) + "_anchors"])
    return t


def run_proposals(name, g, pad=0):
    """the op on the golden maps of a case; pad > 0: the maps are column blocks of one wider row buffer"""
    from dualfusion import ops
    c = vt.CASES[name]
    src = "car" if name == "nodir" else name
    t = tables(name, g)
    rows = c["B"] * c["H"] * c["W"]
    maps = [g[src + "_cls"].reshape(rows, -1), g[src + "_box"].reshape(rows, -1), g[src + "_dir"].reshape(rows, -1)]
    if pad:
        wide = torch.full((rows, sum(m.shape[1] for m in maps) + 3 * pad), 1e30, device="cuda")
        views, col = [], pad
        for m in maps:
            wide[:, col:col + m.shape[1]] = dev(m)
            views.append(wide[:, col:col + m.shape[1]])
            col += m.shape[1] + pad
        assert views[0].stride(0) > views[0].shape[1]
    else:
        views = [dev(m) for m in maps]
    x_shifts, y_shifts = t.on("cuda")
    out = ops.anchor_proposals(views[0], views[1], views[2] if c["NB"] else None, x_shifts, y_shifts, c["B"], c["H"], c["W"], c["C"],
                               t.anchor_set, t.table.tolist(), c["thresh"], c["pre"], c["post"], dir_offset=vt.DIR_OFFSET,
                               dir_limit_offset=vt.DIR_LIMIT_OFFSET)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def restated(name, g):
    c = vt.CASES[name]
    src = "car" if name == "nodir" else name
    return vt.proposals(g[src + "_cls"], g[src + "_box"], g[src + "_dir"] if c["NB"] else None, g[src + "_anchors"].reshape(-1, 7),
                        c["pre"], c["post"], c["thresh"], vt.DIR_OFFSET, vt.DIR_LIMIT_OFFSET)


def match_rows(got, table):
    """index of the row of `table` [n, 7] closest to each row of got [m, 7], and that distance"""
    d = np.abs(got[:, None, :].astype(np.float64) - table[None].astype(np.float64)).max(-1)
    return d.argmin(1), d.min(1)


def check_proposals(name, g, out):
    c = vt.CASES[name]
    src = "car" if name == "nodir" else name
    rois, scores, labels, num = out
    ref = restated(name, g)
    assert rois.shape == (c["B"], c["post"], 7) and labels.dtype == np.int64 and num.dtype == np.int32
    assert np.array_equal(num, ref["num"]) and np.array_equal(num, (ref["index"] >= 0).sum(1))
    cls_max = g[src + "_cls"].max(-1)
    for b in range(c["B"]):
        n = num[b]
        idx, dist = match_rows(rois[b, :n], g[name + "_dense"][b])          # recovered from the boxes themselves
        assert dist.max() <= 1e-4, dist.max()
        assert np.array_equal(idx, ref["index"][b, :n]), (name, b)
        assert np.array_equal(scores[b, :n].view(np.uint32), cls_max[b][idx].view(np.uint32))       # the raw logits, bit for bit
        assert np.array_equal(rois[b, n:], np.zeros((c["post"] - n, 7), np.float32))
        assert np.array_equal(scores[b, n:].view(np.uint32), np.zeros((c["post"] - n,), np.uint32))
        assert (labels[b, n:] == 1).all()
    assert np.array_equal(labels, g[name + "_roi_labels"]) and np.array_equal(scores, g[name + "_roi_scores"])
    judge("proposals " + name, [("rois", ref["rois"], g[name + "_rois"], rois)])


@pytest.mark.parametrize("name", ["car", "small", "multi", "nodir"])
def test_proposals_on_the_golden_maps(g, name):
    check_proposals(name, g, run_proposals(name, g))


def test_proposals_with_leading_dimensions_larger_than_the_rows(g):
    out = run_proposals("car", g, pad=5)
    check_proposals("car", g, out)
    for a, b in zip(out, run_proposals("car", g)):
        assert np.array_equal(a, b)


def test_proposals_order_by_the_raw_logits_and_ties_by_index():
    """Logits above +20 and below -20 whose float32 sigmoids coincide (1 and 0): the order follows the logits; exact ties go
    to the lower anchor index; -0.0 ties with +0.0."""
    from dualfusion import dense_heads, ops
    H, W = 5, 4
    grid, rng = np.array([W * 8, H * 8, 40]), vt._range(W, H)
    far = dict(vt.CAR, anchor_sizes=[[0.2, 0.1, 1.0]])                       # boxes too small to overlap at a 0.4 m pitch
    t = dense_heads.AnchorTables([far], grid, rng)
    cls = np.full((H * W * 2,), -50.0, np.float32)
    order = [(17, 30.0), (3, 25.000002), (9, 25.0), (5, 21.0), (6, 21.0), (33, 21.0), (12, 0.0), (20, -0.0), (8, -21.0),
             (1, -21.000002), (30, -30.0), (2, -30.0)]
    for i, v in order:
        cls[i] = v
    s = 1 / (1 + np.exp(-cls.astype(np.float64)))
    assert np.float32(s[17]) == np.float32(s[3]) == np.float32(s[5]) == 1 and cls[3] != cls[9] and cls[8] != cls[1]
    want = [17, 3, 9, 5, 6, 33, 12, 20, 8, 1, 2, 30]
    x_shifts, y_shifts = t.on("cuda")
    rois, scores, labels, num = ops.anchor_proposals(dev(cls.reshape(H * W, 2)), torch.zeros(H * W, 14, device="cuda"), None, x_shifts,
                                                     y_shifts, 1, H, W, 1, t.anchor_set, t.table.tolist(), 0.7, 12, 12)
    anchors = t.dense().numpy().reshape(-1, 7)
    assert int(num[0]) == 12
    idx, dist = match_rows(rois[0].cpu().numpy(), anchors)
    assert dist.max() <= 1e-5 and list(idx) == want
    assert np.array_equal(scores[0].cpu().numpy().view(np.uint32), cls[want].view(np.uint32))


def run_final(name, g, raw):
    from dualfusion import ops
    labels = dev(g[name + "_roi_labels"]) if vt.CASES[name]["C"] > 1 else None
    out = ops.roi_decode_select(dev(g[name + "_rois"]), dev(g[name + "_rcnn_cls"]), dev(g[name + "_rcnn_reg"]), labels,
                                vt.FINAL["score_thresh"], vt.FINAL["thresh"], vt.FINAL["pre"], vt.FINAL["post"], output_raw_score=raw)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def check_final(name, g, raw, out, what="final"):
    box_preds, boxes, scores, labels, counts = out
    tag = name + ("_raw" if raw else "")
    B, post = len(counts), vt.FINAL["post"]
    want_boxes = vt.roi_decode(g[name + "_rois"], g[name + "_rcnn_reg"])
    fin = vt.final_select(want_boxes, g[name + "_rcnn_cls"], g[name + "_roi_labels"] if vt.CASES[name]["C"] > 1 else None,
                          vt.FINAL["score_thresh"], vt.FINAL["thresh"], vt.FINAL["pre"], vt.FINAL["post"], raw_score=raw)
    assert np.array_equal(counts, fin["counts"]) and np.array_equal(counts, g[tag + "_final_counts"])
    for b in range(B):
        n = counts[b]
        idx, dist = match_rows(boxes[b, :n], g[name + "_box_preds"][b]) if n else (np.zeros((0,), np.int64), np.zeros((1,)))
        # (zero RoIs decode to the same zero-size box: their rows are told apart by nothing, so compare the rows they name)
        assert dist.max() <= 1e-4
        assert np.array_equal(g[name + "_box_preds"][b][idx], g[name + "_box_preds"][b][fin["index"][b, :n]]), (name, b)
        assert np.array_equal(boxes[b, n:], np.zeros((post - n, 7), np.float32)) and not scores[b, n:].any() and not labels[b, n:].any()
    assert np.array_equal(labels, g[tag + "_final_labels"])
    pairs = [("batch_box_preds", want_boxes, g[name + "_box_preds"], box_preds), ("pred_boxes", fin["boxes"], g[tag + "_final_boxes"], boxes)]
    if raw:
        assert np.array_equal(scores, g[tag + "_final_scores"])             # raw logits pass through unchanged
    else:
        pairs.append(("pred_scores", fin["scores"], g[tag + "_final_scores"], scores))
    judge("%s %s" % (what, tag), pairs)


@pytest.mark.parametrize("name,raw", [("car", False), ("car", True), ("multi", False)])
def test_roi_decode_and_final_selection_on_the_golden_rois(g, name, raw):
    out = run_final(name, g, raw)
    check_final(name, g, raw, out)
    if name == "car":
        assert out[4][1] == 0                                               # nothing of frame 1 passes SCORE_THRESH
        assert (np.abs(g["car_rois"][2]).sum(-1) == 0).sum() == 16          # zero-padded RoIs went in, and some came out:
        assert (np.abs(out[1][2, :out[4][2], 3:6]).sum(-1) == 0).any()      # zero-size boxes, as the reference returns them


def test_proposals_make_the_host_wait_for_nothing(g):
    """One call for all frames with no device-to-host copy: under torch's synchronisation debug mode any read of a device
    value by the host (item, tolist, nonzero, a boolean mask) raises."""
    from dualfusion import ops
    c = vt.CASES["car"]
    t = tables("car", g)
    rows = c["B"] * c["H"] * c["W"]
    cls, box, dirs = (dev(g["car_" + k].reshape(rows, -1)) for k in ("cls", "box", "dir"))
    x_shifts, y_shifts = t.on("cuda")
    table = t.table.tolist()
    rcnn_cls, rcnn_reg = dev(g["car_rcnn_cls"]), dev(g["car_rcnn_reg"])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = ops.anchor_proposals(cls, box, dirs, x_shifts, y_shifts, c["B"], c["H"], c["W"], c["C"], t.anchor_set, table, c["thresh"],
                                   c["pre"], c["post"], dir_offset=vt.DIR_OFFSET, dir_limit_offset=vt.DIR_LIMIT_OFFSET)
        rd = ops.roi_decode_select(out[0], rcnn_cls, rcnn_reg, None, 0.3, 0.1, 4096, 100)
        with pytest.raises(RuntimeError, match="synchroniz"):
            out[3].tolist()                                                 # the mode does see a read
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert np.array_equal(out[3].cpu().numpy(), restated("car", g)["num"]) and rd[4].shape == (3,)


def test_results_are_bit_identical_from_run_to_run(g):
    a, b = run_proposals("car", g), run_proposals("car", g)
    c, d = run_final("car", g, False), run_final("car", g, False)
    for x, y in zip(a + c, b + d):
        assert np.array_equal(x, y)


# ---------------------------------------------------------------------------------------------------- modules
MOD_H, MOD_W, MOD_B, MOD_C = 12, 10, 2, 16
HEAD_LEVELS = (("x_a", 1, 8), ("x_b", 2, 16))


def small_roi_head_cfg():
    def layer(radius, nsample, c, cout):
        return {"MLPS": [[c, cout]], "QUERY_RANGES": [[2, 2, 2]], "POOL_RADIUS": [radius], "NSAMPLE": [nsample], "POOL_METHOD": "max_pool"}
    return {"CLASS_AGNOSTIC": True, "SHARED_FC": [32], "CLS_FC": [16], "REG_FC": [16], "DP_RATIO": 0.3,
            "ROI_GRID_POOL": {"FEATURES_SOURCE": [n for n, _, _ in HEAD_LEVELS], "GRID_SIZE": 3,
                              "POOL_LAYERS": {"x_a": layer(0.57, 8, 16, 16), "x_b": layer(1.0, 16, 32, 32)}},
            "NMS_CONFIG": {"TEST": {"NMS_TYPE": "nms_gpu", "MULTI_CLASSES_NMS": False, "NMS_PRE_MAXSIZE": 128, "NMS_POST_MAXSIZE": 24,
                                    "NMS_THRESH": 0.7}}}


def module_pair(seed):
    """AnchorHeadSingle on a 12 x 10 map and a VoxelRCNNHead with TEST proposals 128 -> 24, weights drawn so that the logits
    spread like 2 N(0, 1) and the residuals like 0.05 N(0, 1)"""
    from dualfusion import dense_heads, roi_heads
    torch.manual_seed(seed)
    cfg = vt.head_cfg("car")
    grid, rng = np.array([MOD_W * 8, MOD_H * 8, 40]), vt._range(MOD_W, MOD_H)
    head = dense_heads.AnchorHeadSingle(cfg, MOD_C, 1, ["Car"], grid, rng).eval()
    with torch.no_grad():
        head.conv_cls.weight.normal_(0, 2 / np.sqrt(MOD_C))
        head.conv_cls.bias.zero_()
        head.conv_box.weight.normal_(0, 0.05 / np.sqrt(MOD_C))
        head.conv_dir_cls.weight.normal_(0, 1 / np.sqrt(MOD_C))
    rh = roi_heads.VoxelRCNNHead({n: c for n, _, c in HEAD_LEVELS}, small_roi_head_cfg(), [0.0, -2.4, 0.0, 7.0, 2.4, 1.0],
                                 [0.4, 0.2, 0.2]).eval()
    x = torch.randn(MOD_B, MOD_C, MOD_H, MOD_W)
    rcnn_cls, rcnn_reg = 2 * torch.randn(MOD_B * 24, 1), 0.05 * torch.randn(MOD_B * 24, 7)
    return head, rh, x, rcnn_cls, rcnn_reg


def module_margins(head, cls, box, dirs):
    anchors = head.anchors.numpy().reshape(-1, 7)
    n = anchors.shape[0]
    return vt.proposals(cls.reshape(MOD_B, n, 1), box.reshape(MOD_B, n, 7), dirs.reshape(MOD_B, n, 2), anchors, 128, 24, 0.7,
                        vt.DIR_OFFSET, vt.DIR_LIMIT_OFFSET)


MODULE_SEED = 1


def test_fused_and_composed_modules_agree_with_the_restatement(monkeypatch):
    from dualfusion import vr_detector
    head, rh, x, rcnn_cls, rcnn_reg = module_pair(MODULE_SEED)
    hd, rd = copy.deepcopy(head).cuda(), copy.deepcopy(rh).cuda()
    rd.post_process_cfg = vt.post_cfg()
    results = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("DF3D_VR_TAIL_FUSED", mode)
        with torch.no_grad():
            bd = hd({"batch_size": MOD_B, "spatial_features_2d": x.cuda()})
            assert ("dense_cls_rows" in bd) == (mode == "1") and ("batch_box_preds" in bd) == (mode == "0")
            if mode == "1":
                maps = [bd[k].cpu().numpy() for k in ("dense_cls_rows", "dense_box_rows", "dense_dir_rows")]
            rd.proposal_layer(bd, rd.model_cfg["NMS_CONFIG"]["TEST"])
            assert bd["has_class_labels"] is False and bd["roi_labels"].dtype == torch.int64
            bd["rcnn_cls"], bd["rcnn_reg"] = rcnn_cls.cuda(), rcnn_reg.cuda()
            rd.predict(bd)
            assert ("final_selection" in bd) == (mode == "1") and bd["cls_preds_normalized"] is False
            preds = vr_detector.post_processing(bd, rd.post_process_cfg)
        results[mode] = dict(rois=bd["rois"].cpu().numpy(), roi_scores=bd["roi_scores"].cpu().numpy(),
                             roi_labels=bd["roi_labels"].cpu().numpy(), box_preds=bd["batch_box_preds"].cpu().numpy(),
                             cls_preds=bd["batch_cls_preds"].cpu().numpy(), preds=[{k: v.cpu().numpy() for k, v in p.items()} for p in preds])
    cls, box, dirs = maps
    ref = module_margins(head, cls, box, dirs)
    assert ref["min_gap"] > 0 and ref["close"] == 0 and ref["floor_dist"] >= vt.FLOOR_MARGIN       # preconditions of exactness
    anchors = head.anchors.numpy().reshape(-1, 7)
    n = anchors.shape[0]
    dense, _ = vt.dense_decode(box.reshape(MOD_B, n, 7), dirs.reshape(MOD_B, n, 2), anchors, vt.DIR_OFFSET, vt.DIR_LIMIT_OFFSET)
    with torch.no_grad():                                                   # the float32 yardstick: the composition on the CPU
        view = lambda v: torch.from_numpy(v).view(MOD_B, MOD_H, MOD_W, -1)
        yard_dense = head.generate_predicted_boxes(MOD_B, view(cls), view(box), view(dirs))[1].numpy()
    yard_rois = np.where(ref["index"][..., None] >= 0, yard_dense[np.arange(MOD_B)[:, None], np.maximum(ref["index"], 0)], 0)
    want_preds = vt.roi_decode(ref["rois"], rcnn_reg.numpy())
    with torch.no_grad():
        yard_preds = rh.generate_predicted_boxes(MOD_B, torch.from_numpy(yard_rois), rcnn_cls, rcnn_reg)[1].numpy()
    fin = vt.final_select(want_preds, rcnn_cls.numpy(), None, vt.FINAL["score_thresh"], vt.FINAL["thresh"], vt.FINAL["pre"],
                          vt.FINAL["post"])
    assert fin["min_gap"] > 0 and fin["close"] == 0 and fin["thresh_dist"] >= 1e-4
    for mode, r in results.items():
        what = "modules fused" if mode == "1" else "modules composed"
        for b in range(MOD_B):
            m = ref["num"][b]
            idx, dist = match_rows(r["rois"][b, :m], dense[b])
            assert dist.max() <= 1e-4 and np.array_equal(idx, ref["index"][b, :m]), (what, b)
            assert not r["rois"][b, m:].any() and not r["roi_scores"][b, m:].any() and (r["roi_labels"][b] == 1).all()
            assert np.array_equal(r["roi_scores"][b, :m], cls.reshape(MOD_B, n)[b][idx])
            k = fin["counts"][b]
            assert len(r["preds"][b]["pred_scores"]) == k
            pidx, pdist = match_rows(r["preds"][b]["pred_boxes"], want_preds[b])
            assert (pdist.max() if k else 0) <= 1e-4 and np.array_equal(pidx, fin["index"][b, :k]), (what, b)
            assert (r["preds"][b]["pred_labels"] == 1).all()
        assert np.array_equal(r["cls_preds"].reshape(-1, 1), rcnn_cls.numpy())
        judge(what, [("rois", ref["rois"], yard_rois, r["rois"]), ("batch_box_preds", want_preds, yard_preds, r["box_preds"])])
    for b in range(MOD_B):
        for k in ("pred_boxes", "pred_scores"):
            assert np.abs(results["1"]["preds"][b][k] - results["0"]["preds"][b][k]).max(initial=0) <= 1e-5
    with pytest.raises(KeyError, match="rois"):
        rd({"batch_size": MOD_B})


# ---------------------------------------------------------------------------------------------------- whole chain
def test_whole_chain_returns_boxes_for_two_sweeps():
    from dualfusion import iou3d_nms, ops, synth, vr_detector
    import roipool_reference as rp
    torch.manual_seed(5)
    roi_cfg = dict(rp.HEAD_CFG)
    roi_cfg["NMS_CONFIG"] = {"TEST": {"NMS_TYPE": "nms_gpu", "MULTI_CLASSES_NMS": False, "NMS_PRE_MAXSIZE": 2048,
                                      "NMS_POST_MAXSIZE": 100, "NMS_THRESH": 0.7}}
    post = vt.post_cfg()
    post["NMS_CONFIG"]["NMS_POST_MAXSIZE"] = 500
    cfg = {"NAME": "VoxelRCNN", "BACKBONE_3D": {"NAME": "VoxelBackBone8x"},
           "MAP_TO_BEV": {"NAME": "HeightCompression", "NUM_BEV_FEATURES": 256},
           "BACKBONE_2D": {"NAME": "BaseBEVBackbone", "LAYER_NUMS": [1, 1], "LAYER_STRIDES": [1, 2], "NUM_FILTERS": [64, 128],
                           "UPSAMPLE_STRIDES": [1, 2], "NUM_UPSAMPLE_FILTERS": [128, 128]},
           "DENSE_HEAD": dict(vt.head_cfg("car")), "ROI_HEAD": roi_cfg, "POST_PROCESSING": post}
    model = vr_detector.VoxelRCNN(cfg, 1, ["Car"], np.array([1408, 1600, 40]), synth.KITTI_RANGE, synth.KITTI_VOXEL).cuda().eval()
    points = [torch.from_numpy(synth.kitti_sweep(seed=40 + b)[:, :4].copy()).cuda() for b in range(2)]
    feats, coords = ops.hard_voxelize_clouds(points, synth.KITTI_VOXEL, synth.KITTI_RANGE, 5, 40000, resident_inputs=False)
    with torch.no_grad():
        pred_dicts, _ = model({"voxel_features": feats, "voxel_coords": coords, "batch_size": 2})
    assert len(pred_dicts) == 2
    for p in pred_dicts:
        boxes, scores, labels = p["pred_boxes"], p["pred_scores"], p["pred_labels"]
        n = scores.shape[0]
        assert 0 < n <= 100 and tuple(boxes.shape) == (n, 7) and labels.shape[0] == n
        assert bool(torch.isfinite(boxes).all()) and bool(torch.isfinite(scores).all())
        assert bool((scores >= 0.3).all()) and bool((scores[1:] <= scores[:-1]).all())
        assert bool((labels == 1).all())
        iou = iou3d_nms.boxes_iou_bev(boxes.contiguous(), boxes.contiguous())
        iou.fill_diagonal_(0)
        assert float(iou.max()) <= 0.1 + 1e-4
