"""df3d_topk_keys on the MI355X on every path of topk_final_kernel and over its whole key range, against a full sort
(tests/topk_reference.py `select`).  Everything is integer-exact: outputs and counts are compared with np.array_equal.

tests/test_topk_host.py shows, without a GPU, that every family below reaches the path it is named after (region sort,
radix exit after level 0 / 1 / 2, streaming) and that hi = 1 and 3 (key bits 55:54) leave that route unchanged."""
import numpy as np
import pytest

import topk_reference as tr

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"


def run(keys, k):
    """keys u64 [S, n] -> (out u64 [S, k], count [S]) of the device; the input must come back unchanged"""
    from dualfusion import ops
    dev = torch.from_numpy(np.ascontiguousarray(keys).view(np.int64)).to(DEV)
    out, cnt = ops.topk_keys(dev, k)
    torch.cuda.synchronize()
    assert np.array_equal(dev.cpu().numpy().view(np.uint64), keys), "the keys were modified"
    return out.cpu().numpy().view(np.uint64), cnt.cpu().numpy()


def check(keys, k):
    want, want_cnt = tr.select(keys, k)
    out, cnt = run(keys, k)
    assert np.array_equal(cnt, want_cnt), (cnt.tolist(), want_cnt.tolist())
    assert np.array_equal(out, want), "first difference at %s" % (np.argwhere(out != want)[:1].tolist(),)


@pytest.mark.parametrize("k", [1, 100, 4096])
@pytest.mark.parametrize("hi", [0, 1, 3])
@pytest.mark.parametrize("name", sorted(tr.TIE_KINDS))
def test_tie_families_equal_a_full_sort(name, hi, k):
    check(tr.family(name, hi)[None], k)


@pytest.mark.parametrize("hi", [0, 1, 3])
@pytest.mark.parametrize("name", sorted(tr.EDGES))
def test_capacity_edges_equal_a_full_sort(name, hi):
    row, k, _ = tr.EDGES[name]
    check(row(hi)[None], k)


@pytest.mark.parametrize("name", sorted(tr.small_rows()))
def test_degenerate_sizes_equal_a_full_sort(name):
    row, k = tr.small_rows()[name]
    check(row[None], k)


@pytest.mark.parametrize("hi", [0, 3])
def test_one_launch_whose_segments_take_five_different_paths(hi):
    """The path is chosen per workgroup from device data: a saturated frame next to an ordinary one in a batch."""
    rows = [tr.family("ties_l1", hi, 11, tie=1000, seg=1), tr.family("ties_l0", hi, 12, seg=2), tr.family("ties_l1", hi, 13, seg=3),
            tr.family("ties_l2", hi, 14, seg=4), tr.family("identical", hi, 15, seg=5)]
    assert [tr.branch(r, 100) for r in rows] == list(tr.PATHS)
    keys = tr.stack(rows)
    assert keys.shape == (5, 9001)
    check(keys, 100)
    check(keys[::-1].copy(), 4096)


def test_300_short_segments():
    rs = np.random.RandomState(300)
    S, n, k = 300, 168, 60
    keys = (np.arange(S, dtype=np.uint64)[:, None] % np.uint64(256)) << np.uint64(56) | rs.randint(0, 1 << 56, size=(S, n)).astype(np.uint64)
    keys[rs.uniform(size=(S, n)) < 0.3] = tr.ONES
    keys[7, 5:] = tr.ONES                                       # a segment with fewer than k candidates
    keys[8] = (np.uint64(8) << np.uint64(56)) | np.uint64(0x00C0FFEE12345678)      # and one of identical keys, bits 55:54 set
    check(keys, k)


@pytest.mark.parametrize("name", ["identical", "identical_long", "ties_l2"])
def test_duplicates_give_bit_identical_results_from_run_to_run(name):
    """duplicate keys are appended to the sort buffer in the order of LDS atomics: the sorted output must not show it"""
    from dualfusion import ops
    keys = torch.from_numpy(tr.stack([tr.family(name, hi, seg=hi) for hi in (0, 1, 3)]).view(np.int64)).to(DEV)
    a, b = ops.topk_keys(keys, 4096), ops.topk_keys(keys, 4096)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---------------------------------------------------------------------------------------------------- the detection tails
# The same families through the real key builders: constant maps, more than TK_BUF (8192) equal candidates per segment, so
# only the index decides and the select leaves the region sort (index bits [13:6] differ: radix exit after level 1).
def rows_of(a):
    """[B, C, H, W] -> device rows [B*H*W, C]"""
    B, C, H, W = a.shape
    return torch.from_numpy(np.ascontiguousarray(a.transpose(0, 2, 3, 1).reshape(B * H * W, C))).to(DEV)


@pytest.mark.parametrize("pre_max", [100, 1000])
def test_centerhead_predict_on_constant_score_maps(pre_max):
    """One task, one class, 96 x 96 = 9216 pixels per sample: sample 0 has a constant score below 1, sample 1 the score 1.0
    exactly (logit 20: key bits [55:24] are all zero).  Boxes of 2 cm at a 0.6 m pitch: NMS suppresses nothing, so the kept
    pixels are 0 .. post_max - 1 in ascending order; each pixel carries its index in the velocity channel."""
    from dualfusion import ops
    from oracle import oracle as orc
    B, H, W, post_max = 2, 96, 96, pre_max
    f32 = np.float32
    assert H * W > tr.BUF
    pix = np.arange(H * W, dtype=f32).reshape(1, 1, H, W)
    p = dict(hm=np.stack([np.full((1, H, W), 0.3, f32), np.full((1, H, W), 20.0, f32)]), reg=np.full((B, 2, H, W), 0.5, f32),
             height=np.zeros((B, 1, H, W), f32), dim=np.full((B, 3, H, W), -4.0, f32),
             rot=np.stack([np.zeros((B, H, W), f32), np.ones((B, H, W), f32)], 1),
             vel=np.concatenate([np.broadcast_to(pix, (B, 1, H, W)), np.arange(B, dtype=f32).reshape(B, 1, 1, 1) * np.ones((1, 1, H, W), f32)], 1))
    assert f32(1) / (f32(1) + np.exp(f32(-20))) == f32(1)
    cfg = dict(post_center_limit_range=[-61.2, -61.2, -1.0, 61.2, 61.2, 1.0], score_threshold=0.1, pc_range=[-54, -54], out_size_factor=8,
               voxel_size=[0.075, 0.075], nms=dict(nms_pre_max_size=pre_max, nms_post_max_size=post_max, nms_iou_threshold=0.2))
    st = {}
    want = orc.centerhead_predict([p], cfg, [1], margin_out=st)
    assert st["iou_close"] == 0 and st["thr_gap"] > 1e-3 and st["range_gap"] > 1e-3
    task = {k: rows_of(v) for k, v in p.items()}
    task["label_base"] = 0
    boxes, scores, labels, counts = ops.centerhead_predict([task], B, H, W, 8, [0.075, 0.075], [-54, -54], cfg["post_center_limit_range"],
                                                           0.1, ops.NMS_ROTATED, 0.2, pre_max, post_max)
    torch.cuda.synchronize()
    assert counts.cpu().tolist() == [post_max, post_max]
    boxes, scores, labels = boxes.cpu().numpy(), scores.cpu().numpy(), labels.cpu().numpy()
    for b in range(B):
        assert len(want[b]["scores"]) == post_max
        assert np.array_equal(want[b]["box3d_lidar"][:, 6], np.arange(post_max, dtype=f32))        # what the oracle expects
        assert np.array_equal(boxes[b, :, 6], np.arange(post_max, dtype=f32)) and (boxes[b, :, 7] == b).all()
        np.testing.assert_allclose(boxes[b], want[b]["box3d_lidar"], rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(scores[b], want[b]["scores"], rtol=1e-5, atol=1e-6)
        assert labels[b].tolist() == want[b]["label_preds"].tolist()
    assert (scores[1] == 1).all()


@pytest.mark.parametrize("K", [200, 4000])
def test_heatmap_proposals_on_constant_maps(K):
    """B = 2, C = 2, 72 x 72 constant logits: every interior pixel is a 3 x 3 local maximum (the comparison is >=), 9800 equal
    scores per sample; the border's zeros come after them.  The order is exact: equal scores, ascending class * H * W + pixel."""
    from test_gpu_tfhead import _np_proposals
    from dualfusion import ops
    B, C, H, W = 2, 2, 72, 72
    heat = np.stack([np.full((C, H, W), 0.3, np.float32), np.full((C, H, W), 20.0, np.float32)])
    cls, pix, sup = _np_proposals(heat, K, (), 1)
    assert (sup > 0).reshape(B, -1).sum(1).tolist() == [9800, 9800] and 9800 > tr.BUF
    inner = np.array([y * W + x for y in range(1, H - 1) for x in range(1, W - 1)])
    assert np.array_equal(pix[0], inner[:K]) and (cls[0] == 0).all()                                # what the restatement expects
    tc, tp, qs, qp, _ = ops.heatmap_proposals(rows_of(heat), B, C, H, W, 3, (), K)
    torch.cuda.synchronize()
    assert np.array_equal(tc.cpu().numpy(), cls) and np.array_equal(tp.cpu().numpy(), pix)
    qs = qs.cpu().numpy()
    for b in range(B):
        np.testing.assert_allclose(qs[b], sup[b][:, pix[b]], rtol=1e-6, atol=1e-7)
    assert (qs[1] == 1).all()


@pytest.mark.parametrize("pre_max", [100, 1000])
def test_anchor_proposals_on_constant_logits(pre_max):
    """48 x 48 x 4 = 9216 anchors per frame with one logit (0.3 in frame 0, -1.5 in frame 1: both branches of the ordered
    float bits).  tests/test_gpu_vrtail.py test_proposals_order_by_the_raw_logits_and_ties_by_index has 40 anchors and at
    most three equal logits among the twelve it selects (28 equal ones stay unselected): a region sort.  Here 9216 tie.
    Anchors of 5 cm, the four of a pixel 0.1 m apart through their x residuals: NMS suppresses nothing, the kept anchors are
    0 .. post_max - 1."""
    import vrtail_reference as vt
    from dualfusion import dense_heads, ops
    B, H, W, A, post_max = 2, 48, 48, 4, pre_max
    n = H * W * A
    assert n > tr.BUF
    tiny = dict(vt.CAR, anchor_sizes=[[0.05, 0.05, 1.0]], anchor_rotations=[0, 0.5, 1.0, 1.57])
    t = dense_heads.AnchorTables([tiny], np.array([W * 8, H * 8, 40]), vt._range(W, H))
    anchors = t.dense().numpy().reshape(-1, 7)
    assert anchors.shape[0] == n and len(t.anchor_set) == A
    cls = np.stack([np.full((n, 1), 0.3, np.float32), np.full((n, 1), -1.5, np.float32)])
    box = np.zeros((B, n, 7), np.float32)
    box[:, :, 0] = (np.arange(n) % A) * np.float32(0.1 / np.hypot(0.05, 0.05))
    ref = vt.proposals(cls, box, None, anchors, pre_max, post_max, 0.7)
    assert ref["close"] == 0 and ref["suppressed"].tolist() == [0, 0] and ref["min_gap"] == 0
    assert np.array_equal(ref["index"], np.broadcast_to(np.arange(post_max), (B, post_max)))       # what the restatement expects
    x_shifts, y_shifts = t.on("cuda")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    rois, scores, labels, num = ops.anchor_proposals(dev(cls.reshape(B * H * W, A)), dev(box.reshape(B * H * W, A * 7)), None, x_shifts,
                                                     y_shifts, B, H, W, 1, t.anchor_set, t.table.tolist(), 0.7, pre_max, post_max)
    torch.cuda.synchronize()
    assert num.cpu().tolist() == [post_max, post_max] and bool((labels == 1).all())
    assert np.abs(rois.cpu().numpy() - ref["rois"]).max() <= 1e-4                                   # neighbours are 0.1 m apart
    assert np.array_equal(scores.cpu().numpy(), ref["roi_scores"].astype(np.float32))


def test_roi_decode_select_at_its_largest_roi_count():
    """df3d_roi_decode_select accepts at most 4096 RoIs per frame (9216 are refused, asserted below), so its select never
    leaves the region sort; with one logit for all 4096 RoIs the tie group is region 1 filled to its last slot (P = 4096).
    RoIs of 0.1 m on a 1 m grid, zero residuals: NMS suppresses nothing, the kept RoIs are 0 .. post_max - 1."""
    import vrtail_reference as vt
    from dualfusion import Df3dError, ops
    B, N, post_max = 2, tr.TIE_CAP, 100
    rois = np.zeros((B, N, 7), np.float32)
    rois[:, :, 0], rois[:, :, 1] = np.arange(N) % 64, np.arange(N) // 64
    rois[:, :, 3:6] = 0.1
    rcnn_cls = np.concatenate([np.full((N, 1), 0.3, np.float32), np.full((N, 1), 20.0, np.float32)])
    rcnn_reg = np.zeros((B * N, 7), np.float32)
    want_boxes = vt.roi_decode(rois, rcnn_reg)
    fin = vt.final_select(want_boxes, rcnn_cls, None, 0.3, 0.1, 4096, post_max)
    assert fin["close"] == 0 and fin["min_gap"] == 0 and fin["counts"].tolist() == [post_max, post_max]
    assert np.array_equal(fin["index"], np.broadcast_to(np.arange(post_max), (B, post_max)))
    dev = lambda a: torch.from_numpy(a).to(DEV)
    box_preds, boxes, scores, labels, counts = ops.roi_decode_select(dev(rois), dev(rcnn_cls), dev(rcnn_reg), None, 0.3, 0.1, 4096, post_max)
    torch.cuda.synchronize()
    assert counts.cpu().tolist() == [post_max, post_max] and bool((labels == 1).all())
    assert np.abs(boxes.cpu().numpy() - fin["boxes"]).max() <= 1e-5 and np.abs(box_preds.cpu().numpy() - want_boxes).max() <= 1e-5
    np.testing.assert_allclose(scores.cpu().numpy(), fin["scores"], rtol=1e-6)
    big = torch.zeros((1, 9216, 7), device=DEV)
    with pytest.raises((Df3dError, ValueError)):
        ops.roi_decode_select(big, torch.zeros((9216, 1), device=DEV), torch.zeros((9216, 7), device=DEV), None, 0.3, 0.1, 4096, post_max)
