"""Float64 numpy restatement of the Voxel-RCNN tail (anchor proposals, RoI decode, final selection), written from the formulas
of DESIGN section 7.11, and the margin predicates that make an index mismatch a bug and not rounding.  Test infrastructure:
never imported by the package.

Shapes: cls [B, H*W*A, C], box [B, H*W*A, 7], dir [B, H*W*A, NB] or None, anchors [H*W*A, 7]; anchor i = (y*W + x)*A + a."""
import numpy as np

from oracle import oracle as orc

U32 = 2.0 ** -24
IOU_MARGIN = 1e-4
FLOOR_MARGIN = 1e-3


def first_argmax(v):
    """max and first arg-max along the last axis (torch.max)"""
    idx = np.argmax(v, axis=-1)
    return np.take_along_axis(v, idx[..., None], -1)[..., 0], idx


def descending(scores):
    """indices by descending score, ties to the lower index"""
    return np.argsort(-np.asarray(scores, np.float64), kind="stable")


def min_gap(scores):
    """smallest gap between two scores of one list (0 = a tie)"""
    s = np.sort(np.asarray(scores, np.float64))
    return float(np.diff(s).min()) if len(s) > 1 else np.inf


def residual_decode(t, a):
    """t, a [..., 7] float64 -> boxes [..., 7]"""
    t, a = np.asarray(t, np.float64), np.asarray(a, np.float64)
    diag = np.sqrt(a[..., 3] ** 2 + a[..., 4] ** 2)
    return np.stack([t[..., 0] * diag + a[..., 0], t[..., 1] * diag + a[..., 1], t[..., 2] * a[..., 5] + a[..., 2],
                     np.exp(t[..., 3]) * a[..., 3], np.exp(t[..., 4]) * a[..., 4], np.exp(t[..., 5]) * a[..., 5],
                     t[..., 6] + a[..., 6]], -1)


def direction(rg, dir_logits, dir_offset, dir_limit_offset):
    """-> corrected heading, distance of v/p + o from the nearest integer (what floor sees)"""
    nb = dir_logits.shape[-1]
    period = 2 * np.pi / nb
    lab = first_argmax(dir_logits)[1]
    v = rg - dir_offset
    q = v / period + dir_limit_offset
    dist = np.abs(q - np.round(q))
    return v - np.floor(q) * period + dir_offset + period * lab, dist


def dense_decode(box, dir, anchors, dir_offset=0.0, dir_limit_offset=0.0):
    """every anchor of every frame decoded: [B, n, 7] float64, floor distances [B, n] (or None)"""
    out = residual_decode(box, np.asarray(anchors, np.float64)[None])
    dist = None
    if dir is not None:
        out[..., 6], dist = direction(out[..., 6], np.asarray(dir, np.float64), dir_offset, dir_limit_offset)
    return out, dist


def nms(boxes_sorted, thresh, margin=IOU_MARGIN):
    """rotated NMS of score-ordered boxes through the project's NMS oracle -> (keep, IoUs within margin of the threshold)"""
    if len(boxes_sorted) == 0:
        return np.zeros((0,), np.int64), 0
    return orc.nms_bev(np.asarray(boxes_sorted, np.float32), thresh, rotated=True, margin=margin)


def proposals(cls, box, dir, anchors, pre_max, post_max, thresh, dir_offset=0.0, dir_limit_offset=0.0):
    """-> dict: index [B, POST] (anchor indices, -1 in unused slots), rois [B, POST, 7] f64, roi_scores [B, POST],
    roi_labels [B, POST], num [B], and the margins (min_gap, floor_dist, close, suppressed [B])."""
    B, n = cls.shape[0], cls.shape[1]
    k = min(pre_max, n)
    res = dict(index=-np.ones((B, post_max), np.int64), rois=np.zeros((B, post_max, 7)), roi_scores=np.zeros((B, post_max)),
               roi_labels=np.ones((B, post_max), np.int64), num=np.zeros((B,), np.int64), suppressed=np.zeros((B,), np.int64))
    gap, floor_dist, close = np.inf, np.inf, 0
    for b in range(B):
        score, label = first_argmax(np.asarray(cls[b], np.float64))
        gap = min(gap, min_gap(score))
        top = descending(score)[:k]
        boxes = residual_decode(box[b][top], np.asarray(anchors, np.float64)[top])
        if dir is not None:
            boxes[:, 6], dist = direction(boxes[:, 6], np.asarray(dir[b][top], np.float64), dir_offset, dir_limit_offset)
            floor_dist = min(floor_dist, float(dist.min()))
        keep, c = nms(boxes, thresh)
        close += c
        res["suppressed"][b] = k - len(keep)
        keep = keep[:post_max]
        m = len(keep)
        res["num"][b] = m
        res["index"][b, :m] = top[keep]
        res["rois"][b, :m] = boxes[keep]
        res["roi_scores"][b, :m] = score[top[keep]]
        res["roi_labels"][b, :m] = label[top[keep]] + 1
    res.update(min_gap=gap, floor_dist=floor_dist, close=close)
    return res


def roi_decode(rois, rcnn_reg):
    """rois [B, N, 7], rcnn_reg [B*N, 7] -> batch_box_preds [B, N, 7] float64"""
    rois = np.asarray(rois, np.float64)
    B, N = rois.shape[:2]
    local = rois.copy()
    local[..., 0:3] = 0
    g = residual_decode(np.asarray(rcnn_reg, np.float64).reshape(B, N, 7), local)
    c, s = np.cos(rois[..., 6]), np.sin(rois[..., 6])
    x, y = g[..., 0] * c - g[..., 1] * s, g[..., 0] * s + g[..., 1] * c
    g[..., 0], g[..., 1] = x + rois[..., 0], y + rois[..., 1]
    g[..., 2] += rois[..., 2]
    return g


def final_select(box_preds, rcnn_cls, roi_labels, score_thresh, thresh, pre_max, post_max, raw_score=False):
    """box_preds [B, N, 7], rcnn_cls [B*N, C], roi_labels [B, N] or None -> dict: index [B, POST] (-1 unused), counts [B],
    scores / labels [B, POST], margins (min_gap over the candidates, thresh_dist, close)."""
    B, N = box_preds.shape[:2]
    logits = np.asarray(rcnn_cls, np.float64).reshape(B, N, -1)
    res = dict(index=-np.ones((B, post_max), np.int64), counts=np.zeros((B,), np.int64), scores=np.zeros((B, post_max)),
               labels=np.zeros((B, post_max), np.int64), boxes=np.zeros((B, post_max, 7)))
    gap, close, thresh_dist = np.inf, 0, np.inf
    for b in range(B):
        raw, label = first_argmax(logits[b])
        score = 1.0 / (1.0 + np.exp(-raw))
        thresh_dist = min(thresh_dist, float(np.abs(score - score_thresh).min()))
        cand = np.nonzero(score >= score_thresh)[0]
        if len(cand) == 0:
            continue
        gap = min(gap, min_gap(score[cand]))
        top = cand[descending(score[cand])[:pre_max]]
        keep, c = nms(box_preds[b][top], thresh)
        close += c
        sel = top[keep[:post_max]]
        m = len(sel)
        res["counts"][b] = m
        res["index"][b, :m] = sel
        res["boxes"][b, :m] = box_preds[b][sel]
        res["scores"][b, :m] = raw[sel] if raw_score else score[sel]
        res["labels"][b, :m] = roi_labels[b][sel] if roi_labels is not None else label[sel] + 1
    res.update(min_gap=gap, close=close, thresh_dist=thresh_dist)
    return res


def rel_err(got, want):
    """max error over max magnitude of one tensor"""
    want = np.asarray(want, np.float64)
    scale = float(np.abs(want).max()) if want.size else 0.0
    if want.size == 0:
        return 0.0
    return float(np.abs(np.asarray(got, np.float64) - want).max()) / (scale if scale > 0 else 1.0)


# ---- the configurations of the fixture (tests/golden/vr_tail.npz; tests/golden/make_golden_vrtail.py writes it) -------------
# (x, y, z) range chosen so that a stride-8 map of 0.05 m voxels has a 0.4 m anchor pitch without align_center
def _range(W, H):
    return [0.0, -0.2 * (H - 1), -3.0, 0.4 * (W - 1), 0.2 * (H - 1), 1.0]


CAR = {"class_name": "Car", "anchor_sizes": [[3.9, 1.6, 1.56]], "anchor_rotations": [0, 1.57], "anchor_bottom_heights": [-1.78],
       "align_center": False, "feature_map_stride": 8, "matched_threshold": 0.6, "unmatched_threshold": 0.45}
PED = {"class_name": "Pedestrian", "anchor_sizes": [[0.8, 0.6, 1.73]], "anchor_rotations": [0, 1.57],
       "anchor_bottom_heights": [-0.6], "align_center": True, "feature_map_stride": 8, "matched_threshold": 0.5,
       "unmatched_threshold": 0.35}
CYC = {"class_name": "Cyclist", "anchor_sizes": [[1.76, 0.6, 1.73]], "anchor_rotations": [0, 1.57],
       "anchor_bottom_heights": [-0.9], "align_center": False, "feature_map_stride": 8, "matched_threshold": 0.5,
       "unmatched_threshold": 0.35}

CASES = {
    # name: H, W, B, sets, C, NB (0 = no direction classifier), PRE, POST, NMS threshold
    "car": dict(H=25, W=22, B=3, sets=[CAR], C=1, NB=2, pre=256, post=32, thresh=0.7),
    "small": dict(H=5, W=4, B=2, sets=[CAR], C=1, NB=2, pre=256, post=32, thresh=0.7),
    "multi": dict(H=10, W=8, B=2, sets=[CAR, PED, CYC], C=3, NB=2, pre=256, post=32, thresh=0.7),
    "nodir": dict(H=25, W=22, B=3, sets=[CAR], C=1, NB=0, pre=256, post=32, thresh=0.7),
}
DIR_OFFSET, DIR_LIMIT_OFFSET = 0.78539, 0.0
FINAL = dict(score_thresh=0.3, thresh=0.1, pre=4096, post=100)


def case_geometry(name):
    """-> grid_size [3] (voxels), point_cloud_range [6] of a case"""
    c = CASES[name]
    return np.array([c["W"] * 8, c["H"] * 8, 40]), _range(c["W"], c["H"])


def head_cfg(name):
    """the AnchorHeadSingle config of a case (plain dicts)"""
    c = CASES[name]
    cfg = {"NAME": "AnchorHeadSingle", "CLASS_AGNOSTIC": False, "DIR_OFFSET": DIR_OFFSET, "DIR_LIMIT_OFFSET": DIR_LIMIT_OFFSET,
           "NUM_DIR_BINS": 2, "ANCHOR_GENERATOR_CONFIG": c["sets"],
           "TARGET_ASSIGNER_CONFIG": {"NAME": "AxisAlignedTargetAssigner", "BOX_CODER": "ResidualCoder"}}
    if c["NB"]:
        cfg["USE_DIRECTION_CLASSIFIER"] = True
    return cfg


def nms_cfg(name):
    c = CASES[name]
    return {"NMS_TYPE": "nms_gpu", "MULTI_CLASSES_NMS": False, "NMS_PRE_MAXSIZE": c["pre"], "NMS_POST_MAXSIZE": c["post"],
            "NMS_THRESH": c["thresh"]}


def post_cfg(raw=False):
    return {"RECALL_THRESH_LIST": [0.3, 0.5, 0.7], "SCORE_THRESH": FINAL["score_thresh"], "OUTPUT_RAW_SCORE": raw,
            "EVAL_METRIC": "kitti", "NMS_CONFIG": {"MULTI_CLASSES_NMS": False, "NMS_TYPE": "nms_gpu", "NMS_THRESH": FINAL["thresh"],
                                                   "NMS_PRE_MAXSIZE": FINAL["pre"], "NMS_POST_MAXSIZE": FINAL["post"]}}
