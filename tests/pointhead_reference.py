"""Host reference of the PV-RCNN point head (csrc/pointhead.hip, dualfusion/dense_heads.py PointHeadSimple).

  points_in_boxes / assign_targets   numpy restatements that REPLAY the kernel's float32 arithmetic (z test, rotation by -rz,
                                     double comparisons against d / 2 + float(1e-5), first box wins): the label oracle
  assign_targets_f64                 the same geometry by brute force in float64
  near_face                          how many (point, box) pairs lie within 1e-4 m of a tested face in float64.  1e-4 m is more
                                     than 10 float32 spacings at the far edge of the KITTI range (7.6e-6 at 70.4 m): with
                                     near_face == 0 a label mismatch is a bug, not rounding (the library's cosf / sinf need not
                                     round as numpy's do)
  cls_layer_loss                     get_cls_layer_loss of the reference (one-hot targets, weights tensor) in torch, in the
                                     dtype of its input: float64 = the reference value and, through autograd, its gradient;
                                     float32 = the yardstick
  the fixtures                       seeded cases of the GPU tests, cleaned until near_face == 0, with their coverage counts"""
import numpy as np
import torch

F32 = np.float32
MARGIN = float(F32(1e-5))
NEAR = 1e-4
EXTRA = (0.2, 0.2, 0.2)
KITTI_RANGE = (0.0, -40.0, -3.0, 70.4, 40.0, 1.0)


# ---------------------------------------------------------------------------------------------------- geometry
def _local_f32(pts, boxes):
    """[n, 3], [N, 7] float32 -> az, ax, ay [n, N] as the kernel forms them: float32 differences, cos / sin of -rz in float32,
    products and sums one operation at a time"""
    pts, boxes = np.asarray(pts, F32), np.asarray(boxes, F32)
    x, y, z = pts[:, None, 0], pts[:, None, 1], pts[:, None, 2]
    az = np.abs(z - boxes[None, :, 2])
    sx, sy = x - boxes[None, :, 0], y - boxes[None, :, 1]
    a = -boxes[None, :, 6]
    cosa, sina = np.cos(a, dtype=F32), np.sin(a, dtype=F32)
    lx = (sx * cosa).astype(F32) + (sy * (-sina)).astype(F32)
    ly = (sx * sina).astype(F32) + (sy * cosa).astype(F32)
    return az.astype(F32), np.abs(lx).astype(F32), np.abs(ly).astype(F32)


def _inside(az, ax, ay, sizes):
    """check_pt_in_box3d: outside when az > dz / 2 (strict), inside when ax < dx / 2 + MARGIN and ay < dy / 2 + MARGIN, in double"""
    half = np.asarray(sizes, np.float64)[None] / 2.0
    return ~(az.astype(np.float64) > half[..., 2]) & (ax.astype(np.float64) < half[..., 0] + MARGIN) & \
        (ay.astype(np.float64) < half[..., 1] + MARGIN)


def first_true(mask):
    """[n, N] bool -> int32 [n]: the lowest index that is set, -1 if none"""
    hit = mask.any(axis=1)
    return np.where(hit, mask.argmax(axis=1), -1).astype(np.int32)


def points_in_boxes(boxes, pts):
    """points_in_boxes_gpu: boxes [B, N, 7], pts [B, npts, 3] -> int32 [B, npts]"""
    boxes, pts = np.asarray(boxes, F32), np.asarray(pts, F32)
    out = np.full(pts.shape[:2], -1, np.int32)
    for b in range(boxes.shape[0]):
        if boxes.shape[1]:
            out[b] = first_true(_inside(*_local_f32(pts[b], boxes[b]), boxes[b][:, 3:6]))
    return out


def frame_of(points, B):
    """the frame a row belongs to (`bs_idx == k` on floats), -1 for a row of no frame 0..B-1"""
    bf = np.asarray(points, F32)[:, 0]
    k = np.clip(np.nan_to_num(bf), 0, max(B - 1, 0)).astype(np.int64)
    return np.where((bf >= 0) & (bf < B) & (k.astype(F32) == bf), k, -1)


def _assign(points, gt, extra, num_class, local, as_sizes):
    P, (B, G) = len(points), gt.shape[:2]
    labels, idx = np.zeros((P,), np.int64), np.full((P,), -1, np.int32)
    detail = {"plain": np.zeros((P, G), bool), "ext": np.zeros((P, G), bool)}
    frame = frame_of(points, B)
    for b in range(B):
        rows = np.nonzero(frame == b)[0]
        if not len(rows) or not G:
            continue
        az, ax, ay = local(points[rows, 1:4], gt[b, :, :7])
        plain = _inside(az, ax, ay, as_sizes(gt[b, :, 3:6], None))
        ext = _inside(az, ax, ay, as_sizes(gt[b, :, 3:6], extra))
        detail["plain"][rows], detail["ext"][rows] = plain, ext
        first = first_true(plain)
        fg, e = first >= 0, ext.any(axis=1)
        cls = np.ones(len(rows), np.int64) if num_class == 1 else gt[b, np.maximum(first, 0), 7].astype(np.int64)
        lab = np.zeros(len(rows), np.int64)
        lab[fg ^ e] = -1                                                   # the reference's order: the ignore flag first,
        lab[fg] = cls[fg]                                                  # then the class over every foreground row
        labels[rows], idx[rows] = lab, first
    return labels, idx, detail


def assign_targets(points, gt_boxes, extra, num_class, detail=False):
    """assign_stack_targets (ignore flag) with the kernel's float32 arithmetic: points [P, 4], gt_boxes [B, G, 8]
    -> labels int64 [P], box_idx int32 [P] (, {'plain', 'ext'}: bool [P, G] of the row's own frame)"""
    points, gt = np.asarray(points, F32), np.asarray(gt_boxes, F32)
    sizes = lambda s, ex: s if ex is None else (s + np.asarray(ex, F32)).astype(F32)
    out = _assign(points, gt, extra, num_class, _local_f32, sizes)
    return out if detail else out[:2]


def _local_f64(pts, boxes):
    pts, boxes = np.asarray(pts, np.float64), np.asarray(boxes, np.float64)
    sx, sy = pts[:, None, 0] - boxes[None, :, 0], pts[:, None, 1] - boxes[None, :, 1]
    c, s = np.cos(-boxes[None, :, 6]), np.sin(-boxes[None, :, 6])
    return np.abs(pts[:, None, 2] - boxes[None, :, 2]), np.abs(sx * c - sy * s), np.abs(sx * s + sy * c)


def assign_targets_f64(points, gt_boxes, extra, num_class):
    """the same rules by brute force in float64 (the float32 INPUTS, widened; the enlarged sizes as float32 sums)"""
    points, gt = np.asarray(points, F32), np.asarray(gt_boxes, F32)
    sizes = lambda s, ex: s.astype(np.float64) if ex is None else (s + np.asarray(ex, F32)).astype(F32).astype(np.float64)
    return _assign(points, gt, extra, num_class, _local_f64, sizes)[:2]


def near_face(points, gt_boxes, extra):
    """(point, box of the point's frame) pairs whose float64 distance to a tested face -- xy at half size + 1e-5, z at half
    size, of the box and of the enlarged box -- is below 1e-4 m while the other two coordinates are within 1e-4 m of being
    inside.  A z distance of exactly 0 is not counted: on-face points are crafted from exactly representable numbers, which
    float32 and float64 evaluate alike."""
    points, gt = np.asarray(points, F32), np.asarray(gt_boxes, F32)
    B, G = gt.shape[:2]
    frame, n = frame_of(points, B), 0
    for b in range(B):
        rows = np.nonzero(frame == b)[0]
        if not len(rows) or not G:
            continue
        a = np.stack(_local_f64(points[rows, 1:4], gt[b, :, :7]), axis=-1)[..., [1, 2, 0]]            # ax, ay, az
        for ex in (None, extra):
            s = gt[b, :, 3:6] if ex is None else (gt[b, :, 3:6] + np.asarray(ex, F32)).astype(F32)
            lim = s.astype(np.float64)[None] / 2.0 + np.array([MARGIN, MARGIN, 0.0])
            d = np.abs(a - lim)
            close = d < NEAR
            close[..., 2] &= d[..., 2] != 0
            loose = a <= lim + NEAR
            for ax in range(3):
                others = [k for k in range(3) if k != ax]
                n += int((close[..., ax] & loose[..., others[0]] & loose[..., others[1]]).sum())
    return n


# ---------------------------------------------------------------------------------------------------- loss
def sigmoid_focal_loss(logits, target, weights, alpha=0.25, gamma=2.0):
    """SigmoidFocalClassificationLoss.forward (VR/pcdet/utils/loss_utils.py:9-72)"""
    p = torch.sigmoid(logits)
    alpha_weight = target * alpha + (1 - target) * (1 - alpha)
    pt = target * (1.0 - p) + (1.0 - target) * p
    bce = torch.clamp(logits, min=0) - logits * target + torch.log1p(torch.exp(-torch.abs(logits)))
    return alpha_weight * torch.pow(pt, gamma) * bce * weights.unsqueeze(-1)


def cls_layer_loss(preds, labels, weight):
    """get_cls_layer_loss (point_head_template.py:131-155) in the dtype of `preds` [P, C]; labels int64 [P] -> (loss, pos_num)"""
    num_class = preds.shape[1]
    positives = labels > 0
    cls_weights = ((labels == 0) * 1.0 + 1.0 * positives).to(preds.dtype)
    pos_normalizer = positives.sum(dim=0).to(preds.dtype)
    cls_weights = cls_weights / torch.clamp(pos_normalizer, min=1.0)
    one_hot = preds.new_zeros(labels.shape[0], num_class + 1)
    one_hot.scatter_(-1, (labels * (labels >= 0).long()).unsqueeze(dim=-1), 1.0)
    return sigmoid_focal_loss(preds, one_hot[..., 1:], cls_weights).sum() * weight, pos_normalizer


def loss_and_grad(preds, labels, weight, dtype, upstream=1.0):
    """numpy in -> (loss, pos_num, d(upstream * loss) / d preds) computed in `dtype` on the host, as float64 arrays"""
    x = torch.from_numpy(np.asarray(preds)).to(dtype).requires_grad_(True)
    loss, pos = cls_layer_loss(x, torch.from_numpy(np.asarray(labels, np.int64)), weight)
    (upstream * loss).backward()
    return float(loss.detach()), float(pos), x.grad.double().numpy()


def rel_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max(initial=0) / max(float(np.abs(want).max(initial=0)), 1e-30))


# ---------------------------------------------------------------------------------------------------- fixtures
MAIN_COUNTS = (300, 213)
# frame 0: boxes 0 and 1 overlap and differ in class; box 0 has cz 0.5, dz 2 (the on-face point); rows 3 and 4 are padding
MAIN_GT = np.array([[[10.0, 2.0, 0.5, 4.0, 2.0, 2.0, 0.3, 1], [11.0, 2.5, 0.5, 4.0, 2.0, 2.0, -0.4, 2],
                     [30.0, -10.0, -0.5, 0.8, 0.6, 1.75, 1.2, 3], [0] * 8, [0] * 8],
                    [[20.0, -5.0, -0.75, 3.9, 1.6, 1.5, 2.0, 2], [45.0, 12.0, -0.25, 1.75, 0.6, 1.75, -1.0, 3],
                     [8.0, -3.0, -1.0, 4.2, 1.8, 1.6, 0.0, 1], [0] * 8, [0] * 8]], F32)
ON_FACE = (10.0, 2.0, 1.5)               # |z - cz| = 1.0 = dz / 2 exactly: inside box 0 of frame 0
IN_BOTH = (10.75, 2.25, 0.25)            # inside boxes 0 and 1 of frame 0: the lower index (class 1) wins
PADDING_HIT = (0.05, 0.05, 0.05)         # inside the enlarged zero rows only: -1
EXT_ONLY = (30.0, -10.0, 0.4375)         # 0.0625 above the top face of box 2 of frame 0 (dz / 2 = 0.875): enlarged box only


def _scatter(rs, n, boxes):
    """n points: two thirds around the real boxes of the frame (inside, near and just outside them), the rest over the range"""
    real = boxes[np.abs(boxes[:, 3:6]).sum(axis=1) > 0]
    out = np.empty((n, 3), F32)
    for i in range(n):
        if len(real) and rs.uniform() < 0.67:
            g = real[rs.randint(len(real))]
            local = rs.uniform(-0.75, 0.75, 3) * (g[3:6] + 0.6)
            c, s = np.cos(g[6]), np.sin(g[6])
            out[i] = (g[0] + local[0] * c - local[1] * s, g[1] + local[0] * s + local[1] * c, g[2] + local[2])
        else:
            out[i] = [rs.uniform(KITTI_RANGE[k], KITTI_RANGE[k + 3]) for k in range(3)]
    return out


def clean(points, gt, extra, rs, keep=0):
    """redraw rows (not the first `keep`) until no pair is near a face"""
    points = np.array(points, F32, copy=True)
    B = gt.shape[0]
    for _ in range(200):
        bad = [i for i in range(keep, len(points)) if near_face(points[i:i + 1], gt, extra)]
        if not bad:
            assert near_face(points, gt, extra) == 0
            return points
        for i in bad:
            b = int(points[i, 0])
            points[i, 1:4] = _scatter(rs, 1, gt[b] if 0 <= b < B else gt[0])[0]
    raise AssertionError("could not clean the fixture")


def main_case(seed=11):
    """-> points [514, 4] stacked (300 rows of frame 0, 213 of frame 1, then one row of frame 2), gt [2, 5, 8]; the crafted
    rows come first in their frames"""
    rs = np.random.RandomState(seed)
    crafted0 = np.array([ON_FACE, IN_BOTH, PADDING_HIT, EXT_ONLY], F32)
    f0 = np.concatenate([crafted0, _scatter(rs, MAIN_COUNTS[0] - len(crafted0), MAIN_GT[0])])
    f1 = np.concatenate([np.array([PADDING_HIT], F32), _scatter(rs, MAIN_COUNTS[1] - 1, MAIN_GT[1])])
    stray = np.array([[2.0, 10.0, 2.0, 0.5]], F32)                                 # frame 2 of B = 2, at the centre of a box
    points = np.concatenate([np.concatenate([np.full((len(f), 1), b, F32), f], axis=1) for b, f in enumerate((f0, f1))] + [stray])
    fixed = np.zeros(len(points), bool)
    fixed[:len(crafted0)] = True
    fixed[MAIN_COUNTS[0]] = True
    fixed[-1] = True
    order = np.concatenate([np.nonzero(fixed)[0], np.nonzero(~fixed)[0]])
    cleaned = clean(points[order], MAIN_GT, EXTRA, rs, keep=int(fixed.sum()))
    points[order] = cleaned
    return points, MAIN_GT.copy()


MAIN_ROWS = {"on_face": 0, "in_both": 1, "padding_hit": 2, "ext_only": 3, "padding_hit_frame1": MAIN_COUNTS[0], "stray": 513}


def interleaved(points, seed=3):
    """the same rows in a seeded order that mixes the frames -> (points, the permutation)"""
    perm = np.random.RandomState(seed).permutation(len(points))
    return points[perm].copy(), perm


def empty_frame_case():
    """B = 3 with no point in frame 1: the main rows of frame 1 moved to frame 2 (the stray row then belongs to it too)"""
    points, gt = main_case()
    points = points.copy()
    points[points[:, 0] >= 1, 0] = 2
    gt3 = np.stack([gt[0], gt[1], gt[1]])
    rs = np.random.RandomState(5)
    return clean(points, gt3, EXTRA, rs, keep=0), gt3


def chunk_case(seed=7, G=130):
    """G = 130 ground-truth rows (a second LDS chunk of 128): small boxes on a lattice; the LAST box owns row 0, box 128 row 1
    -> points [300, 4] of one frame, gt [1, 130, 8]"""
    rs = np.random.RandomState(seed)
    gt = np.zeros((1, G, 8), F32)
    for k in range(G):
        gt[0, k] = [4.0 + 5.0 * (k % 13), -30.0 + 6.0 * (k // 13), -1.0 + 0.125 * (k % 5), 2.0 + 0.25 * (k % 3), 1.5, 1.5,
                    0.25 * (k % 7) - 0.75, 1 + k % 3]
    pts = _scatter(rs, 300, gt[0])
    pts[0], pts[1] = gt[0, G - 1, :3], gt[0, G - 2, :3]
    points = np.concatenate([np.zeros((300, 1), F32), pts], axis=1)
    return clean(points, gt, EXTRA, rs, keep=2), gt


NEG_EXTRA = (0.2, -0.3, 0.2)


def negative_extra_case(seed=9):
    """extra width with a negative entry on the overlapping boxes of the main case's frame 0: rows inside a box but outside
    every `enlarged` (here shrunken) box exist; the reference writes the class over the ignore flag there
    -> points [257, 4] of one frame, gt [1, 5, 8]"""
    rs = np.random.RandomState(seed)
    gt = MAIN_GT[:1].copy()
    pts = np.stack([rs.uniform(7.5, 13.5, 257), rs.uniform(0.0, 4.5, 257), rs.uniform(-0.8, 1.8, 257)], axis=1).astype(F32)
    points = np.concatenate([np.zeros((257, 1), F32), pts], axis=1)
    return clean_neg(points, gt, rs), gt


def clean_neg(points, gt, rs):
    for _ in range(200):
        bad = [i for i in range(len(points)) if near_face(points[i:i + 1], gt, NEG_EXTRA)]
        if not bad:
            return points
        for i in bad:
            points[i, 1:4] = [rs.uniform(7.5, 13.5), rs.uniform(0.0, 4.5), rs.uniform(-0.8, 1.8)]
    raise AssertionError("could not clean the fixture")


def fg_without_ext_rows(points, gt, extra):
    """rows inside a box and inside no enlarged box (possible only under a negative extra width)"""
    _, idx, d = assign_targets(points, gt, extra, 3, detail=True)
    return [int(i) for i in np.nonzero(idx >= 0)[0] if not d["ext"][i].any()]


TARGET_CASES = ("main", "interleaved", "empty_frame", "no_gt", "chunk", "negative_extra")


def target_case(name):
    """-> points [P, 4], gt [B, G, 8], extra"""
    if name == "main":
        return main_case() + (EXTRA,)
    if name == "interleaved":
        points, gt = main_case()
        return interleaved(points)[0], gt, EXTRA
    if name == "empty_frame":
        return empty_frame_case() + (EXTRA,)
    if name == "no_gt":
        return main_case()[0], np.zeros((2, 0, 8), F32), EXTRA
    if name == "chunk":
        return chunk_case() + (EXTRA,)
    if name == "negative_extra":
        return negative_extra_case() + (NEG_EXTRA,)
    raise KeyError(name)


LOSS_P = 513
LOSS_WEIGHT = 1.0
LOSS_CASES = ("c1", "c3", "no_positive", "all_ignored")


def loss_case(name, seed=21):
    """-> preds float32 [513, C] (two rows hold logits of +-40), labels int64 [513]"""
    rs = np.random.RandomState(seed + LOSS_CASES.index(name))
    C = 1 if name == "c1" else 3
    preds = (rs.standard_normal((LOSS_P, C)) * 3).astype(F32)
    preds[5], preds[6] = 40.0, -40.0
    if name == "no_positive":
        labels = rs.choice([-1, 0], LOSS_P)
    elif name == "all_ignored":
        labels = np.full(LOSS_P, -1)
    else:
        labels = rs.choice(np.arange(-1, C + 1), LOSS_P, p=[0.15, 0.55] + [0.3 / C] * C)
        labels[5], labels[6] = 1, 0                                       # +40 on a positive, -40 on a background row
        labels[7], preds[7] = C, -40.0                                    # a confidently wrong positive
    return preds, labels.astype(np.int64)


# ---------------------------------------------------------------------------------------------------- configs
def point_head_cfg(fc=(32, 32), before_fusion=True, agnostic=False):
    """POINT_HEAD of kitti_models/pv_rcnn_mm_*.yaml with test-sized layers (plain dicts)"""
    return {"NAME": "PointHeadSimple", "CLS_FC": list(fc), "CLASS_AGNOSTIC": agnostic, "USE_POINT_FEATURES_BEFORE_FUSION": before_fusion,
            "TARGET_CONFIG": {"GT_EXTRA_WIDTH": list(EXTRA)},
            "LOSS_CONFIG": {"LOSS_REG": "smooth-l1", "LOSS_WEIGHTS": {"point_cls_weight": 1.0}}}


def pv_rcnn_cfg(num_keypoints=256, sources=("bev", "x_conv3", "raw_points")):
    """A PVRCNN config shaped like the tail of pv_rcnn_mm_mvx+actrv2.yaml: the whole-chain set-up of tests/test_gpu_vrtail.py
    with PFE and POINT_HEAD added and the PV-RCNN RoI head; TRAIN proposals inside the candidate cap."""
    import anchorloss_reference as al
    import stacksa_reference as sr
    import vrtail_reference as vt
    nms = lambda pre, post, thresh: {"NMS_TYPE": "nms_gpu", "MULTI_CLASSES_NMS": False, "NMS_PRE_MAXSIZE": pre,
                                     "NMS_POST_MAXSIZE": post, "NMS_THRESH": thresh}
    roi = sr.head_cfg()
    roi["NMS_CONFIG"] = {"TRAIN": nms(2048, 64, 0.8), "TEST": nms(2048, 100, 0.7)}
    roi["TARGET_CONFIG"] = dict(roi["TARGET_CONFIG"], ROI_PER_IMAGE=16)
    roi["ROI_GRID_POOL"] = dict(roi["ROI_GRID_POOL"], GRID_SIZE=3)
    pfe = dict(sr.vsa_cfg(), NUM_KEYPOINTS=num_keypoints, FEATURES_SOURCE=list(sources))
    pfe.pop("VOXEL_SIZE"), pfe.pop("POINT_CLOUD_RANGE")
    post = vt.post_cfg()
    post["NMS_CONFIG"]["NMS_POST_MAXSIZE"] = 500
    return {"NAME": "PVRCNN", "BACKBONE_3D": {"NAME": "VoxelBackBone8x"},
            "MAP_TO_BEV": {"NAME": "HeightCompression", "NUM_BEV_FEATURES": 256}, "PFE": pfe,
            "BACKBONE_2D": {"NAME": "BaseBEVBackbone", "LAYER_NUMS": [1, 1], "LAYER_STRIDES": [1, 2], "NUM_FILTERS": [64, 128],
                            "UPSAMPLE_STRIDES": [1, 2], "NUM_UPSAMPLE_FILTERS": [128, 128]},
            "DENSE_HEAD": al.train_head_cfg("car"), "POINT_HEAD": point_head_cfg(), "ROI_HEAD": roi, "POST_PROCESSING": post}
