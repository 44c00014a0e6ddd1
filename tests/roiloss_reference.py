"""Float64 numpy restatement of the Voxel-RCNN second-stage training path (ProposalTargetLayer, the canonical transform of
RoIHeadTemplate.assign_targets and the three RCNN losses with their analytic gradients), written from the formulas of DESIGN
section 7.14; the case table and the seeded input generators of the fixture tests/golden/roi_loss.npz; and the margin and
coverage predicates that make an index or label mismatch a bug and not rounding.  Test infrastructure: never imported by
the package.

Shapes: rois [B, R, 7] = (x, y, z, dx, dy, dz, heading); roi_scores [B, R]; roi_labels [B, R] (1-based); gt [B, G, 8] = (box,
class); u_fg [B, R], u_slot [B, M] float32 draws in [0, 1); rcnn_cls [B*M, 1], rcnn_reg [B*M, 7]."""
import numpy as np

THRESH_MARGIN = 1e-4     # max IoU of a RoI from any of the four thresholds
GAP_MARGIN = 1e-6        # best and second-best IoU of a RoI (unless both are exactly 0); direct and flipped corner distance
HEADING_MARGIN = 1e-3    # folded heading from pi/2, pi and 3 pi/2
BETA_MARGIN = 1e-4       # |code-weighted diff| from 1/9; corner distance from 1
LOGIT_MAX = 8.0
BETA = 1.0 / 9.0
TWO_PI = 2 * np.pi

B, M, G, NUM_CLASS = 6, 16, 8, 3
SAMPLER = {"ROI_PER_IMAGE": M, "FG_RATIO": 0.5, "SAMPLE_ROI_BY_EACH_CLASS": True, "CLS_SCORE_TYPE": "roi_iou", "CLS_FG_THRESH": 0.75,
           "CLS_BG_THRESH": 0.25, "CLS_BG_THRESH_LO": 0.1, "HARD_BG_RATIO": 0.8, "REG_FG_THRESH": 0.55}
LOSS_CFG = {"CLS_LOSS": "BinaryCrossEntropy", "REG_LOSS": "smooth-l1", "CORNER_LOSS_REGULARIZATION": True,
            "LOSS_WEIGHTS": {"rcnn_cls_weight": 1.0, "rcnn_reg_weight": 1.5, "rcnn_corner_weight": 0.75,
                             "code_weights": [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.5]}}
# R is no multiple of 64 (100) or of 256 (300)
CASES = {
    "iou": dict(R=100, by_class=True, score="roi_iou"),
    "cls": dict(R=100, by_class=False, score="cls"),
    "wide": dict(R=300, by_class=True, score="cls"),
}
SIZES = np.array([[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]])       # Car, Pedestrian, Cyclist
RANGE = np.array([0.0, -40.0, 70.4, 40.0])


def sampler_cfg(name, m=M):
    cfg = dict(SAMPLER)
    cfg.update(ROI_PER_IMAGE=m, SAMPLE_ROI_BY_EACH_CLASS=CASES[name]["by_class"], CLS_SCORE_TYPE=CASES[name]["score"])
    return cfg


def frame_plan(R):
    """(n_fg, n_hard, n_easy) of the six frames: more fg than round(FG_RATIO * M); fewer; hard bg only; easy bg only; fg only;
    the empty frame (all easy)"""
    return [(20, 30, R - 50), (3, 30, R - 33), (10, R - 10, 0), (10, 0, R - 10), (R, 0, 0), (0, 0, R)]


# ---------------------------------------------------------------------------------------------------- 3-D IoU, float64
def _corners(b):
    hx, hy = b[:, 3] / 2, b[:, 4] / 2
    px, py = np.stack([-hx, hx, hx, -hx], 1), np.stack([-hy, -hy, hy, hy], 1)
    c, s = np.cos(b[:, 6])[:, None], np.sin(b[:, 6])[:, None]
    return np.stack([px * c - py * s + b[:, 0:1], px * s + py * c + b[:, 1:2]], -1)


def _cross(u, v):
    return u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]


def _inside(pts, b):
    """pts [P, 4, 2] strictly inside box b [P, 7]"""
    d = pts - b[:, None, 0:2]
    c, s = np.cos(b[:, 6])[:, None], np.sin(b[:, 6])[:, None]
    lx, ly = d[..., 0] * c + d[..., 1] * s, -d[..., 0] * s + d[..., 1] * c
    return (np.abs(lx) < b[:, None, 3] / 2) & (np.abs(ly) < b[:, None, 4] / 2)


def bev_overlap_pairs(a, b):
    """area of the intersection of the footprints of paired boxes a, b [P, 7] -> [P]: the vertices of the intersection polygon
    (proper edge crossings and the corners of one box inside the other), ordered about their centroid, shoelace"""
    P = a.shape[0]
    if P == 0:
        return np.zeros((0,))
    A, Bc = _corners(a), _corners(b)
    p, r = A[:, :, None, :], (np.roll(A, -1, 1) - A)[:, :, None, :]
    q, s = Bc[:, None, :, :], (np.roll(Bc, -1, 1) - Bc)[:, None, :, :]
    rxs = _cross(r, s)
    safe = np.where(rxs == 0, 1.0, rxs)
    t, u = _cross(q - p, s) / safe, _cross(q - p, r) / safe
    hit = (rxs != 0) & (t > 0) & (t < 1) & (u > 0) & (u < 1)
    X = p + t[..., None] * r
    pts = np.concatenate([X.reshape(P, 16, 2), Bc, A], 1)
    ok = np.concatenate([hit.reshape(P, 16), _inside(Bc, a), _inside(A, b)], 1)
    cnt = ok.sum(1)
    ctr = (pts * ok[..., None]).sum(1) / np.maximum(cnt, 1)[:, None]
    rel = pts - ctr[:, None, :]
    ang = np.where(ok, np.arctan2(rel[..., 1], rel[..., 0]), np.inf)
    order = np.argsort(ang, 1, kind="stable")
    rel = np.take_along_axis(rel, order[..., None], 1)
    good = np.take_along_axis(ok, order, 1)
    rel = np.where(good[..., None], rel, rel[:, 0:1, :])           # the unused slots repeat the first vertex: no area
    nxt = np.roll(rel, -1, 1)
    area = 0.5 * np.abs((rel[..., 0] * nxt[..., 1] - nxt[..., 0] * rel[..., 1]).sum(1))
    return np.where(cnt >= 3, area, 0.0)


def iou3d(a, b):
    """pcdet's boxes_iou3d_gpu in float64: a [n, 7], b [m, 7] -> [n, m]"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    n, m = a.shape[0], b.shape[0]
    h = np.clip(np.minimum((a[:, 2] + a[:, 5] / 2)[:, None], (b[:, 2] + b[:, 5] / 2)[None]) -
                np.maximum((a[:, 2] - a[:, 5] / 2)[:, None], (b[:, 2] - b[:, 5] / 2)[None]), 0, None)
    reach = 0.5 * np.hypot(a[:, 3], a[:, 4])[:, None] + 0.5 * np.hypot(b[:, 3], b[:, 4])[None]
    near = (np.hypot(a[:, 0:1] - b[None, :, 0], a[:, 1:2] - b[None, :, 1]) <= reach * (1 + 1e-9) + 1e-9) & (h > 0)
    i, j = np.nonzero(near)
    bev = np.zeros((n, m))
    bev[i, j] = bev_overlap_pairs(a[i], b[j])
    o3 = bev * h
    vol_a, vol_b = (a[:, 3] * a[:, 4] * a[:, 5])[:, None], (b[:, 3] * b[:, 4] * b[:, 5])[None]
    return o3 / np.maximum(vol_a + vol_b - o3, 1e-6)


def bev_overlap_clip(a, b):
    """a second, independent evaluation of one pair: Sutherland-Hodgman clipping of a's footprint by b's four half planes"""
    poly = [tuple(v) for v in _corners(np.asarray(a, np.float64)[None])[0]]
    clip = _corners(np.asarray(b, np.float64)[None])[0]
    for k in range(4):
        e0, e1 = clip[k], clip[(k + 1) % 4]
        side = lambda v: (e1[0] - e0[0]) * (v[1] - e0[1]) - (e1[1] - e0[1]) * (v[0] - e0[0])
        out = []
        for i in range(len(poly)):
            cur, prev = poly[i], poly[i - 1]
            sc, sp = side(cur), side(prev)
            if (sc >= 0) != (sp >= 0):
                w = sp / (sp - sc)
                out.append((prev[0] + w * (cur[0] - prev[0]), prev[1] + w * (cur[1] - prev[1])))
            if sc >= 0:
                out.append(cur)
        poly = out
        if not poly:
            return 0.0
    x, y = np.array([v[0] for v in poly]), np.array([v[1] for v in poly])
    return 0.5 * abs(float((x * np.roll(y, -1) - np.roll(x, -1) * y).sum()))


# ---------------------------------------------------------------------------------------------------- targets
def valid_count(gt):
    k = gt.shape[0] - 1
    while k > 0 and gt[k].sum() == 0:
        k -= 1
    return k + 1


def max_overlaps(rois, labels, gt, by_class):
    """-> best IoU [R], its ground-truth row [R], the second-best IoU among the rows that competed [R] (-1: none)"""
    n = valid_count(gt)
    iou = iou3d(rois[:, :7], gt[:n, :7])
    if by_class:
        iou = np.where(gt[None, :n, 7].astype(np.int64) == labels[:, None], iou, -1.0)
    arg = iou.argmax(1)                                               # first maximum wins
    best = iou[np.arange(len(arg)), arg]
    rest = iou.copy()
    rest[np.arange(len(arg)), arg] = -1.0
    second = rest.max(1) if n > 1 else np.full(len(arg), -1.0)
    none = best < 0
    return np.where(none, 0.0, best), np.where(none, 0, arg), np.where(none, -1.0, second)


def py_mod(a, m):
    return np.mod(a, m)


def targets(rois, scores, labels, gt, u_fg, u_slot, cfg):
    """everything df3d_roi_targets returns, per the sampling definition of DESIGN section 7.14, and the margins"""
    rois, gt = np.asarray(rois, np.float64), np.asarray(gt, np.float64)
    nB, R = rois.shape[:2]
    m = cfg["ROI_PER_IMAGE"]
    reg_fg, cls_fg, cls_bg, lo = cfg["REG_FG_THRESH"], cfg["CLS_FG_THRESH"], cfg["CLS_BG_THRESH"], cfg["CLS_BG_THRESH_LO"]
    fg_per_image = int(np.round(cfg["FG_RATIO"] * m))
    out = dict(inds=np.zeros((nB, m), np.int64), counts=np.zeros((nB, 3), np.int64), ious_all=np.zeros((nB, R)),
               asg_all=np.zeros((nB, R), np.int64), thresh_dist=np.inf, gap=np.inf)
    for b in range(nB):
        iou, asg, second = max_overlaps(rois[b], labels[b], gt[b], cfg["SAMPLE_ROI_BY_EACH_CLASS"])
        out["ious_all"][b], out["asg_all"][b] = iou, asg
        out["thresh_dist"] = min(out["thresh_dist"], min(np.abs(iou - t).min() for t in (reg_fg, cls_fg, cls_bg, lo)))
        contested = (second >= 0) & ~((iou == 0) & (second == 0))
        if contested.any():
            out["gap"] = min(out["gap"], float((iou - second)[contested].min()))
        fg = np.nonzero(iou >= min(reg_fg, cls_fg))[0]
        easy = np.nonzero(iou < lo)[0]
        hard = np.nonzero((iou < reg_fg) & (iou >= lo))[0]
        out["counts"][b] = (len(fg), len(hard), len(easy))
        u = u_slot[b].astype(np.float64)
        pick = lambda lst, s: lst[np.floor(u[s] * len(lst)).astype(np.int64)]

        def background(F):
            s = np.arange(F, m)
            if len(hard) and len(easy):
                k = min(int((m - F) * cfg["HARD_BG_RATIO"]), len(hard))
                return np.concatenate([pick(hard, s[:k]), pick(easy, s[k:])])
            return pick(hard if len(hard) else easy, s)

        if len(fg) and (len(hard) or len(easy)):
            F = min(fg_per_image, len(fg))
            order = np.argsort(u_fg[b, :len(fg)], kind="stable")
            sel = np.concatenate([fg[order[:F]], background(F)])
        elif len(fg):
            sel = pick(fg, np.arange(m))
        else:
            sel = background(0)
        out["inds"][b] = sel
    bi = np.arange(nB)[:, None]
    s_rois, s_iou = rois[bi, out["inds"]], out["ious_all"][bi, out["inds"]]
    src = gt[bi, out["asg_all"][bi, out["inds"]]]
    out.update(rois=s_rois, roi_labels=labels[bi, out["inds"]], roi_scores=np.asarray(scores, np.float64)[bi, out["inds"]],
               gt_iou_of_rois=s_iou, gt_of_rois_src=src, reg_valid_mask=(s_iou > reg_fg).astype(np.int64))
    hardl = (s_iou > cls_fg).astype(np.float64)
    hardl[(s_iou > cls_bg) & (s_iou < cls_fg)] = -1
    soft = np.where(s_iou > cls_fg, 1.0, np.where(s_iou < cls_bg, 0.0, (s_iou - cls_bg) / (cls_fg - cls_bg)))
    out["cls_labels_cls"], out["cls_labels_roi_iou"] = hardl, soft
    out["rcnn_cls_labels"] = hardl if cfg["CLS_SCORE_TYPE"] == "cls" else soft
    # canonical transform (roi_head_template.py:113-132)
    can = src.copy()
    roi_ry = py_mod(s_rois[..., 6], TWO_PI)
    x, y = src[..., 0] - s_rois[..., 0], src[..., 1] - s_rois[..., 1]
    c, s = np.cos(-roi_ry), np.sin(-roi_ry)
    can[..., 0], can[..., 1], can[..., 2] = x * c - y * s, x * s + y * c, src[..., 2] - s_rois[..., 2]
    h = py_mod(src[..., 6] - roi_ry, TWO_PI)
    dist = np.minimum(np.minimum(np.abs(h - np.pi / 2), np.abs(h - np.pi)), np.abs(h - 1.5 * np.pi))
    opposite = (h > np.pi * 0.5) & (h < np.pi * 1.5)
    h = np.where(opposite, py_mod(h + np.pi, TWO_PI), h)
    dist = np.minimum(dist, np.abs(h - np.pi))
    h = np.where(h > np.pi, h - TWO_PI, h)
    can[..., 6] = np.clip(h, -np.pi / 2, np.pi / 2)
    out["gt_of_rois"] = can
    real = np.abs(src[..., :7]).sum(-1) > 0                           # (the heading of an all-zero row decides nothing)
    out["heading_dist"] = float(dist[real].min()) if real.any() else np.inf
    out["fold_branches"] = {bool(v) for v in opposite[real]}
    return out


def targets_clean(t):
    return t["thresh_dist"] >= THRESH_MARGIN and t["gap"] >= GAP_MARGIN and t["heading_dist"] >= HEADING_MARGIN


def keys_distinct(u_fg):
    return all(len(np.unique(row)) == len(row) for row in u_fg)


# ---------------------------------------------------------------------------------------------------- losses
def _corners3d(box):
    """boxes_to_corners_3d: [n, 7] -> [n, 8, 3]"""
    tmpl = np.array([[1, 1, -1], [1, -1, -1], [-1, -1, -1], [-1, 1, -1], [1, 1, 1], [1, -1, 1], [-1, -1, 1], [-1, 1, 1]]) / 2.0
    loc = box[:, None, 3:6] * tmpl[None]
    c, s = np.cos(box[:, 6])[:, None], np.sin(box[:, 6])[:, None]
    return np.stack([loc[..., 0] * c - loc[..., 1] * s, loc[..., 0] * s + loc[..., 1] * c, loc[..., 2]], -1) + box[:, None, 0:3]


def losses(rcnn_cls, rcnn_reg, rois, gt_of_rois, gt_of_rois_src, reg_valid_mask, rcnn_cls_labels, loss_cfg=LOSS_CFG,
           upstream=(1.0, 1.0, 1.0)):
    """-> loss [3] (cls, reg, corner), grad_cls [N, 1], grad_reg [N, 7] of sum_j upstream[j] * loss[j], and the margins"""
    w = loss_cfg["LOSS_WEIGHTS"]
    cw = np.asarray(w["code_weights"], np.float64)
    x = np.asarray(rcnn_cls, np.float64).reshape(-1)
    p = np.asarray(rcnn_reg, np.float64).reshape(-1, 7)
    N = x.shape[0]
    r = np.asarray(rois, np.float64).reshape(N, 7)
    g = np.asarray(gt_of_rois, np.float64).reshape(N, -1)[:, :7]
    s = np.asarray(gt_of_rois_src, np.float64).reshape(N, -1)[:, :7]
    fg = np.asarray(reg_valid_mask).reshape(N) > 0
    t = np.asarray(rcnn_cls_labels, np.float64).reshape(N)
    out = {}
    # classification
    cared = t >= 0
    valid = max(float(cared.sum()), 1.0)
    bce = np.maximum(x, 0) - x * t + np.log1p(np.exp(-np.abs(x)))
    l_cls = (bce * cared).sum() / valid * w["rcnn_cls_weight"]
    g_cls = (1 / (1 + np.exp(-x)) - t) * cared / valid * w["rcnn_cls_weight"] * upstream[0]
    # regression
    fg_sum = float(fg.sum())
    da = np.maximum(r[:, 3:6], 1e-5)
    diag = np.hypot(da[:, 0], da[:, 1])
    gd = np.maximum(g[:, 3:6], 1e-5)
    tg = np.concatenate([g[:, 0:2] / diag[:, None], g[:, 2:3] / da[:, 2:3], np.log(gd / da), g[:, 6:7]], 1)
    d = (p - tg) * cw
    n = np.abs(d)
    l_reg = (np.where(n < BETA, 0.5 * n * n / BETA, n - 0.5 * BETA) * fg[:, None]).sum() / max(fg_sum, 1.0) * w["rcnn_reg_weight"]
    g_reg = np.where(n < BETA, d / BETA, np.sign(d)) * cw * fg[:, None] / max(fg_sum, 1.0) * w["rcnn_reg_weight"] * upstream[1]
    out["beta_dist"] = float(np.abs(n[fg] - BETA).min()) if fg.any() else np.inf
    out["reg_branches"] = {bool(v) for v in (n[fg] < BETA).reshape(-1)}
    # corners
    l_corner, out["corner_dist"], out["flip_gap"], out["huber_branches"] = 0.0, np.inf, np.inf, set()
    if loss_cfg["CORNER_LOSS_REGULARIZATION"] and fg_sum > 0:
        rr, pp, ss = r[fg], p[fg], s[fg]
        diag_raw = np.hypot(rr[:, 3], rr[:, 4])
        xyz = np.stack([pp[:, 0] * diag_raw, pp[:, 1] * diag_raw, pp[:, 2] * rr[:, 5]], 1)
        dims = np.exp(pp[:, 3:6]) * rr[:, 3:6]
        heading = pp[:, 6] + rr[:, 6]
        c0, s0 = np.cos(rr[:, 6]), np.sin(rr[:, 6])
        ctr = np.stack([xyz[:, 0] * c0 - xyz[:, 1] * s0, xyz[:, 0] * s0 + xyz[:, 1] * c0, xyz[:, 2]], 1) + rr[:, 0:3]
        pred = _corners3d(np.concatenate([ctr, dims, heading[:, None]], 1))
        flip = ss.copy()
        flip[:, 6] += np.pi
        e1, e2 = pred - _corners3d(ss), pred - _corners3d(flip)
        d1, d2 = np.linalg.norm(e1, axis=2), np.linalg.norm(e2, axis=2)
        direct = d1 <= d2
        dist, e = np.where(direct, d1, d2), np.where(direct[..., None], e1, e2)
        k = w["rcnn_corner_weight"] / (8.0 * fg_sum)
        l_corner = np.where(dist < 1, 0.5 * dist * dist, dist - 0.5).sum() * k
        out["corner_dist"], out["flip_gap"] = float(np.abs(dist - 1).min()), float(np.abs(d1 - d2).min())
        out["huber_branches"] = {bool(v) for v in (dist < 1).reshape(-1)}
        gp = np.where(dist[..., None] > 0, np.where(dist < 1, dist, 1.0)[..., None] * e / np.where(dist > 0, dist, 1.0)[..., None], 0.0)
        tmpl = np.array([[1, 1, -1], [1, -1, -1], [-1, -1, -1], [-1, 1, -1], [1, 1, 1], [1, -1, 1], [-1, -1, 1], [-1, 1, 1]]) / 2.0
        cr, sr = np.cos(heading)[:, None], np.sin(heading)[:, None]
        pa, pb = tmpl[None, :, 0] * dims[:, 0:1], tmpl[None, :, 1] * dims[:, 1:2]
        g_ctr = gp.sum(1)
        g_dx = ((gp[..., 0] * cr + gp[..., 1] * sr) * tmpl[None, :, 0]).sum(1)
        g_dy = ((-gp[..., 0] * sr + gp[..., 1] * cr) * tmpl[None, :, 1]).sum(1)
        g_dz = (gp[..., 2] * tmpl[None, :, 2]).sum(1)
        g_h = (gp[..., 0] * (-pa * sr - pb * cr) + gp[..., 1] * (pa * cr - pb * sr)).sum(1)
        gc = np.stack([(g_ctr[:, 0] * c0 + g_ctr[:, 1] * s0) * diag_raw, (-g_ctr[:, 0] * s0 + g_ctr[:, 1] * c0) * diag_raw,
                       g_ctr[:, 2] * rr[:, 5], g_dx * dims[:, 0], g_dy * dims[:, 1], g_dz * dims[:, 2], g_h], 1)
        g_reg[fg] += gc * k * upstream[2]
    out.update(loss=np.array([l_cls, l_reg, l_corner]), grad_cls=g_cls.reshape(N, 1), grad_reg=g_reg, logit_max=float(np.abs(x).max()))
    return out


def loss_clean(l):
    return (l["beta_dist"] >= BETA_MARGIN and l["corner_dist"] >= BETA_MARGIN and l["flip_gap"] >= GAP_MARGIN and
            l["logit_max"] <= LOGIT_MAX)


# ---------------------------------------------------------------------------------------------------- seeded inputs
def _draw_boxes(rs, n, classes):
    cls = rs.choice(classes, n)
    out = np.zeros((n, 8))
    out[:, 0], out[:, 1] = rs.uniform(RANGE[0] + 5, RANGE[2] - 5, n), rs.uniform(RANGE[1] + 5, RANGE[3] - 5, n)
    out[:, 3:6] = SIZES[cls - 1] * rs.uniform(0.8, 1.25, (n, 3))
    out[:, 2] = -1.0 + rs.uniform(-0.2, 0.2, n)
    out[:, 6] = rs.uniform(-np.pi, np.pi, n)
    out[:, 7] = cls
    return out


def _band(v, lo, hi, thresholds):
    return (v >= lo) & (v <= hi) & np.all(np.abs(v[:, None] - np.asarray(thresholds)[None]) > 10 * THRESH_MARGIN, axis=1)


def make_frame(rs, R, plan, by_class, frame):
    """ground truth [G, 8] and R RoIs whose best overlaps fall into the three bands as `plan` = (n_fg, n_hard, n_easy) asks:
    a pool of candidates around the ground truth (small, medium and large perturbations, a third of them turned by pi, a few
    of a class the frame has no box of) is drawn, rated in float64 and the first of each band taken, then interleaved"""
    thresholds = [SAMPLER[k] for k in ("REG_FG_THRESH", "CLS_FG_THRESH", "CLS_BG_THRESH", "CLS_BG_THRESH_LO")]
    gt = np.zeros((G, 8))
    if plan[0] + plan[1] > 0:
        classes = [1, 2] if frame == 1 else [1, 2, 3]               # frame 1: no ground truth of class 3, row 0 of class 1
        boxes = _draw_boxes(rs, 5, classes)
        if frame == 1:
            boxes[0, 7], boxes[0, 3:6] = 1, SIZES[0]
        gt[0:2], gt[3:6] = boxes[0:2], boxes[2:5]                   # row 2: an interior all-zero row; rows 6, 7: trailing
    real = gt[np.abs(gt).sum(1) > 0]
    want = dict(fg=plan[0], hard=plan[1], easy=plan[2])
    picked = {k: [] for k in want}
    for _ in range(40):
        n = 4 * R
        if len(real):
            src = real[rs.randint(0, len(real), n)]
            scale = rs.choice([0.03, 0.12, 0.3, 3.0], n)[:, None]
            cand = src[:, :7].copy()
            cand[:, 0:3] += rs.normal(0, 1, (n, 3)) * scale * src[:, 3:6] * [1.0, 1.0, 0.5]
            cand[:, 3:6] *= np.exp(rs.normal(0, 1, (n, 3)) * np.minimum(scale, 0.3) * 0.5)
            cand[:, 6] += rs.normal(0, 1, n) * np.minimum(scale[:, 0], 0.5) + np.pi * (rs.uniform(0, 1, n) < 0.33)
            lab = src[:, 7].astype(np.int64)
            if by_class and frame == 1:
                lab = np.where(rs.uniform(0, 1, n) < 0.1, 3, lab)
        else:
            drawn = _draw_boxes(rs, n, [1, 2, 3])
            cand, lab = drawn[:, :7], drawn[:, 7].astype(np.int64)
        cand = cand.astype(np.float32).astype(np.float64)
        best, _, second = max_overlaps(cand, lab, gt.astype(np.float32).astype(np.float64), by_class)
        apart = (second < 0) | ((best == 0) & (second == 0)) | (best - second > 10 * GAP_MARGIN)
        bands = dict(fg=_band(best, 0.6, 1.0, thresholds), hard=_band(best, 0.12, 0.5, thresholds), easy=best < 0.05)
        for k in want:
            for i in np.nonzero(bands[k] & apart)[0]:
                if len(picked[k]) < want[k]:
                    picked[k].append((cand[i], lab[i]))
        if all(len(picked[k]) == want[k] for k in want):
            break
    else:
        raise AssertionError("frame %d: the candidate pool does not fill the plan %s" % (frame, plan))
    rows = picked["fg"] + picked["hard"] + picked["easy"]
    perm = rs.permutation(R)
    rois = np.stack([rows[i][0] for i in perm])
    labels = np.array([rows[i][1] for i in perm], np.int64)
    return gt, rois, labels


def make_inputs(name, seed, R=None, m=M, plans=None):
    """-> rois, roi_scores, roi_labels, gt_boxes, u_fg, u_slot of a case"""
    c = CASES[name]
    R = c["R"] if R is None else R
    plans = frame_plan(R) if plans is None else plans
    rs = np.random.RandomState(seed)
    frames = [make_frame(rs, R, plan, c["by_class"], f) for f, plan in enumerate(plans)]
    gt = np.stack([f[0] for f in frames]).astype(np.float32)
    rois = np.stack([f[1] for f in frames]).astype(np.float32)
    labels = np.stack([f[2] for f in frames])
    scores = rs.normal(0, 2, labels.shape).astype(np.float32)
    # distinct keys by construction: a permutation of the R cells of [0, 1) and a place inside the cell
    u_fg = ((np.stack([rs.permutation(R) for _ in plans]) + rs.uniform(0.25, 0.75, labels.shape)) / R).astype(np.float32)
    u_slot = rs.uniform(0, 1, (len(plans), m)).astype(np.float32)
    return rois, scores, labels, gt, np.minimum(u_fg, np.float32(1 - 2.0 ** -24)), np.minimum(u_slot, np.float32(1 - 2.0 ** -24))


def make_preds(seed, n):
    """rcnn_cls [n, 1] (|logit| <= 8) and rcnn_reg [n, 7]: rows alternate between small and large residuals, so that both
    branches of the smooth-L1 and of the corner Huber loss occur"""
    rs = np.random.RandomState(seed + 7919)
    cls = np.clip(rs.normal(0, 2.5, (n, 1)), -LOGIT_MAX, LOGIT_MAX).astype(np.float32)
    scale = np.where(np.arange(n) % 2 == 0, 0.03, 0.35)[:, None]
    return cls, (rs.normal(0, 1, (n, 7)) * scale).astype(np.float32)


def restate(name, g):
    """(targets, losses) of a case of the fixture from its stored inputs"""
    t = targets(g[name + "_rois"], g[name + "_roi_scores"], g[name + "_roi_labels"], g[name + "_gt"], g[name + "_u_fg"], g[name + "_u_slot"],
                sampler_cfg(name))
    l = losses(g[name + "_rcnn_cls"], g[name + "_rcnn_reg"], t["rois"], t["gt_of_rois"], t["gt_of_rois_src"], t["reg_valid_mask"],
               t["rcnn_cls_labels"])
    return t, l


def coverage(name, g, t, l):
    """which of the conditions of the issue a case of the fixture covers"""
    fgpi = int(np.round(SAMPLER["FG_RATIO"] * M))
    cnt, gt = t["counts"], g[name + "_gt"]
    zero = np.abs(gt).sum(-1) == 0
    cov = dict(
        more_fg=bool(((cnt[:, 0] > fgpi) & (cnt[:, 1] > 0) & (cnt[:, 2] > 0)).any()),
        fewer_fg=bool(((cnt[:, 0] > 0) & (cnt[:, 0] < fgpi) & (cnt[:, 1] + cnt[:, 2] > 0)).any()),
        hard_only=bool(((cnt[:, 1] > 0) & (cnt[:, 2] == 0)).any()), easy_only=bool(((cnt[:, 1] == 0) & (cnt[:, 2] > 0) & (cnt[:, 0] > 0)).any()),
        fg_only=bool(((cnt[:, 0] > 0) & (cnt[:, 1] + cnt[:, 2] == 0)).any()), empty_frame=bool(zero.all(1).any()),
        interior_zero=any(zero[b, :valid_count(gt[b])].any() and not zero[b].all() for b in range(gt.shape[0])),
        fold=t["fold_branches"], huber=l["huber_branches"], reg=l["reg_branches"], unserved=False)
    if CASES[name]["by_class"]:
        labels = g[name + "_roi_labels"]
        for b in range(gt.shape[0]):
            present = set(gt[b, :valid_count(gt[b]), 7].astype(int))
            if not zero[b, 0] and any(int(v) not in present and int(v) != int(gt[b, 0, 7]) for v in labels[b]):
                cov["unserved"] = True
    return cov
