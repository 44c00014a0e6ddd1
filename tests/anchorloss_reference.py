"""Float64 numpy restatement of the Voxel-RCNN first-stage training path (AxisAlignedTargetAssigner and the RPN losses with
their analytic gradients), written from the formulas of DESIGN section 7.13, the case table of the fixture
tests/golden/anchor_loss.npz and the margin predicates that make a label mismatch a bug and not rounding.  Test
infrastructure: never imported by the package.

Shapes: anchors [N, 7] with N = H*W*A and anchor i = (y*W + x)*A + a; gt [B, M, 8] = (x, y, z, dx, dy, dz, heading, class);
cls [B, N, C], box [B, N, 7], dir [B, N, NB] or None."""
import numpy as np

import vrtail_reference as vt

FLOOR_MARGIN = vt.FLOOR_MARGIN      # direction-bin quotient from an integer
THRESH_MARGIN = 1e-4                # anchor-max IoU from a matched / unmatched threshold
GAP_MARGIN = 1e-6                   # best and second-best IoU where the order decides something: ~10 float32 roundings of an IoU <= 1
BETA_MARGIN = 1e-4                  # |code-weighted diff| from the smooth-L1 change point
BETA = 1.0 / 9.0
LOSS_WEIGHTS = {"cls_weight": 1.0, "loc_weight": 2.0, "dir_weight": 0.2, "code_weights": [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]}

# per case of vrtail_reference.CASES: the class names of the data set (one more than the anchor sets serve, where a GT class
# without anchors is wanted) and the number of ground-truth boxes of a full frame; M = num_gt + 3 all-zero rows
TRAIN = {
    "car": dict(class_names=["Car", "Van"], num_gt=12),
    "small": dict(class_names=["Car"], num_gt=3),
    "multi": dict(class_names=["Car", "Pedestrian", "Cyclist"], num_gt=9),
    "nodir": dict(class_names=["Car", "Van"], num_gt=12),
}


def source(name):
    """'nodir' shares the arrays of 'car'"""
    return "car" if name == "nodir" else name


def train_head_cfg(name):
    """the AnchorHeadSingle config of a case with the training keys (plain dicts)"""
    cfg = vt.head_cfg(name)
    cfg["TARGET_ASSIGNER_CONFIG"] = {"NAME": "AxisAlignedTargetAssigner", "POS_FRACTION": -1.0, "SAMPLE_SIZE": 512,
                                     "NORM_BY_NUM_EXAMPLES": False, "MATCH_HEIGHT": False, "BOX_CODER": "ResidualCoder"}
    cfg["LOSS_CONFIG"] = {"LOSS_WEIGHTS": dict(LOSS_WEIGHTS)}
    return cfg


def set_params(name):
    """-> per anchor set: 1-based class id, matched, unmatched"""
    sets, names = vt.CASES[name]["sets"], TRAIN[name]["class_names"]
    return ([names.index(s["class_name"]) + 1 for s in sets], [s["matched_threshold"] for s in sets],
            [s["unmatched_threshold"] for s in sets])


def anchor_sets(name):
    """set of every anchor slot a (two rotations per set)"""
    return [s for s in range(len(vt.CASES[name]["sets"])) for _ in range(2)]


def make_gt(name, seed):
    """The seeded ground truth of a case: sizes = the set's anchor size x U(0.8, 1.25), centres uniform in the range,
    headings uniform in (-pi, pi).  Frame 0: num_gt boxes with an all-zero row in their middle and two at the end; with
    B = 3, frame 1 fills all M rows, one of them wholly outside the range, one of a class no anchor set serves and one
    whose centre lies 2.5 m past the range (only the border anchors reach it, below the unmatched threshold: matched
    through the forced rule alone); the last frame is empty."""
    c, tr = vt.CASES[name], TRAIN[name]
    _, rng = vt.case_geometry(name)
    rs = np.random.RandomState(seed)
    n, names = tr["num_gt"], tr["class_names"]
    M = n + 3

    def boxes(count):
        out = np.zeros((count, 8))
        for i in range(count):
            s = c["sets"][i % len(c["sets"])]
            size = np.asarray(s["anchor_sizes"][0]) * rs.uniform(0.8, 1.25, 3)
            z = s["anchor_bottom_heights"][0] + size[2] / 2 + rs.uniform(-0.2, 0.2)
            out[i] = [rs.uniform(rng[0], rng[3]), rs.uniform(rng[1], rng[4]), z, size[0], size[1], size[2], rs.uniform(-np.pi, np.pi),
                      names.index(s["class_name"]) + 1]
        return out

    gt = np.zeros((c["B"], M, 8))
    first = boxes(n)
    gt[0, :n // 2] = first[:n // 2]
    gt[0, n // 2 + 1:n + 1] = first[n // 2:]
    if c["B"] > 2:
        full = boxes(M)
        full[1, 0] = rng[3] + 20.0                                 # wholly outside the range
        if len(names) > len(c["sets"]):
            full[2, 7] = len(names)                                # a class without anchors
        full[3, 0] = rng[3] + 2.5                                  # reached by the border anchors only
        gt[1] = full
    return gt.astype(np.float32)


def make_preds(name, seed):
    """seeded head maps: logits ~ 2 N(0, 1), residuals 0.3 N(0, 1) (both branches of the smooth L1), direction logits N(0, 1)"""
    c = vt.CASES[name]
    rs = np.random.RandomState(10000 + seed)
    per = c["H"] * c["W"] * 2 * len(c["sets"])
    return ((2 * rs.standard_normal((c["B"], per, c["C"]))).astype(np.float32),
            (0.3 * rs.standard_normal((c["B"], per, 7))).astype(np.float32), rs.standard_normal((c["B"], per, 2)).astype(np.float32))


# ---- assignment -----------------------------------------------------------------------------------------------------------
def aligned_bev(b):
    b = np.asarray(b, np.float64)
    rot = np.abs(b[:, 6] - np.floor(b[:, 6] / np.pi + 0.5) * np.pi)
    keep = (rot < np.pi / 4)[:, None]
    dims = np.where(keep, b[:, [3, 4]], b[:, [4, 3]])
    return np.concatenate([b[:, 0:2] - dims / 2, b[:, 0:2] + dims / 2], 1)


def nearest_bev_iou(a, g):
    """[N, 7], [G, 7] -> [N, G]"""
    a, g = aligned_bev(a), aligned_bev(g)
    x_len = np.maximum(np.minimum(a[:, None, 2], g[None, :, 2]) - np.maximum(a[:, None, 0], g[None, :, 0]), 0)
    y_len = np.maximum(np.minimum(a[:, None, 3], g[None, :, 3]) - np.maximum(a[:, None, 1], g[None, :, 1]), 0)
    inter = x_len * y_len
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_g = (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1])
    return inter / np.maximum(area_a[:, None] + area_g[None, :] - inter, 1e-6)


def residual_encode(g, a):
    """g, a [n, 7] -> targets [n, 7]"""
    g, a = np.asarray(g, np.float64), np.asarray(a, np.float64)
    ad, gd = np.maximum(a[:, 3:6], 1e-5), np.maximum(g[:, 3:6], 1e-5)
    diag = np.sqrt(ad[:, 0] ** 2 + ad[:, 1] ** 2)
    return np.stack([(g[:, 0] - a[:, 0]) / diag, (g[:, 1] - a[:, 1]) / diag, (g[:, 2] - a[:, 2]) / ad[:, 2], np.log(gd[:, 0] / ad[:, 0]),
                     np.log(gd[:, 1] / ad[:, 1]), np.log(gd[:, 2] / ad[:, 2]), g[:, 6] - a[:, 6]], 1)


def valid_count(gt_frame):
    """index of the last row whose seven box values sum to non-zero in float32, plus one; at least 1"""
    s = np.asarray(gt_frame, np.float32)[:, :7]
    acc = s[:, 0].copy()
    for e in range(1, 7):
        acc = (acc + s[:, e]).astype(np.float32)
    nz = np.nonzero(acc != 0)[0]
    return int(nz[-1]) + 1 if len(nz) else 1


def _second(v, axis):
    """second largest along an axis (-inf where there is one entry)"""
    if v.shape[axis] < 2:
        return np.full(np.delete(v.shape, axis), -np.inf)
    return np.sort(v, axis=axis).take(-2, axis=axis)


def assign(anchors, anchor_set, A, gt, set_class, matched, unmatched):
    """-> dict: labels, gt_ids [B, N] int32, num_pos [B], targets [B, N, 7], weights [B, N] float64, and the margins and
    coverage counts: thresh_dist, argmax_ties (anchors whose two best IoUs > 0 are equal), positive_gap (best - second of
    the positives), gt_gap_bad (GTs whose best and second-best anchor IoU are neither equal nor GAP_MARGIN apart),
    forced_only (GTs matched through the forced rule alone), forced_below (forced anchors below the unmatched threshold),
    ignored, unmatched_gt (GTs of a served class whose max IoU is 0)."""
    anchors = np.asarray(anchors, np.float64)
    N, B = anchors.shape[0], gt.shape[0]
    slot = np.arange(N) % A
    set_of = np.asarray(anchor_set)[slot]
    res = dict(labels=-np.ones((B, N), np.int32), gt_ids=-np.ones((B, N), np.int32), targets=np.zeros((B, N, 7)),
               weights=np.zeros((B, N)), thresh_dist=np.inf, argmax_ties=0, positive_gap=np.inf, gt_gap_bad=0, forced_only=0,
               forced_below=0, ignored=0, unmatched_gt=0)
    for b in range(B):
        n = valid_count(gt[b])
        cls = gt[b, :n, 7].astype(np.int32)
        for s in range(len(set_class)):
            idx = np.nonzero(set_of == s)[0]
            rows = np.nonzero(cls == set_class[s])[0]
            if len(rows) == 0:
                res["labels"][b, idx] = 0
                continue
            iou = nearest_bev_iou(anchors[idx], gt[b, rows, :7])
            arg = iou.argmax(1)
            best = iou[np.arange(len(idx)), arg]
            second = _second(iou, 1)
            gmax = iou.max(0)
            gsecond = _second(iou, 0)
            res["unmatched_gt"] += int((gmax == 0).sum())
            res["gt_gap_bad"] += int(((gmax > 0) & (gsecond != gmax) & (gmax - gsecond < GAP_MARGIN)).sum())
            forced = ((iou == np.where(gmax == 0, -1.0, gmax)[None]).any(1))
            pos = best >= matched[s]
            lab = -np.ones(len(idx), np.int32)
            ids = -np.ones(len(idx), np.int32)
            take = forced | pos
            lab[take] = cls[rows[arg[take]]]
            ids[take] = rows[arg[take]]
            lab[(best < unmatched[s]) & ~forced] = 0
            res["labels"][b, idx], res["gt_ids"][b, idx] = lab, ids
            res["thresh_dist"] = min(res["thresh_dist"], float(np.abs(best - matched[s]).min()), float(np.abs(best - unmatched[s]).min()))
            res["argmax_ties"] += int(((best > 0) & (second == best)).sum())
            fg = lab > 0
            if fg.any():
                res["positive_gap"] = min(res["positive_gap"], float((best - second)[fg].min()))
                res["targets"][b, idx[fg]] = residual_encode(gt[b, rows[arg[fg]], :7], anchors[idx[fg]])
                res["weights"][b, idx[fg]] = 1.0
            res["forced_below"] += int((forced & (best < unmatched[s])).sum())
            for k in range(len(rows)):                              # GTs no anchor reaches by the threshold, yet matched
                mine = fg & (arg == k)
                if gmax[k] > 0 and mine.any() and not (pos & mine).any():
                    res["forced_only"] += 1
        res["ignored"] += int((res["labels"][b] == -1).sum())
    res["num_pos"] = (res["labels"] > 0).sum(1).astype(np.int32)
    return res


def assign_clean(r):
    return (r["thresh_dist"] >= THRESH_MARGIN and r["argmax_ties"] == 0 and r["positive_gap"] >= GAP_MARGIN and r["gt_gap_bad"] == 0)


# ---- losses ---------------------------------------------------------------------------------------------------------------
def losses(cls, box, dirs, anchors, labels, targets, num_classes, dir_offset=vt.DIR_OFFSET, weights=LOSS_WEIGHTS, beta=BETA,
           upstream=(1.0, 1.0, 1.0)):
    """-> dict: loss [3] (cls, loc, dir), grad_cls, grad_box, grad_dir (of sum_j upstream[j] * loss[j]; grad_dir None without
    direction classifier), and the margins floor_dist, beta_dist, bins (the direction bins the positives hit)."""
    cls, box = np.asarray(cls, np.float64), np.asarray(box, np.float64)
    anchors = np.asarray(anchors, np.float64)
    B, N, C = cls.shape
    pos = labels > 0
    w = 1.0 / np.maximum(pos.sum(1, keepdims=True), 1.0)                               # [B, 1]
    # classification
    lab = np.where(pos, 1, labels) if num_classes == 1 else labels
    tt = (lab[..., None] == np.arange(1, C + 1)[None, None]).astype(np.float64)
    cared = (labels >= 0)[..., None] * w[..., None]
    p = 1.0 / (1.0 + np.exp(-cls))
    alpha_w = tt * 0.25 + (1 - tt) * 0.75
    pt = tt * (1 - p) + (1 - tt) * p
    bce = np.maximum(cls, 0) - cls * tt + np.log1p(np.exp(-np.abs(cls)))
    l_cls = (alpha_w * pt ** 2 * bce * cared).sum() / B * weights["cls_weight"]
    dpt = (1 - 2 * tt) * p * (1 - p)
    g_cls = alpha_w * (2 * pt * dpt * bce + pt ** 2 * (p - tt)) * cared / B * weights["cls_weight"] * upstream[0]
    # regression
    cw = np.asarray(weights["code_weights"], np.float64)
    tg = np.asarray(targets, np.float64)
    d = (box - tg) * cw
    d[..., 6] = cw[6] * (np.sin(box[..., 6]) * np.cos(tg[..., 6]) - np.cos(box[..., 6]) * np.sin(tg[..., 6]))
    dd = np.broadcast_to(cw, d.shape).copy()
    dd[..., 6] = cw[6] * (np.cos(box[..., 6]) * np.cos(tg[..., 6]) + np.sin(box[..., 6]) * np.sin(tg[..., 6]))
    n = np.abs(d)
    regw = (pos * w)[..., None]
    l_loc = (np.where(n < beta, 0.5 * n ** 2 / beta, n - 0.5 * beta) * regw).sum() / B * weights["loc_weight"]
    g_box = np.where(n < beta, d / beta, np.sign(d)) * dd * regw / B * weights["loc_weight"] * upstream[1]
    res = dict(grad_cls=g_cls, grad_box=g_box, grad_dir=None, floor_dist=np.inf, bins=set(),
               beta_dist=float(np.abs(n - beta)[pos].min()) if pos.any() else np.inf)
    l_dir = 0.0
    if dirs is not None:
        dirs = np.asarray(dirs, np.float64)
        NB = dirs.shape[-1]
        v = tg[..., 6] + anchors[None, :, 6] - dir_offset
        offset_rot = v - np.floor(v / (2 * np.pi)) * (2 * np.pi)
        q = offset_rot / (2 * np.pi / NB)
        bins = np.clip(np.floor(q), 0, NB - 1).astype(np.int64)
        if pos.any():
            res["floor_dist"] = float(np.abs(q - np.round(q))[pos].min())
            res["bins"] = set(bins[pos].tolist())
        mx = dirs.max(-1, keepdims=True)
        e = np.exp(dirs - mx)
        soft = e / e.sum(-1, keepdims=True)
        ce = (mx[..., 0] + np.log(e.sum(-1))) - np.take_along_axis(dirs, bins[..., None], -1)[..., 0]
        l_dir = (ce * pos * w).sum() / B * weights["dir_weight"]
        onehot = (bins[..., None] == np.arange(NB)[None, None]).astype(np.float64)
        res["grad_dir"] = (soft - onehot) * regw / B * weights["dir_weight"] * upstream[2]
    res["loss"] = np.array([l_cls, l_loc, l_dir])
    return res


def loss_clean(r, with_dir):
    return r["beta_dist"] >= BETA_MARGIN and (not with_dir or r["floor_dist"] >= FLOOR_MARGIN)


def restate(name, g):
    """assignment and losses of a case on the arrays of the fixture -> (assign dict, losses dict)"""
    c, src = vt.CASES[name], source(name)
    anchors = g[src + "_anchors"].reshape(-1, 7)
    sc, matched, unmatched = set_params(name)
    a = assign(anchors, anchor_sets(name), 2 * len(c["sets"]), g[src + "_gt"], sc, matched, unmatched)
    l = losses(g[src + "_cls"], g[src + "_box"], g[src + "_dir"] if c["NB"] else None, anchors, a["labels"], a["targets"], c["C"])
    return a, l
