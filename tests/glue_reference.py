"""Host reference of the camera-fusion glue (include/df3d_hip.h, "Camera-fusion glue of the CenterPoint adapter" down to
df3d_assemble_queries2_compact): one plain numpy function per ABI contract, written from the contract text and not from the
kernels.  Floating results are evaluated in float64; `fp32=True` evaluates the same formula in numpy float32, which is the
yardstick of what plain fp32 arithmetic makes of it (a kernel may sit at four times the yardstick's largest error plus 1e-6
of the tensor's scale: `assert_within_yardstick`).  Integers and copies are exact.

Conventions of the ABI: indices [n, 4] i32 (b, z, y, x), batch-sorted; grid [ncam, n, 2] i32 (x, y) on the feature map;
mask [ncam, n] u8; pos [ncam, n] i32; image index = b * ncam + cam."""
import numpy as np

MARGIN = 64.0 * 2.0 ** -23      # 64 ulp: an fp32 chain of three 4-term dot products, a 3-term one and a division


def _dt(fp32):
    return np.float32 if fp32 else np.float64


# ------------------------------------------------------------------------------------------------------- projection
def project(indices, batch, ncam, scale_xyz, pc_min, lidar2cam, intrinsic, raw_hw, depth_thres, image_scale, feat_scale,
            aug_inv=None, fp32=False):
    """df3d_project_voxels.  Corner, optional augmentation (+ translate, then the row vector times rescale / rotate / flip),
    lidar2cam, intrinsic and the division in float64 (float32 with fp32=True); the two later truncations
    long(image_scale * float(g)) and int(float(g) * feat_scale) in fp32 as the contract has them -- each is one fp32 multiply
    of exact integers, so numpy's float32 reproduces it bit for bit.
    -> grid [ncam, n, 2] i32, mask [ncam, n] u8, point_inv [n, 3], depth [ncam, n] (0 where masked), decided [ncam, n] bool.
    decided: u, v are further than 64 ulp (of max(1, |.|)) from the nearest integer and cz is further than that from the
    depth threshold -- the pairs on which an fp32 evaluation in any order must give the same integers."""
    dt = _dt(fp32)
    ind = np.asarray(indices).reshape(-1, 4)
    n = len(ind)
    b = ind[:, 0].astype(np.int64)
    scale = np.asarray(scale_xyz, np.float32).astype(dt)
    pmin = np.asarray(pc_min, np.float32).astype(dt)
    p = ind[:, [3, 2, 1]].astype(dt) * scale + pmin
    if aug_inv is not None:
        g = np.asarray(aug_inv, np.float32).reshape(batch, 30).astype(dt)
        p = p + g[b, 0:3]
        for f in range(3):
            m = g[:, 3 + 9 * f:12 + 9 * f].reshape(batch, 3, 3)[b]           # [n, 3, 3]; q_j = sum_i p_i m[i][j]
            p = (p[:, :, None] * m).sum(1, dtype=dt)
    l2c = np.asarray(lidar2cam, np.float32).reshape(batch, ncam, 4, 4).astype(dt)
    K = np.asarray(intrinsic, np.float32).reshape(batch, ncam, 3, 3).astype(dt)
    hw = np.asarray(raw_hw).reshape(batch, ncam, 2).astype(np.int64)
    fs = np.asarray(feat_scale, np.float32).reshape(batch, ncam, 2)
    thres = np.asarray(depth_thres, np.float32).astype(dt)
    s = np.float32(image_scale)
    grid = np.zeros((ncam, n, 2), np.int32)
    mask = np.zeros((ncam, n), np.uint8)
    depth = np.zeros((ncam, n), dt)
    decided = np.zeros((ncam, n), bool)
    ph = np.concatenate([p, np.ones((n, 1), dt)], 1)
    with np.errstate(all="ignore"):
        for cam in range(ncam):
            c = (l2c[b, cam, :3, :] * ph[:, None, :]).sum(2, dtype=dt)     # [n, 3] camera xyz
            uvw = (K[b, cam] * c[:, None, :]).sum(2, dtype=dt)
            u, v, cz = uvw[:, 0] / uvw[:, 2], uvw[:, 1] / uvw[:, 2], c[:, 2]
            ok = np.isfinite(u) & np.isfinite(v) & (np.abs(u) < 1e9) & (np.abs(v) < 1e9)
            us, vs = np.where(ok, u, 0), np.where(ok, v, 0)
            gx = (s * np.trunc(us).astype(np.float32)).astype(np.int64)        # fp32 multiply, truncation toward zero
            gy = (s * np.trunc(vs).astype(np.float32)).astype(np.int64)
            ok &= (gx > 0) & (gx < hw[b, cam, 1]) & (gy > 0) & (gy < hw[b, cam, 0]) & (cz > thres[cam])
            fx = (gx.astype(np.float32) * fs[b, cam, 0]).astype(np.int64)
            fy = (gy.astype(np.float32) * fs[b, cam, 1]).astype(np.int64)
            grid[cam, :, 0] = np.where(ok, fx, 0)
            grid[cam, :, 1] = np.where(ok, fy, 0)
            mask[cam] = ok
            depth[cam] = np.where(ok, cz, 0)
            far = lambda x: np.abs(x - np.round(x)) > MARGIN * np.maximum(1.0, np.abs(x))     # noqa: E731
            decided[cam] = np.isfinite(u) & np.isfinite(v) & far(us.astype(np.float64)) & far(vs.astype(np.float64)) & \
                (np.abs(cz - thres[cam]) > MARGIN * np.maximum(1.0, np.abs(cz)))
    return grid, mask, p, depth, decided


# ----------------------------------------------------------------------------------------------- winner maps, slots
def winner(ind, grid, mask, B, ncam, H, W):
    """df3d_scatter_winner: [B * ncam, H, W] i32, the highest row projected onto each pixel; pixels outside the map are
    dropped; -1 where the pixel is empty."""
    ind, grid, mask = np.asarray(ind).reshape(-1, 4), np.asarray(grid), np.asarray(mask)
    out = np.full((B * ncam, H, W), -1, np.int32)
    for cam in range(ncam):
        gx, gy = grid[cam, :, 0].astype(np.int64), grid[cam, :, 1].astype(np.int64)
        rows = np.nonzero((mask[cam] != 0) & (gx >= 0) & (gx < W) & (gy >= 0) & (gy < H))[0]
        np.maximum.at(out, (ind[rows, 0].astype(np.int64) * ncam + cam, gy[rows], gx[rows]), rows.astype(np.int32))
    return out


def slots(mask, ind, B, ncam):
    """df3d_query_slots -> pos [ncam, n] i32 (visible rows of the row's sample before it, in that camera: an EXCLUSIVE
    count, on invisible rows too), counts [B * ncam] i32 (list lengths)."""
    ind, mask = np.asarray(ind).reshape(-1, 4), np.asarray(mask)
    n = len(ind)
    pos = np.zeros((ncam, n), np.int32)
    counts = np.zeros(B * ncam, np.int32)
    for b in range(B):
        rows = np.nonzero(ind[:, 0] == b)[0]
        for cam in range(ncam):
            v = (mask[cam, rows] != 0).astype(np.int64)
            pos[cam, rows] = np.cumsum(v) - v
            counts[b * ncam + cam] = v.sum()
    return pos, counts


# ------------------------------------------------------------------------------------------------------- image gate
def gate_S(feat, pinv, T, winner, clear, S_in, s9=None, fp32=False):
    """df3d_gate_scatter_rows / df3d_gate_rows (s9 None: the row response T [9, C + 3] . (feat[row], pinv[row]) computed
    here) and df3d_gate_scatter (s9 [n, 9] given): S [NI, 9, H, W] (+)= the response of every pixel's winner row; with
    `clear` S starts from zero, otherwise from S_in."""
    dt = _dt(fp32)
    win = np.asarray(winner)
    NI, H, W = win.shape
    S = np.zeros((NI, 9, H, W), dt) if clear else np.array(S_in, dt).reshape(NI, 9, H, W)
    img, y, x = np.nonzero(win >= 0)
    rows = win[img, y, x]
    if s9 is None:
        r = np.concatenate([np.asarray(feat)[rows], np.asarray(pinv)[rows]], 1).astype(dt) @ np.asarray(T).astype(dt).T
    else:
        r = np.asarray(s9)[rows].astype(dt)
    S[img, :, y, x] += r
    return S


def gate_att(gate, gate_bias, S, kg, fp32=False):
    """df3d_gate_finish (gate_bias None) / df3d_gate_finish_bias: att [NI, H, W] =
    sigmoid(kg[18] + sum over the 3x3 taps t inside the map of (kg[t] + kg[9 + t] * (gate + gate_bias)[p + t] + S[t][p + t]))."""
    dt = _dt(fp32)
    gate, S, kg = np.asarray(gate).astype(dt), np.asarray(S).astype(dt), np.asarray(kg).astype(dt)
    NI, H, W = gate.shape
    if gate_bias is not None:
        gate = gate + np.asarray(gate_bias).astype(dt).reshape(-1)[0]
    acc = np.full((NI, H, W), kg[18], dt)
    for ty in range(3):
        for tx in range(3):
            k = ty * 3 + tx
            # output pixel (y, x) reads (y + ty - 1, x + tx - 1) where that lies inside the map
            y0, y1 = max(0, 1 - ty), min(H, H + 1 - ty)
            x0, x1 = max(0, 1 - tx), min(W, W + 1 - tx)
            if y0 >= y1 or x0 >= x1:
                continue
            src = (slice(None), slice(y0 + ty - 1, y1 + ty - 1), slice(x0 + tx - 1, x1 + tx - 1))
            acc[:, y0:y1, x0:x1] += kg[k] + kg[9 + k] * gate[src] + S[:, k][src]
    return (1 / (1 + np.exp(-acc))).astype(dt)


# -------------------------------------------------------------------------------------------------- query assembly
def assemble(feat, pinv, ind, grid, mask, pos, img, B, ncam, H, W, max_ne, att=None, want_qpos=False, fp32=False):
    """df3d_assemble_queries (att None, no qpos) / df3d_assemble_queries2 and its variants: the padded per-image query
    tensors.  v_feat [NI, max_ne, C] and qpts [NI, max_ne, 3] are copies of the visible rows at their slots; v_i_feat
    [NI, max_ne, Ci] is the image column at the row's pixel (times att there); qgrid = (x / W, y / H); qpos the depth sine
    embedding of point_inv x: d = x / 60 * 2 pi, d / 10000^(2 (c // 2) / C), sin on even and cos on odd channels.
    Padding rows are zero, qpos 0 on even and 1 on odd channels.  Rows whose slot is >= max_ne are dropped.
    img: [NI, Ci, H, W].  -> dict of arrays (None for qpos unless wanted)."""
    dt = _dt(fp32)
    feat, pinv, ind, grid, mask, pos = [np.asarray(a) for a in (feat, pinv, ind, grid, mask, pos)]
    ind = ind.reshape(-1, 4)
    C = feat.shape[1]
    img = np.asarray(img)
    NI, Ci = B * ncam, img.shape[1]
    out = dict(v_feat=np.zeros((NI, max_ne, C), np.float32), v_i_feat=np.zeros((NI, max_ne, Ci), dt),
               qgrid=np.zeros((NI, max_ne, 2), dt), qpts=np.zeros((NI, max_ne, 3), np.float32), qpos=None)
    if want_qpos:
        out["qpos"] = np.zeros((NI, max_ne, C), dt)
        out["qpos"][:, :, 1::2] = 1
        dim_t = np.asarray(10000.0, dt) ** ((2 * (np.arange(C) // 2)).astype(dt) / np.asarray(C, dt))
    for cam in range(ncam):
        rows = np.nonzero((mask[cam] != 0) & (pos[cam] < max_ne))[0]
        if not len(rows):
            continue
        im = ind[rows, 0].astype(np.int64) * ncam + cam
        sl = pos[cam, rows]
        gx, gy = grid[cam, rows, 0].astype(np.int64), grid[cam, rows, 1].astype(np.int64)
        out["v_feat"][im, sl] = feat[rows]
        out["qpts"][im, sl] = pinv[rows]
        col = img[im, :, gy, gx].astype(dt)
        if att is not None:
            col = col * np.asarray(att)[im, gy, gx].astype(dt)[:, None]
        out["v_i_feat"][im, sl] = col
        out["qgrid"][im, sl, 0] = gx.astype(dt) / np.asarray(W, dt)
        out["qgrid"][im, sl, 1] = gy.astype(dt) / np.asarray(H, dt)
        if want_qpos:
            d = pinv[rows, 0].astype(dt) / np.asarray(60, dt) * np.asarray(2 * np.pi, dt)
            v = d[:, None] / dim_t[None]
            out["qpos"][im, sl] = np.where(np.arange(C) % 2 == 1, np.cos(v), np.sin(v))
    return out


def pixel_rows(ind, grid, mask, B, ncam, H, W):
    """df3d_query_pixel_rows -> pixrow [B * ncam * H * W] i32: rank of every pixel some visible row projects to, in
    image-major, row-major order, -1 elsewhere; and their number."""
    ind, grid, mask = np.asarray(ind).reshape(-1, 4), np.asarray(grid), np.asarray(mask)
    flag = np.zeros((B * ncam, H, W), bool)
    for cam in range(ncam):
        rows = np.nonzero(mask[cam] != 0)[0]
        flag[ind[rows, 0].astype(np.int64) * ncam + cam, grid[cam, rows, 1], grid[cam, rows, 0]] = True
    flat = flag.reshape(-1)
    rank = np.cumsum(flat) - flat
    return np.where(flat, rank, -1).astype(np.int32), int(flat.sum())


def writeback(feat, enh, ind, mask, pos, max_ne):
    """df3d_fusion_writeback: out[row] = feat[row] + sum over the cameras that see the row, in camera order, of
    enh[b * ncam + cam][pos]; slots >= max_ne add nothing.  fp32 adds in that order: plain adds, the same bits."""
    feat, enh, ind, mask, pos = [np.asarray(a) for a in (feat, enh, ind, mask, pos)]
    ind = ind.reshape(-1, 4)
    ncam = mask.shape[0]
    out = np.array(feat, np.float32)
    enh = np.asarray(enh, np.float32).reshape(-1, max_ne, feat.shape[1])
    for cam in range(ncam):
        rows = np.nonzero((mask[cam] != 0) & (pos[cam] < max_ne))[0]
        out[rows] = out[rows] + enh[ind[rows, 0].astype(np.int64) * ncam + cam, pos[cam, rows]]
    return out


# ------------------------------------------------------------------------------------------------------- yardstick
def errors(got, ref64, ref32):
    """-> (largest |got - float64 reference|, largest |fp32 evaluation - float64 reference|, scale of the tensor)."""
    ref64 = np.asarray(ref64, np.float64)
    if ref64.size == 0:
        return 0.0, 0.0, 1.0
    return (float(np.abs(np.asarray(got, np.float64) - ref64).max()), float(np.abs(np.asarray(ref32, np.float64) - ref64).max()),
            max(1.0, float(np.abs(ref64).max())))


def assert_within_yardstick(name, got, ref64, ref32):
    """The rule of tests/test_gpu_cptrain.py: at most four times the fp32 yardstick's largest error plus 1e-6 of the scale --
    room for another summation order and a fast exponential, none for a wrong term."""
    err, yard, scale = errors(got, ref64, ref32)
    print("%s: kernel %.3g, fp32 yardstick %.3g, scale %.3g" % (name, err, yard, scale))
    assert err <= 4.0 * yard + 1e-6 * scale, (name, err, yard, scale)
    return err, yard


# ----------------------------------------------------------------------------------------------------------- inputs
def glue_case(seed, per_sample_rows, ncam, H, W, C, Ci, density, out_of_map=False):
    """Inputs of the slot / scatter kernels: batch-sorted indices with per_sample_rows[b] rows of sample b (zeros allowed),
    a visibility mask of the given density and in-map pixels drawn, per sample, from so few distinct pixels that a pixel
    holds at least 3 visible rows on average: winners are contested; the first four visible rows of every list sit on the map's
    four corners.
    Lists with a shape of their own: in the largest sample the last camera sees nothing and camera 1 (where there is one) sees
    nothing in the first and in the last quarter of the rows; in the second largest sample camera 0 sees every row.
    out_of_map: three entries in ten are redrawn from -3 .. W + 2 / -3 .. H + 2 (for the scatter entries, which drop them)."""
    rs = np.random.RandomState(seed)
    B = len(per_sample_rows)
    n = int(sum(per_sample_rows))
    ind = np.zeros((n, 4), np.int32)
    ind[:, 0] = np.repeat(np.arange(B), per_sample_rows)
    ind[:, 1:] = rs.randint(0, 40, (n, 3))
    mask = (rs.uniform(size=(ncam, n)) < density).astype(np.uint8)
    start = np.concatenate([[0], np.cumsum(per_sample_rows)])
    order = np.argsort(per_sample_rows, kind="stable")[::-1]
    big, second = int(order[0]), int(order[1]) if B > 1 else None
    mask[ncam - 1, start[big]:start[big + 1]] = 0
    if ncam > 2:
        q = per_sample_rows[big] // 4
        mask[1, start[big]:start[big] + q] = 0
        mask[1, start[big + 1] - q:start[big + 1]] = 0
    if second is not None and per_sample_rows[second] > 0:
        mask[0, start[second]:start[second + 1]] = 1
    grid = np.zeros((ncam, n, 2), np.int32)
    corners = np.array([0, W - 1, (H - 1) * W, H * W - 1])
    for b in range(B):
        rows = per_sample_rows[b]
        if rows == 0:
            continue
        npx = int(min(H * W, max(1, density * rows / 3)))
        pix = rs.permutation(H * W)[:npx]
        sel = pix[rs.randint(0, npx, (ncam, rows))]
        grid[:, start[b]:start[b + 1], 0] = sel % W
        grid[:, start[b]:start[b + 1], 1] = sel // W
    if out_of_map:
        redo = rs.uniform(size=(ncam, n)) < 0.3
        wide = np.stack([rs.randint(-3, W + 3, (ncam, n)), rs.randint(-3, H + 3, (ncam, n))], 2).astype(np.int32)
        grid = np.where(redo[:, :, None], wide, grid)
    for b in range(B):                                   # a winner on every corner: the first visible rows of every list go there
        for cam in range(ncam):
            rows = start[b] + np.nonzero(mask[cam, start[b]:start[b + 1]])[0][:4]
            if len(rows) == 4:
                grid[cam, rows, 0], grid[cam, rows, 1] = corners % W, corners // W
    pinv = rs.uniform(-50, 50, (n, 3)).astype(np.float32)
    return dict(B=B, ncam=ncam, H=H, W=W, C=C, Ci=Ci, n=n, ind=ind, mask=mask, grid=np.ascontiguousarray(grid),
                feat=rs.standard_normal((n, C)).astype(np.float32), pinv=pinv,
                img=rs.standard_normal((B * ncam, Ci, H, W)).astype(np.float32),
                att=rs.uniform(0.05, 1.0, (B * ncam, H, W)).astype(np.float32))


SLOT_ROWS = (1, 0, 1024, 1025, 2500, 0)          # a single row, empty samples inside and at the end, the 1024-row pass and past it


def camera_rig(yaw_offset_deg, focal, raw_hw, ncam=6):
    """ncam pinhole cameras at equal yaw spacing around the sensor (x forward, z up), 0.3 m off the axis:
    -> lidar2cam [ncam, 4, 4], intrinsic [ncam, 3, 3] float32; raw_hw [ncam, 2] gives every camera's principal point."""
    base = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])
    l2c, K = np.zeros((ncam, 4, 4)), np.zeros((ncam, 3, 3))
    for c in range(ncam):
        a = np.deg2rad(360.0 / ncam * c + yaw_offset_deg)
        R = base @ np.array([[np.cos(a), np.sin(a), 0.0], [-np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
        l2c[c] = np.eye(4)
        l2c[c, :3, :3] = R
        l2c[c, :3, 3] = -R @ np.array([0.3 * np.cos(a), 0.3 * np.sin(a), -0.3])
        K[c] = [[focal, 0.0, raw_hw[c][1] / 2.0], [0.0, focal, raw_hw[c][0] / 2.0], [0.0, 0.0, 1.0]]
    return l2c.astype(np.float32), K.astype(np.float32)


PROJ_VOXEL, PROJ_RANGE, PROJ_IMAGE_SCALE = [0.075, 0.075, 0.2], [-9.6, -9.6, -5.0, 9.6, 9.6, 3.0], 2.0 / 3.0
PROJ_THRES = [1.0, 0.0, 0.25, 0.5, 0.0, 2.0]     # one depth threshold per camera


def projection_aug(B):
    """A per-sample inverse augmentation [B, 30]: a translation, a rescale, a rotation about z and a flip, all different
    between the samples (the flip alternates between the y and the x axis)."""
    g = np.zeros((B, 30), np.float32)
    for b in range(B):
        a = -(0.17 - 0.3 * b)
        c, s = np.cos(a), np.sin(a)
        g[b, :3] = -np.array([0.21, -0.13, 0.05]) * (b + 1)
        g[b, 3:12] = (np.eye(3) / (1.05 - 0.08 * b)).reshape(-1)
        g[b, 12:21] = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]).reshape(-1)
        g[b, 21:30] = np.diag([1, -1, 1] if b % 2 == 0 else [-1, 1, 1]).reshape(-1)
    return g


def projection_case(coords, d_factor, aug, B=2):
    """The arguments of df3d_project_voxels on one voxel set [n, 4] (b, z, y, x) of the golden geometry: every sample's six
    cameras aimed with a yaw offset and a focal length of their own, an image size (hence a principal point and a feature
    scale) per (sample, camera), a depth threshold per camera.  -> dict of `project`'s keyword arguments (+ feat_hw)."""
    ncam = 6
    raw_hw = np.array([[[160 + 8 * ((b + c) % 3), 213 + 6 * c - 20 * b] for c in range(ncam)] for b in range(B)], np.int32)
    feat_hw = np.array([[[40 + c - 3 * b, 54 - 2 * c + b] for c in range(ncam)] for b in range(B)], np.int32)
    l2c, K = zip(*[camera_rig(7.3 + 11.9 * b, 250.0 - 35.0 * b, raw_hw[b]) for b in range(B)])
    fs = np.stack([(feat_hw[:, :, 1] / raw_hw[:, :, 1].astype(np.float64)).astype(np.float32),
                   (feat_hw[:, :, 0] / raw_hw[:, :, 0].astype(np.float64)).astype(np.float32)], 2)
    return dict(indices=np.ascontiguousarray(coords, np.int32), batch=B, ncam=ncam,
                scale_xyz=(np.asarray(PROJ_VOXEL, np.float32) * np.float32(d_factor)).astype(np.float32),
                pc_min=np.asarray(PROJ_RANGE[:3], np.float32), lidar2cam=np.stack(l2c), intrinsic=np.stack(K), raw_hw=raw_hw,
                depth_thres=np.asarray(PROJ_THRES, np.float32), image_scale=np.float32(PROJ_IMAGE_SCALE), feat_scale=fs,
                aug_inv=projection_aug(B) if aug else None, feat_hw=feat_hw)


def projection_cases(sets):
    """sets: the three golden voxel sets (x_conv2..4, two samples) -> {name: projection_case}: every level without and with
    the augmentation, and a three-sample case whose middle sample has no rows (the last level, its second sample renamed)."""
    cases = {}
    for li, d in enumerate((2, 4, 8)):
        for aug in (False, True):
            cases["level%d%s" % (li, "_aug" if aug else "")] = projection_case(sets[li], d, aug)
    hole = np.array(sets[2], np.int32)
    hole[hole[:, 0] == 1, 0] = 2
    cases["empty_middle_aug"] = projection_case(hole, 8, True, B=3)
    return cases


def project_args(case):
    return {k: v for k, v in case.items() if k != "feat_hw"}


def exact_projection_case():
    """Power-of-two focal length, principal point, voxel size and coordinates, an axis-aligned camera at the origin: every
    intermediate is exactly representable, so there is no margin and every pair counts.  One camera, looking along +x
    (camera x = -lidar y, camera y = -lidar z, depth = lidar x); W_raw = 64, H_raw = 32, focal 16, principal point (32, 16),
    image_scale 1, feat_scale 0.5, threshold 2.  u = 32 - 16 y / x lands on 0, 1, W_raw - 1 and W_raw, depth on the threshold:
    the strict inequalities 0 < x < W_raw, 0 < y < H_raw and depth > thres.  -> (project keyword arguments, expected mask)."""
    l2c = np.eye(4, dtype=np.float32)
    l2c[:3, :3] = [[0, -1, 0], [0, 0, -1], [1, 0, 0]]
    K = np.array([[16, 0, 32], [0, 16, 16], [0, 0, 1]], np.float32)
    # voxel size 0.25, pc_min (-8, -64, -16): x = ix / 4 - 8, y = iy / 4 - 64, z = iz / 4 - 16
    pts = [  # (x, y, z) lidar, expected visibility
        ((4.0, 8.0, 0.0), 0),       # u = 0: not > 0
        ((4.0, 7.75, 0.0), 1),      # u = 1
        ((4.0, -7.75, 0.0), 1),     # u = 63 = W_raw - 1
        ((4.0, -8.0, 0.0), 0),      # u = 64 = W_raw: not < W_raw
        ((4.0, 0.0, 4.0), 0),       # v = 0
        ((4.0, 0.0, 3.75), 1),      # v = 1
        ((4.0, 0.0, -3.75), 1),     # v = 31 = H_raw - 1
        ((4.0, 0.0, -4.0), 0),      # v = 32 = H_raw
        ((2.0, 0.0, 0.0), 0),       # depth on the threshold: not > thres
        ((2.5, 0.0, 0.0), 1),       # just past it
        ((-4.0, 0.0, 0.0), 0),      # behind the camera, pixel (32, 16) inside the image
    ]
    ind = np.array([[0, round((z + 16) * 4), round((y + 64) * 4), round((x + 8) * 4)] for (x, y, z), _ in pts], np.int32)
    args = dict(indices=ind, batch=1, ncam=1, scale_xyz=np.array([0.25, 0.25, 0.25], np.float32),
                pc_min=np.array([-8, -64, -16], np.float32), lidar2cam=l2c[None, None], intrinsic=K[None, None],
                raw_hw=np.array([[[32, 64]]], np.int32), depth_thres=np.array([2.0], np.float32), image_scale=np.float32(1.0),
                feat_scale=np.array([[[0.5, 0.5]]], np.float32), aug_inv=None)
    return args, np.array([m for _, m in pts], np.uint8)
