"""Host references of the Voxel-RCNN RoI grid pooling (numpy only; no GPU, no product code).

voxel_query: the literal triple loop of VR/pcdet/ops/pointnet2/pointnet2_stack/src/voxel_query_gpu.cu:10-89 over a dense
[B, Z, Y, X] table, with dist2 = ((dx*dx) + (dy*dy)) + (dz*dz) in float32, every operation rounded separately (numpy float32
scalars do exactly that).  Grouping and its gradient with float64 sums; NeighborVoxelSAModuleMSG (eval mode) and the head's
layers in float64; the grid points of a RoI as voxelrcnn_head.py:194-215 computes them, in float32 like the reference."""
import numpy as np

F32 = np.float32


# ------------------------------------------------------------------------------------------------ query
def dense_table(indices, batch, shape):
    """generate_voxel2pinds: [B, Z, Y, X] int32, -1 where empty, else the row of `indices` [N, 4] (b, z, y, x)."""
    t = np.full((batch,) + tuple(shape), -1, dtype=np.int32)
    t[indices[:, 0], indices[:, 1], indices[:, 2], indices[:, 3]] = np.arange(len(indices), dtype=np.int32)
    return t


def dist2_f32(p, c):
    dx, dy, dz = F32(p[0]) - F32(c[0]), F32(p[1]) - F32(c[1]), F32(p[2]) - F32(c[2])
    return F32(F32(F32(dx * dx) + F32(dy * dy)) + F32(dz * dz))


def voxel_query(table, xyz, new_xyz, new_coords, max_range, radius, nsample):
    """idx int32 [M, nsample] as the kernel leaves it over a zeroed tensor (idx[m, 0] = -1 for an empty ball), and the
    number of accepted neighbours per centre (not capped)."""
    B, Z, Y, X = table.shape
    zr, yr, xr = max_range
    radius2 = F32(F32(radius) * F32(radius))
    M = len(new_xyz)
    idx = np.zeros((M, nsample), dtype=np.int32)
    found = np.zeros((M,), dtype=np.int64)
    for m in range(M):
        b, cz, cy, cx = (int(v) for v in new_coords[m])
        cnt = 0
        for dz in range(-zr, zr + 1):
            z = cz + dz
            if z < 0 or z >= Z:
                continue
            for dy in range(-yr, yr + 1):
                y = cy + dy
                if y < 0 or y >= Y:
                    continue
                for dx in range(-xr, xr + 1):
                    x = cx + dx
                    if x < 0 or x >= X:
                        continue
                    n = table[b, z, y, x]
                    if n < 0:
                        continue
                    if dist2_f32(xyz[n], new_xyz[m]) > radius2:
                        continue
                    found[m] += 1
                    if cnt < nsample:
                        if cnt == 0:
                            idx[m, :] = n
                        idx[m, cnt] = n
                        cnt += 1
        if cnt == 0:
            idx[m, 0] = -1
    return idx, found


def voxel_query_brute(indices, xyz, new_xyz, new_coords, shape, max_range, radius, nsample):
    """The same answer without a table or a scan: all voxels of the centre's frame inside the index box and the ball,
    ordered by flat cell index (= the scan order), the first nsample of them."""
    radius2 = F32(F32(radius) * F32(radius))
    M = len(new_xyz)
    idx = np.zeros((M, nsample), dtype=np.int32)
    d = xyz[None, :, :].astype(F32) - new_xyz[:, None, :].astype(F32)
    d2 = ((d[..., 0] * d[..., 0]) + (d[..., 1] * d[..., 1])) + (d[..., 2] * d[..., 2])
    assert d2.dtype == F32
    flat = (indices[:, 1].astype(np.int64) * shape[1] + indices[:, 2]) * shape[2] + indices[:, 3]
    for m in range(M):
        box = (indices[:, 0] == new_coords[m, 0])
        for a in range(3):
            box &= np.abs(indices[:, 1 + a].astype(np.int64) - int(new_coords[m, 1 + a])) <= max_range[a]
        rows = np.nonzero(box & ~(d2[m] > radius2))[0]
        rows = rows[np.argsort(flat[rows], kind="stable")][:nsample]
        if len(rows) == 0:
            idx[m, 0] = -1
        else:
            idx[m, :] = rows[0]
            idx[m, :len(rows)] = rows
    return idx


def near_boundary(table, xyz, new_xyz, new_coords, max_range, radius, ulps=8):
    """How many candidates (occupied cells inside the index box) have dist2 within `ulps` float32 ulps of radius^2: where
    that is 0, the accepted set does not depend on how dist2 was rounded."""
    B, Z, Y, X = table.shape
    radius2 = F32(F32(radius) * F32(radius))
    tol = ulps * np.spacing(radius2)
    count = 0
    for m in range(len(new_xyz)):
        b, cz, cy, cx = (int(v) for v in new_coords[m])
        z0, z1 = max(cz - max_range[0], 0), min(cz + max_range[0], Z - 1)
        y0, y1 = max(cy - max_range[1], 0), min(cy + max_range[1], Y - 1)
        x0, x1 = max(cx - max_range[2], 0), min(cx + max_range[2], X - 1)
        if z0 > z1 or y0 > y1 or x0 > x1:
            continue
        rows = table[b, z0:z1 + 1, y0:y1 + 1, x0:x1 + 1].ravel()
        rows = rows[rows >= 0]
        d = xyz[rows].astype(np.float64) - new_xyz[m].astype(np.float64)
        count += int((np.abs((d * d).sum(1) - float(radius2)) <= tol).sum())
    return count


# ------------------------------------------------------------------------------------------------ grouping
def frame_starts(counts):
    counts = np.asarray(counts, dtype=np.int64)
    return np.cumsum(counts) - counts


def frame_of_rows(counts):
    return np.repeat(np.arange(len(counts)), np.asarray(counts, dtype=np.int64))


def global_rows(idx_local, idx_batch_cnt, features_batch_cnt):
    return idx_local.astype(np.int64) + frame_starts(features_batch_cnt)[frame_of_rows(idx_batch_cnt)][:, None]


def group_points_stack(features, features_batch_cnt, idx_local, idx_batch_cnt):
    """group_points_gpu.cu:71-102: out [M, C, nsample] = features[start(frame of m) + idx[m, s], c]."""
    rows = global_rows(idx_local, idx_batch_cnt, features_batch_cnt)
    return np.ascontiguousarray(features[rows].transpose(0, 2, 1))


def group_points_stack_grad(grad_out, idx_local, idx_batch_cnt, features_batch_cnt, N):
    """group_points_gpu.cu:15-45 with float64 sums: grad_features [N, C], sum of |contributions| [N, C], references [N]."""
    rows = global_rows(idx_local, idx_batch_cnt, features_batch_cnt).ravel()
    M, C, ns = grad_out.shape
    g = grad_out.astype(np.float64).transpose(0, 2, 1).reshape(M * ns, C)
    out = np.zeros((N, C))
    mag = np.zeros((N, C))
    np.add.at(out, rows, g)
    np.add.at(mag, rows, np.abs(g))
    return out, mag, np.bincount(rows, minlength=N)


# ------------------------------------------------------------------------------------------------ the pooling module
def bn_fold(p, prefix, eps=1e-5):
    scale = p[prefix + ".weight"].astype(np.float64) / np.sqrt(p[prefix + ".running_var"].astype(np.float64) + eps)
    return scale, p[prefix + ".bias"].astype(np.float64) - p[prefix + ".running_mean"].astype(np.float64) * scale


def neighbor_sa_scale(p, k, features, xyz, new_xyz, idx, pool_method):
    """Scale k of NeighborVoxelSAModuleMSG.forward (voxel_pool_modules.py:84-125) in eval mode, float64.  p: the module's
    state_dict as numpy arrays; idx [M, nsample]: the RAW query result (global rows, -1 in slot 0 for an empty ball).
    Returns the scale's output [M, C_out] and the pooled rows before mlps_out [M, C]."""
    f8 = np.float64
    empty = idx[:, 0] == -1
    rows = np.where(empty[:, None], 0, idx)
    s, t = bn_fold(p, "mlps_in.%d.1" % k)
    feats_in = (features.astype(f8) @ p["mlps_in.%d.0.weight" % k][:, :, 0].astype(f8).T) * s + t          # [N, C]
    grouped = feats_in[rows]                                                                                 # [M, ns, C]
    rel = xyz.astype(f8)[rows] - new_xyz.astype(f8)[:, None, :]
    grouped[empty] = 0
    rel[empty] = 0
    s, t = bn_fold(p, "mlps_pos.%d.1" % k)
    pos = (rel @ p["mlps_pos.%d.0.weight" % k][:, :, 0, 0].astype(f8).T) * s + t
    act = np.maximum(grouped + pos, 0)
    pooled = act.max(1) if pool_method == "max_pool" else act.mean(1)
    s, t = bn_fold(p, "mlps_out.%d.1" % k)
    out = np.maximum((pooled @ p["mlps_out.%d.0.weight" % k][:, :, 0].astype(f8).T) * s + t, 0)
    return out, pooled


# ------------------------------------------------------------------------------------------------ the head
def dense_grid_points(rois, grid_size):
    """voxelrcnn_head.py:206-215, float32: rois [R, 7+] -> [R, g^3, 3]; the index runs x slowest (nonzero() order)."""
    g = grid_size
    ii = np.stack(np.meshgrid(np.arange(g), np.arange(g), np.arange(g), indexing="ij"), -1).reshape(-1, 3).astype(F32)
    size = rois[:, None, 3:6].astype(F32)
    return (ii[None] + F32(0.5)) / F32(g) * size - size / F32(2)


def global_grid_points(rois, grid_size):
    """voxelrcnn_head.py:194-204 in float64 from the float32 local points (the rotation is a matmul: the float32 product
    is compared to this within a few ulps of the coordinates' magnitude)."""
    local = dense_grid_points(rois, grid_size).astype(np.float64)
    a = rois[:, 6].astype(np.float64)
    c, s = np.cos(a), np.sin(a)
    x = local[..., 0] * c[:, None] - local[..., 1] * s[:, None]
    y = local[..., 0] * s[:, None] + local[..., 1] * c[:, None]
    return np.stack([x, y, local[..., 2]], -1) + rois[:, None, 0:3].astype(np.float64)


def grid_coords(grid_xyz_f32, point_cloud_range, voxel_size, stride):
    """voxelrcnn_head.py:130-134,169: floor division in float32, then by the stride; (x, y, z) order."""
    out = []
    for a in range(3):
        c = np.floor_divide(grid_xyz_f32[..., a].astype(F32) - F32(point_cloud_range[a]), F32(voxel_size[a]))
        out.append(np.floor_divide(c, F32(stride)))
    return np.stack(out, -1).astype(np.int32)


def voxel_centers(indices_zyx, stride, voxel_size, point_cloud_range):
    """common_utils.get_voxel_centers in float32: [N, 3] (z, y, x) -> [N, 3] (x, y, z)."""
    size = np.asarray(voxel_size, dtype=F32) * F32(stride)
    return (indices_zyx[:, ::-1].astype(F32) + F32(0.5)) * size + np.asarray(point_cloud_range[:3], dtype=F32)


def fc_stack(p, prefix, x, eps=1e-5):
    """Linear (no bias) + BatchNorm1d (eval) + ReLU blocks of an nn.Sequential whose Dropouts are identities, float64."""
    keys = sorted({int(k[len(prefix) + 1:].split(".")[0]) for k in p if k.startswith(prefix + ".") and k.endswith(".weight")
                   and p[k].ndim == 2})
    for i in keys:
        x = x @ p["%s.%d.weight" % (prefix, i)].astype(np.float64).T
        s, t = bn_fold(p, "%s.%d" % (prefix, i + 1), eps)
        x = np.maximum(x * s + t, 0)
    return x


def head_layers(p, pooled):
    """voxelrcnn_head.py:235-238 in eval mode, float64: pooled [R, g^3 * C] -> rcnn_cls [R, 1], rcnn_reg [R, 7]."""
    shared = fc_stack(p, "shared_fc_layer", pooled.astype(np.float64))
    cls = fc_stack(p, "cls_fc_layers", shared) @ p["cls_pred_layer.weight"].astype(np.float64).T + p["cls_pred_layer.bias"]
    reg = fc_stack(p, "reg_fc_layers", shared) @ p["reg_pred_layer.weight"].astype(np.float64).T + p["reg_pred_layer.bias"]
    return cls, reg


# ------------------------------------------------------------------------------------------------ fixtures
GRID = (5, 24, 20)                       # (z, y, x); X = 20: x-runs straddle the 64-cell words of a directory
CELL = (0.2, 0.2, 0.4)                   # cell size (z, y, x) in metres
LOW = (0.0, -2.4, -1.0)                  # range minimum (z, y, x)
SETTINGS = (((1, 2, 2), 0.45, 4), ((4, 4, 4), 0.8, 16), ((1, 1, 1), 0.3, 16))


def cell_centers(indices):
    """xyz [N, 3] (x, y, z) float32 of the cell centres of `indices` [N, 4] (b, z, y, x) on the base grid."""
    zyx = (indices[:, 1:4].astype(np.float64) + 0.5) * np.asarray(CELL) + np.asarray(LOW)
    return np.ascontiguousarray(zyx[:, ::-1]).astype(F32)


def coords_of(new_xyz, frames):
    """[M, 4] (b, z, y, x) int32: the cell a centre falls into (negative or beyond the grid when it lies outside)."""
    zyx = new_xyz[:, ::-1].astype(np.float64)
    c = np.floor((zyx - np.asarray(LOW)) / np.asarray(CELL)).astype(np.int32)
    return np.ascontiguousarray(np.concatenate([np.asarray(frames, dtype=np.int32)[:, None], c], 1))


def base_fixture(seed, batch=2, occupancy=0.3, centres=108, sort_rows=False):
    """B = 2 frames on GRID at 30 % occupancy (about 1450 voxels), rows permuted inside each frame (or sorted by flat
    index), 108 centres uniform over -0.6 .. 1.0 of the extent: many outside the grid, frame by frame in order."""
    rs = np.random.RandomState(seed)
    Z, Y, X = GRID
    frames = []
    for b in range(batch):
        occ = np.nonzero(rs.uniform(size=Z * Y * X) < occupancy)[0]
        if not sort_rows:
            occ = rs.permutation(occ)
        z, r = np.divmod(occ, Y * X)
        y, x = np.divmod(r, X)
        frames.append(np.stack([np.full_like(z, b), z, y, x], 1))
    indices = np.ascontiguousarray(np.concatenate(frames).astype(np.int32))
    extent = np.asarray(GRID) * np.asarray(CELL)
    zyx = np.asarray(LOW) + rs.uniform(-0.6, 1.0, size=(centres, 3)) * extent
    new_xyz = np.ascontiguousarray(zyx[:, ::-1]).astype(F32)
    per = [centres // batch + (1 if b < centres % batch else 0) for b in range(batch)]
    fr = np.repeat(np.arange(batch), per)
    return {"batch": batch, "shape": GRID, "indices": indices, "xyz": cell_centers(indices), "new_xyz": new_xyz,
            "new_coords": coords_of(new_xyz, fr), "new_cnt": np.asarray(per, dtype=np.int32),
            "xyz_cnt": np.asarray([len(f) for f in frames], dtype=np.int32), "table": dense_table(indices, batch, GRID)}


# the RoI head settings of tools/cfgs/kitti_models/voxel_rcnn_car_mm_mvx+actrv2_hybrid_ifat.yaml (ROI_HEAD section)
def _pool_layer(radius):
    return {"MLPS": [[32, 32]], "QUERY_RANGES": [[4, 4, 4]], "POOL_RADIUS": [radius], "NSAMPLE": [16], "POOL_METHOD": "max_pool"}


HEAD_CFG = {
    "NAME": "VoxelRCNNHead", "CLASS_AGNOSTIC": True, "SHARED_FC": [256, 256], "CLS_FC": [256, 256], "REG_FC": [256, 256],
    "DP_RATIO": 0.3,
    "ROI_GRID_POOL": {"FEATURES_SOURCE": ["x_conv2", "x_conv3", "x_conv4"], "PRE_MLP": True, "GRID_SIZE": 6,
                      "POOL_LAYERS": {"x_conv2": _pool_layer(0.4), "x_conv3": _pool_layer(0.8), "x_conv4": _pool_layer(1.6)}},
}
BACKBONE_CHANNELS = {"x_conv1": 16, "x_conv2": 32, "x_conv3": 64, "x_conv4": 64}
KITTI_RANGE = [0, -40, -3, 70.4, 40, 1]
KITTI_VOXEL = [0.05, 0.05, 0.1]
