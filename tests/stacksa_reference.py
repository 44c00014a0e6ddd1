"""Host restatement of the PV-RCNN point branch (numpy / torch-CPU) for tests/test_stacksa_host.py, tests/test_gpu_stacksa.py
and tests/golden/make_golden_vsa.py: the stacked ball query with float32 distances, stack grouping, one StackSAModuleMSG scale
in any dtype (eval or batch statistics; torch, so float64 autograd gives the training reference), the bilinear BEV sample,
voxel centres, furthest point sampling with the keypoint padding, VoxelSetAbstraction.forward and PVRCNNHead.roi_grid_pool.
Nothing here imports the product."""
import numpy as np
import torch

F32 = np.float32


# ---- ball query
def dist2_f32(points, centre):
    """((dx*dx) + (dy*dy)) + (dz*dz), every operation rounded to float32"""
    d = (centre[None].astype(F32) - points.astype(F32)).astype(F32)
    sq = (d * d).astype(F32)
    return ((sq[:, 0] + sq[:, 1]).astype(F32) + sq[:, 2]).astype(F32)


def frame_starts(counts):
    counts = np.asarray(counts, np.int64)
    return np.cumsum(counts) - counts


def frame_of_rows(counts):
    return np.repeat(np.arange(len(counts)), np.asarray(counts, np.int64))


def ball_query_kernel(radius, nsample, xyz, xyz_cnt, new_xyz, new_cnt, idx=None):
    """ball_query_kernel_stack over `idx` (zeros when not given): idx[m, 0] = -1 for an empty ball, the other slots of an
    empty ball untouched.  Also returns the number of hits of every centre (not capped)."""
    xyz, new_xyz = np.asarray(xyz, F32), np.asarray(new_xyz, F32)
    M = new_xyz.shape[0]
    idx = np.zeros((M, nsample), np.int32) if idx is None else idx
    found = np.zeros(M, np.int64)
    starts, frames = frame_starts(xyz_cnt), frame_of_rows(new_cnt)
    r2 = F32(F32(radius) * F32(radius))
    for m in range(M):
        b = frames[m]
        pts = xyz[starts[b]:starts[b] + xyz_cnt[b]]
        hits = np.nonzero(dist2_f32(pts, new_xyz[m]) < r2)[0] if len(pts) else np.zeros(0, np.int64)
        found[m] = len(hits)
        if len(hits) == 0:
            idx[m, 0] = -1
            continue
        idx[m, :] = hits[0]
        take = hits[:nsample]
        idx[m, :len(take)] = take
    return idx, found


def ball_query_stack(radius, nsample, xyz, xyz_cnt, new_xyz, new_cnt):
    """pointnet2_utils.BallQuery: (idx with the rows of empty balls 0, empty_ball_mask)"""
    idx, _ = ball_query_kernel(radius, nsample, xyz, xyz_cnt, new_xyz, new_cnt)
    empty = idx[:, 0] == -1
    idx[empty] = 0
    return idx, empty


def near_boundary(radius, xyz, xyz_cnt, new_xyz, new_cnt, ulps=8):
    """number of (centre, row of its frame) pairs whose float32 d2 lies within `ulps` ulps of radius^2: with none, the
    accepted set does not depend on how a correct implementation rounds"""
    xyz, new_xyz = np.asarray(xyz, F32), np.asarray(new_xyz, F32)
    starts, frames = frame_starts(xyz_cnt), frame_of_rows(new_cnt)
    r2 = F32(F32(radius) * F32(radius))
    tol = ulps * float(np.spacing(r2))
    n = 0
    for m in range(new_xyz.shape[0]):
        b = frames[m]
        pts = xyz[starts[b]:starts[b] + xyz_cnt[b]]
        if len(pts):
            n += int((np.abs(dist2_f32(pts, new_xyz[m]).astype(np.float64) - float(r2)) <= tol).sum())
    return n


def global_rows(idx_local, idx_cnt, feat_cnt):
    return idx_local.astype(np.int64) + frame_starts(feat_cnt)[frame_of_rows(idx_cnt)][:, None]


# ---- one StackSAModuleMSG scale (the state-dict keys of the reference: mlps.{k}.{0,1,3,4}.*)
def sa_scale(sd, k, radius, nsample, xyz, xyz_cnt, new_xyz, new_cnt, features, dtype=torch.float64, training=False,
             pool_method="max_pool", prefix="", eps=1e-5):
    """xyz / new_xyz float32 arrays; features a torch tensor [N, C] (may require grad) or None; sd: tensors (may require grad).
    Any number of (Conv2d, BatchNorm2d, ReLU) layers.  -> [M, C_out] in `dtype`."""
    idx, empty = ball_query_stack(radius, nsample, xyz, xyz_cnt, new_xyz, new_cnt)
    rows = torch.from_numpy(global_rows(idx, new_cnt, xyz_cnt))
    keep = torch.from_numpy(~empty).to(dtype)[:, None, None]
    x = (torch.from_numpy(np.asarray(xyz, F32)).to(dtype)[rows] - torch.from_numpy(np.asarray(new_xyz, F32)).to(dtype)[:, None]) * keep
    if features is not None:
        x = torch.cat([x, features.to(dtype)[rows] * keep], -1)
    M = x.shape[0]
    x = x.reshape(M * nsample, -1)
    layer = 0
    while "%smlps.%d.%d.weight" % (prefix, k, layer) in sd:
        p = lambda name: sd["%smlps.%d.%d.%s" % (prefix, k, layer + 1, name)].to(dtype)
        x = x @ sd["%smlps.%d.%d.weight" % (prefix, k, layer)].to(dtype)[:, :, 0, 0].T
        mean, var = (x.mean(0), x.var(0, unbiased=False)) if training else (p("running_mean"), p("running_var"))
        x = torch.relu((x - mean) / torch.sqrt(var + eps) * p("weight") + p("bias"))
        layer += 3
    x = x.view(M, nsample, -1)
    return x.max(1)[0] if pool_method == "max_pool" else x.mean(1)


def sa_module(sd, radii, nsamples, xyz, xyz_cnt, new_xyz, new_cnt, features, prefix="", **kw):
    return torch.cat([sa_scale(sd, k, radii[k], nsamples[k], xyz, xyz_cnt, new_xyz, new_cnt, features, prefix=prefix, **kw)
                      for k in range(len(radii))], 1)


# ---- BEV sample
def bev_coords(keypoints, point_cloud_range, voxel_size, stride, dtype=torch.float32):
    """x = (px - range_x) / voxel_x / stride in `dtype`, in that order"""
    kp = keypoints.to(dtype)
    x = (kp[:, 1] - point_cloud_range[0]) / voxel_size[0] / stride
    y = (kp[:, 2] - point_cloud_range[1]) / voxel_size[1] / stride
    return x, y


def bilinear_sample(im, x, y):
    """im [H, W, C].  As the reference does (voxel_set_abstraction.py:27-40): floor(x) and floor(x) + 1 are clamped to the
    map first and the weights come from the CLAMPED corners, so outside the map the two coinciding corners cancel."""
    H, W = im.shape[0], im.shape[1]
    x0, x1 = torch.floor(x).long().clamp(0, W - 1), (torch.floor(x).long() + 1).clamp(0, W - 1)
    y0, y1 = torch.floor(y).long().clamp(0, H - 1), (torch.floor(y).long() + 1).clamp(0, H - 1)
    x0f, x1f, y0f, y1f = x0.to(x.dtype), x1.to(x.dtype), y0.to(y.dtype), y1.to(y.dtype)
    wa, wb, wc, wd = (x1f - x) * (y1f - y), (x1f - x) * (y - y0f), (x - x0f) * (y1f - y), (x - x0f) * (y - y0f)
    return ((im[y0, x0] * wa[:, None] + im[y1, x0] * wb[:, None]) + im[y0, x1] * wc[:, None]) + im[y1, x1] * wd[:, None]


def bev_interpolate(keypoints, bev, point_cloud_range, voxel_size, stride, dtype=torch.float32, coord_dtype=None):
    """keypoints [M, 4] (b, x, y, z), bev [B, C, H, W] (torch) -> [M, C]; frame by frame as the reference does it.
    coord_dtype: the precision of the pixel coordinates (default: dtype); float32 coordinates under float64 sums isolate the
    rounding of the sample from that of the coordinates, whose error is absolute (not relative to a small weight)."""
    x, y = [v.to(dtype) for v in bev_coords(keypoints, point_cloud_range, voxel_size, stride, coord_dtype or dtype)]
    out = torch.zeros((keypoints.shape[0], bev.shape[1]), dtype=dtype)
    for b in range(bev.shape[0]):
        mask = keypoints[:, 0] == b
        out[mask] = bilinear_sample(bev[b].to(dtype).permute(1, 2, 0), x[mask], y[mask])
    return out


# ---- keypoints
def voxel_centers(indices_zyx, stride, voxel_size, point_cloud_range):
    """get_voxel_centers in float32: (zyx -> xyz + 0.5) * (voxel_size * stride) + range minimum"""
    c = np.asarray(indices_zyx)[:, [2, 1, 0]].astype(F32)
    size = (np.asarray(voxel_size, F32) * F32(stride)).astype(F32)
    return ((c + F32(0.5)).astype(F32) * size).astype(F32) + np.asarray(point_cloud_range[:3], F32)


def furthest_point_sample(xyz, m):
    """xyz [N, 3] float32 -> m indices: start at row 0, the running minimum of the float32 squared distances, the maximum.
    Equal maxima (voxel centres lie on a lattice) go the way the reference's kernel sends them (sampling_gpu.cu): thread t
    of a block of bs = the largest power of two <= N (at most 1024) scans rows t, t + bs, .. keeping its first maximum, and
    the block reduction keeps the lower thread: the lowest (row mod bs), then the lowest row."""
    xyz = np.asarray(xyz, F32)
    n = len(xyz)
    bs = max(min(1 << int(np.log(float(n)) / np.log(2.0)), 1024), 1)
    best = np.full(n, 1e10, F32)
    out = np.zeros(m, np.int64)
    for j in range(1, m):
        best = np.minimum(best, dist2_f32(xyz, xyz[out[j - 1]]))
        ties = np.nonzero(best == best.max())[0]
        out[j] = int(ties[np.lexsort((ties, ties % bs))[0]])
    return out


def pad_keypoints(picks, num_keypoints):
    times = int(num_keypoints / len(picks)) + 1
    return np.tile(picks, times)[:num_keypoints]


def sample_keypoints(src_points, batch_indices, batch_size, num_keypoints):
    """-> [B * K, 4] (b, x, y, z) float32"""
    rows = []
    for b in range(batch_size):
        pts = np.asarray(src_points, F32)[np.asarray(batch_indices) == b]
        picks = furthest_point_sample(pts, min(len(pts), num_keypoints))
        if len(pts) < num_keypoints:
            picks = pad_keypoints(picks, num_keypoints)
        rows.append(np.concatenate([np.full((num_keypoints, 1), b, F32), pts[picks]], 1))
    return np.concatenate(rows)


# ---- VoxelSetAbstraction.forward and PVRCNNHead.roi_grid_pool
def vsa_forward(sd, cfg, inputs, dtype=torch.float64, eps=1e-5):
    """cfg: the PFE config (a dict); inputs: points [N, 1 + 3 + C], voxel_coords, bev, bev_stride, levels {name: (indices
    [n, 4] bzyx, features [n, C])}.  -> keypoints [B * K, 4], point_features_before_fusion, point_features (torch, dtype)."""
    B, K = inputs["batch_size"], cfg["NUM_KEYPOINTS"]
    vs, pcr = cfg["VOXEL_SIZE"], cfg["POINT_CLOUD_RANGE"]
    if cfg["POINT_SOURCE"] == "raw_points":
        src, bidx = inputs["points"][:, 1:4], inputs["points"][:, 0]
    else:
        src, bidx = voxel_centers(inputs["voxel_coords"][:, 1:4], 1, vs, pcr), inputs["voxel_coords"][:, 0]
    keypoints = sample_keypoints(src, bidx, B, K)
    new_xyz, new_cnt = keypoints[:, 1:4], [K] * B
    parts = []
    if "bev" in cfg["FEATURES_SOURCE"]:
        parts.append(bev_interpolate(torch.from_numpy(keypoints), torch.from_numpy(inputs["bev"]), pcr, vs, inputs["bev_stride"], dtype))
    if "raw_points" in cfg["FEATURES_SOURCE"]:
        pts = inputs["points"]
        c = cfg["SA_LAYER"]["raw_points"]
        cnt = [int((pts[:, 0] == b).sum()) for b in range(B)]
        feats = torch.from_numpy(pts[:, 4:]) if pts.shape[1] > 4 else None
        parts.append(sa_module(sd, c["POOL_RADIUS"], c["NSAMPLE"], pts[:, 1:4], cnt, new_xyz, new_cnt, feats,
                               prefix="SA_rawpoints.", dtype=dtype))
    names = [s for s in cfg["FEATURES_SOURCE"] if s not in ("bev", "raw_points")]
    for k, name in enumerate(names):
        c = cfg["SA_LAYER"][name]
        ind, feats = inputs["levels"][name]
        cnt = [int((ind[:, 0] == b).sum()) for b in range(B)]
        xyz = voxel_centers(ind[:, 1:4], c["DOWNSAMPLE_FACTOR"], vs, pcr)
        parts.append(sa_module(sd, c["POOL_RADIUS"], c["NSAMPLE"], xyz, cnt, new_xyz, new_cnt, torch.from_numpy(feats),
                               prefix="SA_layers.%d." % k, dtype=dtype))
    before = torch.cat(parts, 1)
    p = lambda n: sd["vsa_point_feature_fusion." + n].to(dtype)
    x = before @ p("0.weight").T
    x = torch.relu((x - p("1.running_mean")) / torch.sqrt(p("1.running_var") + eps) * p("1.weight") + p("1.bias"))
    return keypoints, before, x


def dense_grid_points(rois, grid_size):
    """[R, 7] -> [R, g^3, 3] float32, x index slowest"""
    g = grid_size
    ix = np.stack(np.meshgrid(np.arange(g), np.arange(g), np.arange(g), indexing="ij"), -1).reshape(-1, 3).astype(F32)
    size = np.asarray(rois, F32)[:, None, 3:6]
    return ((ix[None] + F32(0.5)) / F32(g) * size - size / F32(2)).astype(F32)


def global_grid_points(rois, grid_size):
    """rotate the local grid about z by the heading and move it to the RoI centre, with torch float32 (cos / sin / matmul of
    the product's helper are float32 too; the grid points feed a ball query, so the test asserts its margin on THESE points)"""
    rois = torch.from_numpy(np.asarray(rois, F32).reshape(-1, rois.shape[-1]))
    local = torch.from_numpy(dense_grid_points(rois.numpy(), grid_size))
    c, s = torch.cos(rois[:, 6]), torch.sin(rois[:, 6])
    z, o = torch.zeros_like(c), torch.ones_like(c)
    rot = torch.stack((c, s, z, -s, c, z, z, z, o), 1).view(-1, 3, 3)
    return (torch.matmul(local, rot) + rois[:, None, 0:3]).numpy()


def pvrcnn_grid_pool(sd, pool_cfg, rois, point_coords, point_features, point_cls_scores, dtype=torch.float64, grid_xyz=None):
    """rois [B, R, 7]; point_coords [P, 4]; -> [B * R, g^3, C_out] (torch, dtype).  grid_xyz: the grid points to pool at
    (default: global_grid_points)."""
    B, g = rois.shape[0], pool_cfg["GRID_SIZE"]
    feats = torch.from_numpy(point_features).to(dtype) * torch.from_numpy(point_cls_scores).to(dtype).view(-1, 1)
    new_xyz = (global_grid_points(rois, g) if grid_xyz is None else grid_xyz).reshape(-1, 3)
    cnt = [int((point_coords[:, 0] == b).sum()) for b in range(B)]
    out = sa_module(sd, pool_cfg["POOL_RADIUS"], pool_cfg["NSAMPLE"], point_coords[:, 1:4], cnt, new_xyz,
                    [rois.shape[1] * g ** 3] * B, feats, prefix="roi_grid_pool_layer.", dtype=dtype)
    return out.view(-1, g ** 3, out.shape[-1])


# ---- fixtures
# (C_in, C1, C2, nsample) of every scale of the shipped config: raw points without / with intensity, x_conv1, x_conv2,
# x_conv3 / x_conv4, the RoI grid pool
SCALE_CLASSES = ((0, 16, 16, 16), (1, 16, 16, 16), (16, 16, 16, 16), (32, 32, 32, 16), (32, 32, 32, 32), (64, 64, 64, 16),
                 (64, 64, 64, 32), (128, 64, 64, 16))
VSA_SEED = 0            # tests/golden/make_golden_vsa.py asserts the ball-query margins of these seeds
HEAD_SEED = 2


def ball_fixture(seed=0):
    """B = 3, xyz counts [37, 0, 90], centres [5, 3, 11].  Frame 0: 32 rows in [0, 4]^3 and 5 within 0.05 of (10, 10, 10).
    Frame 2: 50 rows in [0, 4]^3 and 40 within 0.3 of (2, 2, 2).  Centres: frame 2 has one AT (10, 10, 10) (its nearest rows
    are frame 0's: an empty ball in its own frame) and one at (2, 2, 2) (40 hits); the others are uniform in [0, 4]^3."""
    rs = np.random.RandomState(seed)
    f0 = np.concatenate([rs.uniform(0, 4, (32, 3)), 10 + rs.uniform(-0.05, 0.05, (5, 3))])
    f2 = np.concatenate([rs.uniform(0, 4, (50, 3)), 2 + rs.uniform(-0.17, 0.17, (40, 3))])
    rs.shuffle(f2)
    xyz = np.concatenate([f0, f2]).astype(F32)
    c0, c1, c2 = rs.uniform(0, 4, (5, 3)), rs.uniform(0, 4, (3, 3)), rs.uniform(0, 4, (11, 3))
    c2[3], c2[7] = (10, 10, 10), (2, 2, 2)
    return {"xyz": xyz, "xyz_cnt": [37, 0, 90], "new_xyz": np.concatenate([c0, c1, c2]).astype(F32), "new_cnt": [5, 3, 11],
            "radius": 0.9, "far": 5 + 3 + 3, "dense": 5 + 3 + 7}


def big_ball_fixture(seed=0):
    """one frame of 5 000 rows in [0, 10]^3 and 70 centres, radius 1.0: about 21 rows per interior ball, so a scan for 16 ends
    after some hundred rows while corner centres read the whole frame"""
    rs = np.random.RandomState(100 + seed)
    new_xyz = rs.uniform(0, 10, (70, 3))
    new_xyz[:6] = [(0, 0, 0), (10, 10, 10), (0, 10, 0), (10, 0, 10), (0, 0, 10), (10, 10, 0)]
    return {"xyz": rs.uniform(0, 10, (5000, 3)).astype(F32), "xyz_cnt": [5000], "new_xyz": new_xyz.astype(F32), "new_cnt": [70],
            "radius": 1.0}


def scale_fixture(c_in, seed=0):
    """M = 70 centres (40 + 30), N = 300 rows (180 + 120) in [0, 4]^3, radius 0.8; centre 0 is far from every row"""
    rs = np.random.RandomState(200 + seed)
    new_xyz = rs.uniform(0, 4, (70, 3))
    new_xyz[0] = (20, 20, 20)
    return {"xyz": rs.uniform(0, 4, (300, 3)).astype(F32), "xyz_cnt": [180, 120], "new_xyz": new_xyz.astype(F32),
            "new_cnt": [40, 30], "radius": 0.8,
            "features": rs.standard_normal((300, c_in)).astype(F32) if c_in else None}


def random_sa_state(mlps, seed, use_xyz=True):
    """state dict of a StackSAModuleMSG with `mlps` (input widths without the 3): kaiming-scaled weights, BatchNorms with
    non-trivial affine parameters and running statistics"""
    rs = np.random.RandomState(seed)
    sd = {}
    for k, spec in enumerate(mlps):
        spec = [spec[0] + (3 if use_xyz else 0)] + list(spec[1:])
        for j in range(len(spec) - 1):
            sd["mlps.%d.%d.weight" % (k, 3 * j)] = (rs.standard_normal((spec[j + 1], spec[j], 1, 1)) * np.sqrt(2.0 / spec[j])).astype(F32)
            pre = "mlps.%d.%d." % (k, 3 * j + 1)
            sd[pre + "weight"] = rs.uniform(0.5, 1.5, spec[j + 1]).astype(F32)
            sd[pre + "bias"] = (0.2 * rs.standard_normal(spec[j + 1])).astype(F32)
            sd[pre + "running_mean"] = (0.3 * rs.standard_normal(spec[j + 1])).astype(F32)
            sd[pre + "running_var"] = rs.uniform(0.5, 2.0, spec[j + 1]).astype(F32)
            sd[pre + "num_batches_tracked"] = np.asarray(1, np.int64)
    return sd


def torch_state(sd, prefix=""):
    return {prefix + k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


# the test-sized PFE / head configs: the shipped layer widths and sample counts on an [8, 32, 32] grid of 0.25 m cells
VSA_RANGE = [0.0, -4.0, -2.0, 8.0, 4.0, 2.0]
VSA_VOXEL = [0.25, 0.25, 0.5]
VSA_GRID = (8, 32, 32)                     # (z, y, x)
VSA_LEVEL_CHANNELS = {"x_conv1": 16, "x_conv2": 32, "x_conv3": 64, "x_conv4": 64}
VSA_BEV = (16, 4, 4)                       # C, H, W at stride 8


def vsa_cfg(point_source="raw_points"):
    return {"NAME": "VoxelSetAbstraction", "POINT_SOURCE": point_source, "NUM_KEYPOINTS": 64, "NUM_OUTPUT_FEATURES": 32,
            "SAMPLE_METHOD": "FPS", "FEATURES_SOURCE": ["bev", "x_conv1", "x_conv2", "x_conv3", "x_conv4", "raw_points"],
            "SA_LAYER": {
                "raw_points": {"MLPS": [[16, 16], [16, 16]], "POOL_RADIUS": [0.4, 0.8], "NSAMPLE": [16, 16]},
                "x_conv1": {"DOWNSAMPLE_FACTOR": 1, "MLPS": [[16, 16], [16, 16]], "POOL_RADIUS": [0.4, 0.8], "NSAMPLE": [16, 16]},
                "x_conv2": {"DOWNSAMPLE_FACTOR": 2, "MLPS": [[32, 32], [32, 32]], "POOL_RADIUS": [0.8, 1.2], "NSAMPLE": [16, 32]},
                "x_conv3": {"DOWNSAMPLE_FACTOR": 4, "MLPS": [[64, 64], [64, 64]], "POOL_RADIUS": [1.2, 2.4], "NSAMPLE": [16, 32]},
                "x_conv4": {"DOWNSAMPLE_FACTOR": 8, "MLPS": [[64, 64], [64, 64]], "POOL_RADIUS": [2.4, 4.8], "NSAMPLE": [16, 32]}},
            "VOXEL_SIZE": VSA_VOXEL, "POINT_CLOUD_RANGE": VSA_RANGE}


def vsa_state(cfg, num_bev=VSA_BEV[0], num_raw=4, seed=1000):
    """seeded state dict of a VoxelSetAbstraction built from `cfg`"""
    sd = {}
    names = [s for s in cfg["FEATURES_SOURCE"] if s not in ("bev", "raw_points")]
    c_in = num_bev
    for k, name in enumerate(names):
        c = cfg["SA_LAYER"][name]
        mlps = [[c["MLPS"][0][0]] + list(m) for m in c["MLPS"]]
        sd.update({"SA_layers.%d.%s" % (k, key): v for key, v in random_sa_state(mlps, seed + 10 * k).items()})
        c_in += sum(m[-1] for m in mlps)
    mlps = [[num_raw - 3] + list(m) for m in cfg["SA_LAYER"]["raw_points"]["MLPS"]]
    sd.update({"SA_rawpoints." + key: v for key, v in random_sa_state(mlps, seed + 90).items()})
    c_in += sum(m[-1] for m in mlps)
    rs = np.random.RandomState(seed + 99)
    out = cfg["NUM_OUTPUT_FEATURES"]
    sd["vsa_point_feature_fusion.0.weight"] = (rs.standard_normal((out, c_in)) * np.sqrt(2.0 / c_in)).astype(F32)
    sd["vsa_point_feature_fusion.1.weight"] = rs.uniform(0.5, 1.5, out).astype(F32)
    sd["vsa_point_feature_fusion.1.bias"] = (0.2 * rs.standard_normal(out)).astype(F32)
    sd["vsa_point_feature_fusion.1.running_mean"] = (0.3 * rs.standard_normal(out)).astype(F32)
    sd["vsa_point_feature_fusion.1.running_var"] = rs.uniform(0.5, 2.0, out).astype(F32)
    sd["vsa_point_feature_fusion.1.num_batches_tracked"] = np.asarray(1, np.int64)
    return sd


def head_pool_state(cfg, input_channels=32, seed=2000):
    """seeded state dict of PVRCNNHead.roi_grid_pool_layer"""
    mlps = [[input_channels] + list(m) for m in cfg["ROI_GRID_POOL"]["MLPS"]]
    return {"roi_grid_pool_layer." + k: v for k, v in random_sa_state(mlps, seed).items()}


# the shipped PFE of kitti_models/pv_rcnn_mm_mvx+actrv2_hybrid*.yaml (KITTI range and voxels)
SHIPPED_PFE = dict(vsa_cfg(), NUM_KEYPOINTS=2048, NUM_OUTPUT_FEATURES=128, VOXEL_SIZE=[0.05, 0.05, 0.1],
                   POINT_CLOUD_RANGE=[0, -40, -3, 70.4, 40, 1])
SHIPPED_HEAD = {
    "NAME": "PVRCNNHead", "CLASS_AGNOSTIC": True, "SHARED_FC": [256, 256], "CLS_FC": [256, 256], "REG_FC": [256, 256], "DP_RATIO": 0.3,
    "NMS_CONFIG": {"TRAIN": {"NMS_TYPE": "nms_gpu", "MULTI_CLASSES_NMS": False, "NMS_PRE_MAXSIZE": 9000, "NMS_POST_MAXSIZE": 512,
                             "NMS_THRESH": 0.8},
                   "TEST": {"NMS_TYPE": "nms_gpu", "MULTI_CLASSES_NMS": False, "NMS_PRE_MAXSIZE": 1024, "NMS_POST_MAXSIZE": 100,
                            "NMS_THRESH": 0.7}},
    "ROI_GRID_POOL": {"GRID_SIZE": 6, "MLPS": [[64, 64], [64, 64]], "POOL_RADIUS": [0.8, 1.6], "NSAMPLE": [16, 16],
                      "POOL_METHOD": "max_pool"},
    "TARGET_CONFIG": {"BOX_CODER": "ResidualCoder", "ROI_PER_IMAGE": 128, "FG_RATIO": 0.5, "SAMPLE_ROI_BY_EACH_CLASS": True,
                      "CLS_SCORE_TYPE": "roi_iou", "CLS_FG_THRESH": 0.75, "CLS_BG_THRESH": 0.25, "CLS_BG_THRESH_LO": 0.1,
                      "HARD_BG_RATIO": 0.8, "REG_FG_THRESH": 0.55},
    "LOSS_CONFIG": {"CLS_LOSS": "BinaryCrossEntropy", "REG_LOSS": "smooth-l1", "CORNER_LOSS_REGULARIZATION": True,
                    "LOSS_WEIGHTS": {"rcnn_cls_weight": 1.0, "rcnn_reg_weight": 1.0, "rcnn_corner_weight": 1.0,
                                     "code_weights": [1.0] * 7}}}


def head_cfg():
    """the test-sized head: the shipped structure with MLPS [[16, 16], [16, 16]], 6 RoIs per image and small FC layers"""
    cfg = {k: v for k, v in SHIPPED_HEAD.items()}
    cfg["SHARED_FC"], cfg["CLS_FC"], cfg["REG_FC"] = [32, 32], [32, 32], [32, 32]
    cfg["ROI_GRID_POOL"] = dict(SHIPPED_HEAD["ROI_GRID_POOL"], MLPS=[[16, 16], [16, 16]])
    cfg["TARGET_CONFIG"] = dict(SHIPPED_HEAD["TARGET_CONFIG"], ROI_PER_IMAGE=6)
    return cfg


def vsa_inputs(seed=VSA_SEED):
    """B = 2: frame 0 has 200 points, frame 1 has 50 (fewer than the 64 keypoints); points [250, 5] (b, x, y, z, intensity);
    four sparse levels of random distinct cells (rows in ascending (b, z, y, x) order) with random features; a BEV map."""
    rs = np.random.RandomState(300 + seed)
    lo, hi = np.asarray(VSA_RANGE[:3]), np.asarray(VSA_RANGE[3:])
    pts = []
    for b, n in enumerate((200, 50)):
        p = rs.uniform(lo + 0.3, hi - 0.3, (n, 3))
        pts.append(np.concatenate([np.full((n, 1), b), p, rs.uniform(0, 1, (n, 1))], 1))
    levels = {}
    for name, stride, per_frame in (("x_conv1", 1, 300), ("x_conv2", 2, 200), ("x_conv3", 4, 80), ("x_conv4", 8, 12)):
        shape = [s // stride for s in VSA_GRID]
        rows = []
        for b in range(2):
            flat = np.sort(rs.choice(int(np.prod(shape)), per_frame, replace=False))
            z, y, x = np.unravel_index(flat, shape)
            rows.append(np.stack([np.full(per_frame, b), z, y, x], 1))
        ind = np.concatenate(rows).astype(np.int32)
        levels[name] = (ind, rs.standard_normal((len(ind), VSA_LEVEL_CHANNELS[name])).astype(F32))
    return {"batch_size": 2, "points": np.concatenate(pts).astype(F32), "voxel_coords": levels["x_conv1"][0],
            "bev": rs.standard_normal((2,) + VSA_BEV).astype(F32), "bev_stride": 8, "levels": levels}


def head_inputs(seed=HEAD_SEED):
    """B = 2, 3 RoIs per frame (the last of frame 1 is the all-zero padding RoI), 64 keypoints per frame with 32 channels"""
    rs = np.random.RandomState(400 + seed)
    lo, hi = np.asarray(VSA_RANGE[:3]), np.asarray(VSA_RANGE[3:])
    coords = np.concatenate([np.concatenate([np.full((64, 1), b), rs.uniform(lo + 0.5, hi - 0.5, (64, 3))], 1) for b in range(2)])
    rois = np.concatenate([rs.uniform(lo + 1.5, hi - 1.5, (2, 3, 3)), rs.uniform(1.5, 4.0, (2, 3, 3)), rs.uniform(-3, 3, (2, 3, 1))], -1)
    rois[1, 2] = 0
    return {"batch_size": 2, "rois": rois.astype(F32), "point_coords": coords.astype(F32),
            "point_features": rs.standard_normal((128, 32)).astype(F32), "point_cls_scores": rs.uniform(0, 1, 128).astype(F32)}
