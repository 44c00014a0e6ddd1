"""Host reference of the dynamic scatter (numpy / CPU torch, float64), written from the behaviour the operator promises:

* a row of `coors` with any negative entry is invalid; the voxels are the distinct valid rows in ascending lexicographic
  order (`np.unique(axis=0)`); `point2voxel_map` is -1 for invalid points;
* `sum` / `mean` / `max` of the point rows per voxel; `mean` = sum / count;
* backward: sum / mean hand every valid point its voxel's gradient (divided by the count for `mean`), `max` hands the
  gradient of each (voxel, channel) to the LOWEST point index whose feature equals the maximum;
* the batched form as a per-sample loop (batch size taken from the last row, samples concatenated in order);
* a DynamicVFE composition from `nn.Linear` / `nn.BatchNorm1d` and indexing, in any dtype.
"""
import numpy as np
import torch
from torch import nn


def plan(coors):
    """-> voxel_coors [M, ndim] int32, point2voxel_map [N] int32, voxel_points_count [M] int32"""
    coors = np.asarray(coors)
    n, ndim = coors.shape
    valid = (coors >= 0).all(axis=1) if n else np.zeros((0,), dtype=bool)
    p2v = np.full((n,), -1, dtype=np.int32)
    if not valid.any():
        return np.zeros((0, ndim), np.int32), p2v, np.zeros((0,), np.int32)
    uniq, inv, cnt = np.unique(coors[valid], axis=0, return_inverse=True, return_counts=True)
    p2v[valid] = inv.reshape(-1).astype(np.int32)
    return uniq.astype(np.int32), p2v, cnt.astype(np.int32)


def reduce(feats, coors, reduce_type, acc=np.float64):
    """-> voxel_feats [M, C] in `acc` (float64; np.longdouble where a float64 result is being judged), voxel_coors,
    point2voxel_map, voxel_points_count"""
    assert reduce_type in ("sum", "mean", "max")
    feats = np.asarray(feats, dtype=acc)
    vc, p2v, cnt = plan(coors)
    m, c = len(vc), feats.shape[1]
    valid = p2v >= 0
    if reduce_type == "max":
        out = np.full((m, c), -np.inf, dtype=acc)
        np.maximum.at(out, p2v[valid], feats[valid])
    else:
        out = np.zeros((m, c), dtype=acc)
        np.add.at(out, p2v[valid], feats[valid])
        if reduce_type == "mean":
            out = out / cnt[:, None].astype(acc)
    return out, vc, p2v, cnt


def abs_sums(feats, p2v, m):
    """S[v, c] = sum of |x| over the voxel's points, float64: the scale of the summation error bounds"""
    feats = np.abs(np.asarray(feats, dtype=np.float64))
    out = np.zeros((m, feats.shape[1]))
    valid = p2v >= 0
    np.add.at(out, p2v[valid], feats[valid])
    return out


def reduce_backward(grad_voxel_feats, feats, coors, reduce_type, dtype=np.float64):
    """-> grad_feats [N, C] in `dtype`: the one division of `mean` happens in that type, so a float32 operator can be
    compared bit for bit"""
    feats = np.asarray(feats, dtype=dtype)
    g = np.asarray(grad_voxel_feats, dtype=dtype)
    vf, _, p2v, cnt = reduce(feats, coors, reduce_type)
    out = np.zeros_like(feats)
    valid = p2v >= 0
    if reduce_type in ("sum", "mean"):
        rows = g[p2v[valid]]
        if reduce_type == "mean":
            rows = rows / cnt[p2v[valid]][:, None].astype(dtype)
        out[valid] = rows
        return out
    n, c = feats.shape
    arg = np.full(vf.shape, n, dtype=np.int64)
    for p in np.nonzero(valid)[0][::-1]:              # descending, so the lowest tied index is written last
        v = p2v[p]
        hit = feats[p] == vf[v]
        arg[v, hit] = p
    for v in range(vf.shape[0]):
        for ch in range(c):
            out[arg[v, ch], ch] = g[v, ch]
    return out


def batched_loop(feats, coors, reduce_type):
    """The per-sample loop over (b, z, y, x) coordinates: batch size = last row's batch id + 1, each sample reduced on its
    (z, y, x) columns, the batch id padded back in front, samples concatenated.  -> voxel_feats, voxel_coors"""
    feats = np.asarray(feats, dtype=np.float64)
    coors = np.asarray(coors)
    batch = int(coors[-1, 0]) + 1
    vfs, vcs = [], []
    for b in range(batch):
        inds = np.nonzero(coors[:, 0] == b)[0]
        vf, vc, _, _ = reduce(feats[inds], coors[inds][:, 1:], reduce_type)
        vfs.append(vf)
        vcs.append(np.concatenate([np.full((len(vc), 1), b, np.int32), vc], axis=1))
    return np.concatenate(vfs, 0), np.concatenate(vcs, 0)


# ------------------------------------------------------------------------------------------ DynamicVFE composition
def _scatter_t(x, p2v, cnt, mode):
    """differentiable torch scatter of rows x [N, C] by the map (mode 'mean' or 'max'; max by the lowest tied index)"""
    m = cnt.shape[0]
    valid = torch.nonzero(p2v >= 0).reshape(-1)
    idx = p2v[valid].long()
    if mode == "mean":
        s = torch.zeros((m, x.shape[1]), dtype=x.dtype).index_add(0, idx, x[valid])
        return s / cnt.to(x.dtype)[:, None]
    with torch.no_grad():
        rows = torch.empty((m, x.shape[1]), dtype=torch.long)
        order = torch.argsort(idx, stable=True)
        bounds = torch.cumsum(torch.cat([torch.zeros(1, dtype=torch.long), cnt.long()]), 0).tolist()
        for v in range(m):
            pts = valid[order[bounds[v]:bounds[v + 1]]]            # ascending point ids of voxel v
            rows[v] = pts[x[pts].max(0).indices]                   # torch returns the first of tied maxima
    return x[rows, torch.arange(x.shape[1])[None, :]]


def _gather_t(vf, p2v):
    out = vf[p2v.clamp(min=0).long()]
    return out * (p2v >= 0).to(vf.dtype)[:, None]


class DynamicVFERef(nn.Module):
    """The DynamicVFE computation for (b, z, y, x) coordinates on the CPU in `dtype`: cluster-centre and voxel-centre
    decorations, then per layer Linear (no bias) -> BatchNorm1d -> ReLU -> scatter -> (gather + concat for the next)."""

    def __init__(self, in_channels, feat_channels, voxel_size, point_cloud_range, mode, eps=1e-3, momentum=0.01,
                 dtype=torch.float64):
        super().__init__()
        self.mode = "max" if mode == "max" else "mean"
        self.vx, self.vy, self.vz = voxel_size
        self.x_offset = self.vx / 2 + point_cloud_range[0]
        self.y_offset = self.vy / 2 + point_cloud_range[1]
        self.z_offset = self.vz / 2 + point_cloud_range[2]
        chans = [in_channels + 6] + list(feat_channels)
        self.vfe_layers = nn.ModuleList([
            nn.Sequential(nn.Linear(chans[i] * (2 if i > 0 else 1), chans[i + 1], bias=False),
                          nn.BatchNorm1d(chans[i + 1], eps=eps, momentum=momentum), nn.ReLU())
            for i in range(len(chans) - 1)]).to(dtype)

    def forward(self, features, coors):
        vc, p2v, cnt = plan(coors.numpy())
        p2v, cnt = torch.from_numpy(p2v), torch.from_numpy(cnt)
        mean = _scatter_t(features[:, :3], p2v, cnt, "mean")
        f_cluster = features[:, :3] - _gather_t(mean, p2v)
        cf = coors.to(features.dtype)
        f_center = torch.stack([features[:, 0] - (cf[:, 3] * self.vx + self.x_offset),
                                features[:, 1] - (cf[:, 2] * self.vy + self.y_offset),
                                features[:, 2] - (cf[:, 1] * self.vz + self.z_offset)], dim=1)
        x = torch.cat([features, f_cluster, f_center], dim=1)
        for i, vfe in enumerate(self.vfe_layers):
            pf = vfe(x)
            vf = _scatter_t(pf, p2v, cnt, self.mode)
            if i != len(self.vfe_layers) - 1:
                x = torch.cat([pf, _gather_t(vf, p2v)], dim=1)
        return vf, torch.from_numpy(vc)
