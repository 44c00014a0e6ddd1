"""Host restatement (numpy) of the stacked furthest point sampling kernel for tests/test_stackfps_host.py,
tests/test_gpu_stackfps.py and tests/golden/make_golden_stackfps.py: both modes of df3d_stack_furthest_point_sample
(include/df3d_hip.h), `sector_fps`, the margin of every pick, and the clouds and segment sizes the tests share.
Nothing here imports the product."""
import math

import numpy as np

F32 = np.float32
STACK, FRAMES = 0, 1                       # DF3D_FPS_STACK / DF3D_FPS_FRAMES
MAXPT = 32                                 # rows per thread kept in registers; above 32 * 1024 rows the minima live in `temp`


# ---- the distance
def _fma32(x, y, c):
    """float32 fma(x, y, c) with ONE rounding, for float32 x, y, c >= 0 held in float64: the product is exact in float64
    (48 bits), the sum is rounded to odd in float64 (TwoSum gives the error's sign), and a round-to-odd value with two or
    more spare bits rounds to float32 as the exact sum would."""
    p = x * y
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    s = np.where((err != 0) & even, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(F32).astype(np.float64)


def dist2_fma(points, centre):
    """fma(dz, dz, fma(dy, dy, dx * dx)) in float32: exactly the three roundings of the kernels' dist2_fma"""
    d = (np.asarray(points, F32) - np.asarray(centre, F32)[None]).astype(F32).astype(np.float64)
    a = (d[:, 0] * d[:, 0]).astype(F32).astype(np.float64)
    return _fma32(d[:, 2], d[:, 2], _fma32(d[:, 1], d[:, 1], a)).astype(F32)


def dist2_unfused(points, centre):
    """((dx * dx) + (dy * dy)) + (dz * dz), every operation rounded to float32"""
    d = (np.asarray(points, F32) - np.asarray(centre, F32)[None]).astype(F32)
    sq = (d * d).astype(F32)
    return ((sq[:, 0] + sq[:, 1]).astype(F32) + sq[:, 2]).astype(F32)


# ---- one segment
def fps_block(n):
    """the largest power of two <= n, at most 1024, from the bit length (the kernel's form)"""
    return min(1 << (int(n).bit_length() - 1), 1024)


def fps_block_log(n):
    """opt_n_threads of the reference and fps_block() of the library: (int)(log(n) / log(2))"""
    return max(min(1 << int(math.log(float(n)) / math.log(2.0)), 1024), 1)


def segment_picks(pts, picks, bs, dist=dist2_fma, margins=None):
    """`picks` local rows of one segment: row 0, then the maximum of the running minimum (started at 1e10) of `dist` to
    the picks so far.  Equal maxima: the lower (k mod bs), then the lower k.  picks may exceed len(pts): the loop keeps
    picking.  margins (a list): gets, per pick, the gap in ulps between the best and the second-best DISTINCT value."""
    pts = np.asarray(pts, F32)
    best = np.full(len(pts), 1e10, F32)
    out = np.zeros(picks, np.int64)
    for j in range(1, picks):
        best = np.minimum(best, dist(pts, pts[out[j - 1]]))
        top = best.max()
        ties = np.nonzero(best == top)[0]
        out[j] = int(ties[np.lexsort((ties, ties % bs))[0]])
        if margins is not None:
            below = best[best < top]
            margins.append((float(top) - float(below.max())) / float(np.spacing(top)) if len(below) else np.inf)
    return out


def pick_margins(pts, picks, bs, dist=dist2_fma):
    """the margins of picks 1 .. picks - 1, and inf in front (pick 0 is the first row whatever the distances are)"""
    m = [np.inf]
    segment_picks(pts, picks, bs, dist, m)
    return np.asarray(m, np.float64)


def count_tied_picks(pts, picks, bs):
    """picks (after the first) taken among two or more rows of equal running minimum"""
    pts = np.asarray(pts, F32)
    best = np.full(len(pts), 1e10, F32)
    out, n = segment_picks(pts, picks, bs), 0
    for j in range(1, picks):
        best = np.minimum(best, dist2_fma(pts, pts[out[j - 1]]))
        n += int((best == best.max()).sum() > 1)
    return n


# ---- the launch
def stack_fps(xyz, xyz_cnt, num_sampled, mode, idx=None, dist=dist2_fma):
    """df3d_stack_furthest_point_sample: -> idx int32 [M] (M = len(idx) when `idx` is given, which is then filled in place
    and otherwise left as it is; else sum(num_sampled)).  Global rows; -1 for a segment without rows; counts clipped to
    the rows and the slots there are."""
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    N = len(xyz)
    num = [max(int(v), 0) for v in num_sampled]
    cnt = [max(int(v), 0) for v in xyz_cnt]
    if idx is None:
        idx = np.zeros(sum(num), np.int32)
    M = len(idx)
    s = t = 0
    for n_k, m_k in zip(cnt, num):
        S, T = min(s, N), min(t, M)
        n, m = min(n_k, N - S), min(m_k, M - T)
        s, t = s + n_k, t + m_k
        if m == 0:
            continue
        if n == 0:
            idx[T:T + m] = -1
            continue
        if mode == STACK:
            picks = segment_picks(xyz[S:S + n], m, 1024, dist)
        else:
            first = segment_picks(xyz[S:S + n], min(n, m), fps_block(n), dist)
            picks = first[np.arange(m) % len(first)]
        idx[T:T + m] = picks + S
    return idx


def variant(n, mode):
    """which in-kernel variant a segment of n rows takes: rows per thread 8 / 16 / 24 / 32 in registers, or 'temp'"""
    bs = 1024 if mode == STACK else fps_block(n)
    ppt = (n + bs - 1) // bs
    for cap in (8, 16, 24, MAXPT):
        if ppt <= cap:
            return str(cap)
    return "temp"


# ---- sector_fps (voxel_set_abstraction.py:78-121)
def sector_of(points, num_sectors):
    """float32 throughout, as the reference's tensors are: (atan2(y, x) + pi) / (2 pi / num_sectors), floor, clamp"""
    points = np.asarray(points, F32)
    ang = (np.arctan2(points[:, 1], points[:, 0]).astype(F32) + F32(np.pi)).astype(F32)
    q = (ang / F32(np.pi * 2 / num_sectors)).astype(F32)
    return np.clip(np.floor(q), 0, num_sectors).astype(np.int64), q


def sector_fps(points, num_sampled_points, num_sectors):
    """-> (sampled points [N_out, 3], xyz in sector order, per-sector counts, per-sector picks)"""
    points = np.asarray(points, F32)
    sec, _ = sector_of(points, num_sectors)
    order = np.argsort(sec, kind="stable")
    order = order[sec[order] < num_sectors]
    xyz = points[order]
    cnt = [int((sec == k).sum()) for k in range(num_sectors)]
    num = [min(c, math.ceil(c / len(points) * num_sampled_points)) for c in cnt]
    if sum(cnt) == 0:
        xyz, cnt, num = points, [len(points)], [num_sampled_points]
    idx = stack_fps(xyz, cnt, num, STACK)
    return xyz[idx], xyz, cnt, num


# ---- the clouds and sizes the host and GPU tests share
def random_cloud(n, seed):
    """float32 points of a KITTI-sized box; used only where every pick's margin is >= MARGIN_ULPS (asserted on the host)"""
    rs = np.random.RandomState(1000 + seed)
    return rs.uniform([0, -40, -3], [70.4, 40, 1], (n, 3)).astype(F32)


def lattice_cloud(n, seed, duplicate=False):
    """coordinates that are multiples of 0.25 below 64 in magnitude (many rows coincide in distance, some in position):
    every product and sum of the distance is exact.  duplicate: every point twice, n rows in all."""
    rs = np.random.RandomState(2000 + seed)
    base = n // 2 if duplicate else n
    pts = (rs.randint(-10, 11, (base, 3)) * 0.25).astype(F32)
    return np.concatenate([pts, pts])[rs.permutation(2 * base)] if duplicate else pts


MARGIN_ULPS = 4.0
SMALL_SIZES = (1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 2049)          # m = min(n, 40)
EDGE_SIZES = (8192, 8193, 16384, 16385, 24576, 24577, 32768, 32769)  # m = 24
SEVEN_SIZES = (5, 0, 700, 9000, 17000, 25000, 33000)
SEVEN_PICKS = (3, 0, 1, 20, 7, 12, 9)
FRAME_SIZES = (200, 50, 5000)                                         # against the batch kernel, 64 picks each


def small_m(n):
    return min(n, 40)


def seven_cloud():
    return np.concatenate([random_cloud(n, 40 + i) for i, n in enumerate(SEVEN_SIZES) if n])


def sector_case(seed=0):
    """(points [300, 3], num_sampled_points, num_sectors): 6 sectors of which one is left empty"""
    rs = np.random.RandomState(3000 + seed)
    ang = rs.uniform(-np.pi, np.pi, 400)
    ang = ang[(ang < -0.05) | (ang > np.pi / 3 + 0.05)]                   # nothing in sector 3 of 6: atan2 in [0, pi / 3)
    q = (ang + np.pi) / (np.pi / 3)
    ang = ang[np.abs(q - np.round(q)) > 0.01][:300]                       # and nothing near a sector's border
    r = rs.uniform(2, 30, len(ang))
    return np.stack([r * np.cos(ang), r * np.sin(ang), rs.uniform(-2, 1, len(ang))], 1).astype(F32), 48, 6
