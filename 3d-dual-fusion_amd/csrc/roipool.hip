// Voxel-RCNN RoI grid pooling (VR/pcdet/ops/pointnet2/pointnet2_stack): voxel query, stack-form grouping and its ordered
// backward, and the fused query + gather + position term + ReLU + pool of NeighborVoxelSAModuleMSG in eval mode.
//
// Voxel query.  The reference (src/voxel_query_gpu.cu:10-89) gives one thread a grid point and walks (2rz+1)(2ry+1)(2rx+1)
// cells of a dense int32 [B,Z,Y,X] tensor.  Here a 16-lane group owns a grid point and each lane takes (dz, dy) ROWS of the
// query range: the x-run of a row is one bit field of the occupancy directory (rulebook.hip), cut from one or two 64-bit
// words, and only its set bits cost a `perm` and an `xyz` read.  Rows are handed out in scan order (dz outer, dy, dx inner),
// 16 per pass; a prefix sum of the lanes' hit counts ranks the hits of a pass, and the scan stops after the pass in which
// the running count reaches nsample.  The dense variant shares the body and reads the reference's tensor cell by cell.
//
// dist2 = ((dx*dx) + (dy*dy)) + (dz*dz) in float32, every operation rounded on its own (__fmul_rn / __fadd_rn: no
// contraction), so the accepted set is a function of the inputs and not of the compiler.
//
// Grouping backward: the reference adds every contribution with a float atomic.  Here the contributions are sorted by the
// row they go to (the plan of dynscatter.hip over the flat [M * nsample] target list: a stable radix sort) and each row sums
// its own in ascending (m, s) order: no atomics, the same bits on every run.
#include "common.h"

namespace df3d {
namespace {

constexpr int VQ_GROUP = 16;           // lanes per grid point
constexpr int VQ_BLOCK = 256;          // 16 grid points per block
constexpr int VQ_MAX_XRANGE = 15;      // the x-run of a row (2 * rx + 1 cells) is cut into one 32-bit mask
constexpr int VP_MAX_NSAMPLE = 16;     // fused pool: the hits of a grid point live in 16 LDS slots

struct QueryGeom {
  int batch, Z, Y, X;
  int rz, ry, rx;
  int nsample;
  float radius2;
  long long n_rows;                    // rows of xyz: every index read from a table is checked against it
};

// ---- cell lookups: the x-run [x0, x0 + len) of row (b, z, y) as a bit mask, and the row number behind a set bit
struct DirectoryLookup {
  GridView g;
  const int32_t *perm;
  unsigned long long w0, w1;
  uint32_t p0;
  int b0;
  __device__ __forceinline__ unsigned load(int b, int z, int y, int x0, int len) {
    const long long flat0 = (long long)b * g.vol + ((long long)z * g.shape[1] + y) * g.shape[2] + x0;
    const long long w = flat0 >> 6;
    b0 = (int)(flat0 & 63);
    w0 = g.bits[w];
    w1 = 0;
    unsigned long long m = w0 >> b0;
    if (b0 + len > 64) {               // the run ends in the next word (which exists: its last cell is a cell of the grid)
      w1 = g.bits[w + 1];
      m |= w1 << (64 - b0);
    }
    const unsigned mask = (unsigned)m & (unsigned)((1ull << len) - 1ull);
    if (mask) p0 = g.prefix[w];
    return mask;
  }
  __device__ __forceinline__ int row(int j) const {
    const int bit = b0 + j;
    int r;
    if (bit < 64)
      r = (int)(p0 + __popcll(w0 & ((1ull << bit) - 1ull)));
    else
      r = (int)(p0 + __popcll(w0) + __popcll(w1 & ((1ull << (bit - 64)) - 1ull)));
    return perm ? perm[r] : r;
  }
};

struct DenseLookup {
  const int32_t *cells;                // [B, Z, Y, X], -1 = empty
  int Z, Y, X;
  const int32_t *run;
  __device__ __forceinline__ unsigned load(int b, int z, int y, int x0, int len) {
    run = cells + ((((long long)b * Z + z) * Y + y) * X + x0);
    unsigned mask = 0;
    for (int j = 0; j < len; ++j) mask |= (run[j] >= 0 ? 1u : 0u) << j;
    return mask;
  }
  __device__ __forceinline__ int row(int j) const { return run[j]; }
};

__device__ __forceinline__ bool vq_accept(const float *__restrict__ xyz, int row, float nx, float ny, float nz, float radius2) {
  const float dx = __fsub_rn(xyz[(long long)row * 3 + 0], nx);
  const float dy = __fsub_rn(xyz[(long long)row * 3 + 1], ny);
  const float dz = __fsub_rn(xyz[(long long)row * 3 + 2], nz);
  const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
  return !(d2 > radius2);
}

// The scan of one grid point by its 16-lane group.  Every lane of the WAVE must call it (the loop condition is made
// wave-uniform, the shuffles stay inside the group); `live` = this group has a grid point.  emit(slot, row) is called
// for the hits 0 .. min(count, nsample) - 1 in scan order.  Returns min(count, nsample), the same in every lane of the group.
template <class Lookup, class Emit>
__device__ __forceinline__ int vq_scan(Lookup &lk, const QueryGeom &q, const float *__restrict__ xyz, bool live, float nx,
                                       float ny, float nz, int cb, int cz, int cy, int cx, Emit emit) {
  const int lane = threadIdx.x & (VQ_GROUP - 1);
  const int ny_rows = 2 * q.ry + 1;
  const int nrows = live && cb >= 0 && cb < q.batch ? (2 * q.rz + 1) * ny_rows : 0;
  // the x-run clipped to the grid; empty when the centre is far outside (64-bit: coordinates of a far centre may be large)
  const long long xlo = (long long)cx - q.rx, xhi = (long long)cx + q.rx;
  const int x0 = (int)(xlo < 0 ? 0 : xlo);
  const int x1 = (int)(xhi > q.X - 1 ? q.X - 1 : xhi);
  const int len = xlo > q.X - 1 || xhi < 0 ? 0 : x1 - x0 + 1;
  int cnt = 0;
  for (int base = 0; __ballot(base < nrows && cnt < q.nsample) != 0ull; base += VQ_GROUP) {
    const bool active = base < nrows && cnt < q.nsample;
    const int r = base + lane;
    unsigned hits = 0;
    if (active && r < nrows && len > 0) {
      const long long z = (long long)cz + (r / ny_rows - q.rz);
      const long long y = (long long)cy + (r % ny_rows - q.ry);
      if (z >= 0 && z < q.Z && y >= 0 && y < q.Y) {
        unsigned mask = lk.load(cb, (int)z, (int)y, x0, len);
        while (mask) {
          const int j = __ffs(mask) - 1;
          mask &= mask - 1;
          const int row = lk.row(j);
          if (row >= 0 && row < q.n_rows && vq_accept(xyz, row, nx, ny, nz, q.radius2)) hits |= 1u << j;
        }
      }
    }
    // exclusive prefix of the lanes' hit counts inside the group, and the group's total
    const int mine = __popc(hits);
    int incl = mine;
#pragma unroll
    for (int d = 1; d < VQ_GROUP; d <<= 1) {
      const int up = __shfl_up(incl, d, VQ_GROUP);
      if (lane >= d) incl += up;
    }
    const int total = __shfl(incl, VQ_GROUP - 1, VQ_GROUP);
    int k = cnt + incl - mine;
    while (hits && k < q.nsample) {
      const int j = __ffs(hits) - 1;
      hits &= hits - 1;
      emit(k, lk.row(j));
      ++k;
    }
    if (active) cnt = cnt + total < q.nsample ? cnt + total : q.nsample;
  }
  return cnt;
}

__device__ __forceinline__ int group_max(int v) {
#pragma unroll
  for (int d = 1; d < VQ_GROUP; d <<= 1) {
    const int o = __shfl_xor(v, d, VQ_GROUP);
    v = o > v ? o : v;
  }
  return v;
}

template <class Lookup>
__global__ __launch_bounds__(VQ_BLOCK) void voxel_query_kernel(Lookup lk, QueryGeom q, const float *__restrict__ xyz,
                                                               const float *__restrict__ new_xyz,
                                                               const int32_t *__restrict__ new_coords, long long M,
                                                               int32_t *__restrict__ idx) {
  const long long m = (long long)blockIdx.x * (VQ_BLOCK / VQ_GROUP) + threadIdx.x / VQ_GROUP;
  const int lane = threadIdx.x & (VQ_GROUP - 1);
  const bool live = m < M;
  float nx = 0.f, ny = 0.f, nz = 0.f;
  int cb = -1, cz = 0, cy = 0, cx = 0;
  if (live) {
    nx = new_xyz[m * 3 + 0], ny = new_xyz[m * 3 + 1], nz = new_xyz[m * 3 + 2];
    cb = new_coords[m * 4 + 0], cz = new_coords[m * 4 + 1], cy = new_coords[m * 4 + 2], cx = new_coords[m * 4 + 3];
  }
  int32_t *out = idx + (live ? m : 0) * q.nsample;
  int first = -1;
  const int cnt = vq_scan(lk, q, xyz, live, nx, ny, nz, cb, cz, cy, cx, [&](int slot, int row) {
    out[slot] = row;
    if (slot == 0) first = row;
  });
  first = group_max(first);            // rows are >= 0: the lane that wrote slot 0 wins
  if (!live) return;
  // the first hit fills every slot before the later hits overwrite theirs (voxel_query_gpu.cu:69-76); an empty ball is
  // -1 in slot 0 over the zeros the reference's caller allocates
  for (int s = cnt + lane; s < q.nsample; s += VQ_GROUP) out[s] = cnt > 0 ? first : (s == 0 ? -1 : 0);
}

// ---- fused pool: C channels = C / 4 lanes of 16 B per row; 16 / (C / 4) samples are gathered at a time and reduced in
// registers, then across the sub-groups by shuffles.  wpos [C, 4] = (wx, wy, wz, shift) of mlps_pos with its BatchNorm folded.
template <int C, bool AVG>
__global__ __launch_bounds__(VQ_BLOCK) void voxel_pool_fused_kernel(DirectoryLookup lk, QueryGeom q,
                                                                    const float *__restrict__ rows_in,
                                                                    const float *__restrict__ xyz,
                                                                    const float *__restrict__ new_xyz,
                                                                    const int32_t *__restrict__ new_coords, long long M,
                                                                    const float *__restrict__ wpos, float *__restrict__ pooled,
                                                                    int32_t *__restrict__ idx, uint8_t *__restrict__ empty) {
  constexpr int LPR = C / 4;           // lanes per row
  constexpr int NSUB = VQ_GROUP / LPR; // rows gathered at a time
  __shared__ int32_t s_idx[VQ_BLOCK / VQ_GROUP][VP_MAX_NSAMPLE];
  const int grp = threadIdx.x / VQ_GROUP;
  const int lane = threadIdx.x & (VQ_GROUP - 1);
  const long long m = (long long)blockIdx.x * (VQ_BLOCK / VQ_GROUP) + grp;
  const bool live = m < M;
  float nx = 0.f, ny = 0.f, nz = 0.f;
  int cb = -1, cz = 0, cy = 0, cx = 0;
  if (live) {
    nx = new_xyz[m * 3 + 0], ny = new_xyz[m * 3 + 1], nz = new_xyz[m * 3 + 2];
    cb = new_coords[m * 4 + 0], cz = new_coords[m * 4 + 1], cy = new_coords[m * 4 + 2], cx = new_coords[m * 4 + 3];
  }
  int32_t *slots = s_idx[grp];
  const int cnt = vq_scan(lk, q, xyz, live, nx, ny, nz, cb, cz, cy, cx, [&](int slot, int row) { slots[slot] = row; });
  __syncthreads();
  const int sub = lane / LPR, c0 = (lane % LPR) * 4;
  float4 w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = *(const float4 *)(wpos + (size_t)(c0 + i) * 4);
  float acc[4] = {0.f, 0.f, 0.f, 0.f};                       // ReLU outputs are >= 0: 0 is neutral for max as for the sum
  for (int s = sub; s < cnt; s += NSUB) {
    const int row = slots[s];
    const float4 f = *(const float4 *)(rows_in + (size_t)row * C + c0);
    const float px = xyz[(size_t)row * 3 + 0] - nx, py = xyz[(size_t)row * 3 + 1] - ny, pz = xyz[(size_t)row * 3 + 2] - nz;
    const float fv[4] = {f.x, f.y, f.z, f.w};
    // the slots past the hit count repeat the first hit: neutral for max, (nsample - cnt) more copies of it in the mean
    const float weight = AVG && s == 0 ? (float)(q.nsample - cnt + 1) : 1.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float v = fmaxf(fv[i] + (w[i].x * px + w[i].y * py + w[i].z * pz + w[i].w), 0.f);
      acc[i] = AVG ? acc[i] + weight * v : fmaxf(acc[i], v);
    }
  }
#pragma unroll
  for (int d = LPR; d < VQ_GROUP; d <<= 1) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float o = __shfl_xor(acc[i], d, VQ_GROUP);
      acc[i] = AVG ? acc[i] + o : fmaxf(acc[i], o);
    }
  }
  if (!live) return;
  if (sub == 0) {
    float4 o;
    if (cnt == 0) {
      // empty ball: features and relative coordinates are zeroed BEFORE the position branch, so every slot holds relu(shift)
      o = make_float4(fmaxf(w[0].w, 0.f), fmaxf(w[1].w, 0.f), fmaxf(w[2].w, 0.f), fmaxf(w[3].w, 0.f));
    } else {
      const float inv = AVG ? 1.f / (float)q.nsample : 1.f;
      o = make_float4(acc[0] * inv, acc[1] * inv, acc[2] * inv, acc[3] * inv);
    }
    *(float4 *)(pooled + (size_t)m * C + c0) = o;
  }
  if (idx)
    for (int s = lane; s < q.nsample; s += VQ_GROUP)
      idx[m * q.nsample + s] = cnt > 0 ? slots[s < cnt ? s : 0] : (s == 0 ? -1 : 0);
  if (empty && lane == 0) empty[m] = cnt == 0;
}

// ---- stack grouping
// frame of stacked row `m` under per-frame counts, and the first feature row of that frame (group_points_gpu.cu:86-94)
__device__ __forceinline__ void stack_frame(const int32_t *__restrict__ idx_cnt, const int32_t *__restrict__ feat_cnt, int B,
                                            long long m, long long &feat_start, int &feat_n) {
  int b = 0;
  long long end = idx_cnt[0];
  for (int k = 1; k < B; ++k) {
    if (m < end) break;
    end += idx_cnt[k];
    b = k;
  }
  feat_start = 0;
  for (int k = 0; k < b; ++k) feat_start += feat_cnt[k];
  feat_n = feat_cnt[b];
}

__global__ __launch_bounds__(256) void group_points_stack_kernel(const float *__restrict__ features,
                                                                 const int32_t *__restrict__ feat_cnt,
                                                                 const int32_t *__restrict__ idx,
                                                                 const int32_t *__restrict__ idx_cnt, int B, long long M, int C,
                                                                 int nsample, long long N, float *__restrict__ out) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= M * C * nsample) return;
  const int s = (int)(t % nsample);
  const int c = (int)((t / nsample) % C);
  const long long m = t / nsample / C;
  long long start;
  int fn;
  stack_frame(idx_cnt, feat_cnt, B, m, start, fn);
  const int i = idx[m * nsample + s];
  const long long row = start + i;
  // an index outside its frame has no meaning in the reference (it reads whatever lies there): zero, never out of bounds
  out[t] = i >= 0 && i < fn && row < N ? features[row * C + c] : 0.f;
}

// target row of every (m, s) entry, -1 where the index is outside its frame
__global__ __launch_bounds__(256) void group_targets_kernel(const int32_t *__restrict__ idx, const int32_t *__restrict__ idx_cnt,
                                                            const int32_t *__restrict__ feat_cnt, int B, long long M,
                                                            int nsample, long long N, int32_t *__restrict__ target) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= M * nsample) return;
  long long start;
  int fn;
  stack_frame(idx_cnt, feat_cnt, B, t / nsample, start, fn);
  const int i = idx[t];
  const long long row = start + i;
  target[t] = i >= 0 && i < fn && row < N ? (int32_t)row : -1;
}

// one thread per (referenced row, channel): the row's contributions in ascending (m, s) order
__global__ __launch_bounds__(256) void group_grad_rows_kernel(const float *__restrict__ grad_out,
                                                              const int32_t *__restrict__ voxel_rows,
                                                              const int32_t *__restrict__ offsets,
                                                              const int32_t *__restrict__ ids,
                                                              const int32_t *__restrict__ status, int C, int nsample,
                                                              long long N, float *__restrict__ grad_features) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long v = t / C;
  const int c = (int)(t % C);
  if (v >= status[0]) return;
  const int row = voxel_rows[v];
  if (row < 0 || row >= N) return;
  float acc = 0.f;
  for (int p = offsets[v], e = offsets[v + 1]; p < e; ++p) {
    const long long id = ids[p];
    const long long m = id / nsample;
    const int s = (int)(id % nsample);
    acc += grad_out[(m * C + c) * nsample + s];
  }
  grad_features[(long long)row * C + c] = acc;
}

struct GradWs {
  int32_t *target, *voxel_rows, *p2v, *count, *offsets, *ids, *status;
  void *plan;
  size_t plan_bytes, bytes;
};

int grad_layout(long long n, void *ws, size_t ws_bytes, GradWs &w, void *stream) {
  w.plan_bytes = df3d_dynamic_scatter_plan_workspace_bytes(n, stream);
  if (w.plan_bytes == 0) {
    set_error("group_points_stack_grad: no plan workspace for %lld entries (1 <= M * nsample < 2^31)", n);
    return DF3D_EINVAL;
  }
  size_t need = 0;
  for (int i = 0; i < 4; ++i) need = arena_need(need, (size_t)n * 4);   // target, voxel_rows, p2v, count
  need = arena_need(need, (size_t)(n + 1) * 4);                         // offsets
  need = arena_need(need, (size_t)n * 4);                               // ids
  need = arena_need(need, 2 * 4);                                       // status
  need = arena_need(need, w.plan_bytes);
  w.bytes = need;
  if (!ws) return DF3D_OK;
  Arena a(ws, ws_bytes);
  w.target = a.take<int32_t>(n);
  w.voxel_rows = a.take<int32_t>(n);
  w.p2v = a.take<int32_t>(n);
  w.count = a.take<int32_t>(n);
  w.offsets = a.take<int32_t>(n + 1);
  w.ids = a.take<int32_t>(n);
  w.status = a.take<int32_t>(2);
  w.plan = a.take<char>(w.plan_bytes);
  if (!w.plan) {
    set_error("group_points_stack_grad: workspace too small (%zu < %zu)", ws_bytes, need);
    return DF3D_ENOMEM;
  }
  return DF3D_OK;
}

int fill_geom(QueryGeom &q, const char *what, int batch, const int *shape, const int *range, float radius, int nsample,
              long long n_rows, long long M) {
  DF3D_CHECK_ARG(batch > 0 && shape[0] > 0 && shape[1] > 0 && shape[2] > 0, "%s: bad grid [%d][%d,%d,%d]", what, batch,
                 shape[0], shape[1], shape[2]);
  DF3D_CHECK_ARG(range[0] >= 0 && range[1] >= 0 && range[2] >= 0, "%s: negative query range", what);
  DF3D_CHECK_ARG(range[2] <= VQ_MAX_XRANGE, "%s: x query range %d is above the limit of %d cells (the x-run of a row is one 32-bit mask)",
                 what, range[2], VQ_MAX_XRANGE);
  DF3D_CHECK_ARG(range[0] <= 1024 && range[1] <= 1024, "%s: z / y query range above the limit of 1024 cells", what);
  DF3D_CHECK_ARG(nsample >= 1 && nsample <= 4096, "%s: nsample %d outside 1..4096", what, nsample);
  DF3D_CHECK_ARG(n_rows >= 0 && n_rows < (1ll << 31) && M >= 0 && M * nsample < (1ll << 40), "%s: bad sizes", what);
  DF3D_CHECK_ARG(radius >= 0.f, "%s: negative radius", what);
  q.batch = batch, q.Z = shape[0], q.Y = shape[1], q.X = shape[2];
  q.rz = range[0], q.ry = range[1], q.rx = range[2];
  q.nsample = nsample;
  q.radius2 = radius * radius;
  q.n_rows = n_rows;
  return DF3D_OK;
}

}  // namespace
}  // namespace df3d

using namespace df3d;

extern "C" int df3d_voxel_query(const void *grid, const int32_t *perm, int batch, const int *shape, const float *xyz,
                                long long n_rows, const float *new_xyz, const int32_t *new_coords, long long M,
                                const int *range, float radius, int nsample, int32_t *idx, void *stream) {
  DF3D_CHECK_ARG(grid && shape && xyz && new_xyz && new_coords && range && idx, "voxel_query: null argument");
  QueryGeom q;
  int rc = fill_geom(q, "voxel_query", batch, shape, range, radius, nsample, n_rows, M);
  if (rc) return rc;
  if (M == 0) return DF3D_OK;
  GridHeader h = grid_layout(batch, shape);
  DirectoryLookup lk;
  lk.g = grid_view(grid, h);
  lk.perm = perm;
  hipLaunchKernelGGL(voxel_query_kernel<DirectoryLookup>, dim3(cdiv(M, VQ_BLOCK / VQ_GROUP)), dim3(VQ_BLOCK), 0,
                     (hipStream_t)stream, lk, q, xyz, new_xyz, new_coords, M, idx);
  DF3D_LAUNCH_CHECK();
  return DF3D_OK;
}

extern "C" int df3d_voxel_query_dense(const int32_t *point_indices, int batch, const int *shape, const float *xyz,
                                      long long n_rows, const float *new_xyz, const int32_t *new_coords, long long M,
                                      const int *range, float radius, int nsample, int32_t *idx, void *stream) {
  DF3D_CHECK_ARG(point_indices && shape && xyz && new_xyz && new_coords && range && idx, "voxel_query_dense: null argument");
  QueryGeom q;
  int rc = fill_geom(q, "voxel_query_dense", batch, shape, range, radius, nsample, n_rows, M);
  if (rc) return rc;
  if (M == 0) return DF3D_OK;
  DenseLookup lk;
  lk.cells = point_indices;
  lk.Z = shape[0], lk.Y = shape[1], lk.X = shape[2];
  lk.run = nullptr;
  hipLaunchKernelGGL(voxel_query_kernel<DenseLookup>, dim3(cdiv(M, VQ_BLOCK / VQ_GROUP)), dim3(VQ_BLOCK), 0,
                     (hipStream_t)stream, lk, q, xyz, new_xyz, new_coords, M, idx);
  DF3D_LAUNCH_CHECK();
  return DF3D_OK;
}

extern "C" int df3d_group_points_stack(const float *features, const int32_t *features_batch_cnt, const int32_t *idx,
                                       const int32_t *idx_batch_cnt, int B, long long M, int C, int nsample, long long N,
                                       float *out, void *stream) {
  DF3D_CHECK_ARG(features && features_batch_cnt && idx && idx_batch_cnt && out, "group_points_stack: null argument");
  DF3D_CHECK_ARG(B >= 1 && M >= 0 && C >= 1 && nsample >= 1 && N >= 0, "group_points_stack: bad sizes");
  const long long total = M * C * nsample;
  DF3D_CHECK_ARG(total < (1ll << 39), "group_points_stack: M * C * nsample = %lld is above the limit of 2^39", total);
  if (total == 0) return DF3D_OK;
  hipLaunchKernelGGL(group_points_stack_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, features,
                     features_batch_cnt, idx, idx_batch_cnt, B, M, C, nsample, N, out);
  DF3D_LAUNCH_CHECK();
  return DF3D_OK;
}

extern "C" size_t df3d_group_points_stack_grad_workspace_bytes(long long M, int nsample, void *stream) {
  if (M <= 0 || nsample <= 0 || M * nsample >= (1ll << 31)) return 0;
  GradWs w;
  if (grad_layout(M * nsample, nullptr, 0, w, stream) != DF3D_OK) return 0;
  return w.bytes;
}

extern "C" int df3d_group_points_stack_grad(const float *grad_out, const int32_t *idx, const int32_t *idx_batch_cnt,
                                            const int32_t *features_batch_cnt, int B, long long M, int C, long long N,
                                            int nsample, float *grad_features, void *workspace, size_t workspace_bytes,
                                            void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  DF3D_CHECK_ARG(grad_out && idx && idx_batch_cnt && features_batch_cnt && grad_features,
                 "group_points_stack_grad: null argument");
  DF3D_CHECK_ARG(B >= 1 && M >= 0 && C >= 1 && nsample >= 1 && N >= 0, "group_points_stack_grad: bad sizes");
  const long long n = M * nsample;
  DF3D_CHECK_ARG(n < (1ll << 31), "group_points_stack_grad: M * nsample = %lld is above the limit of 2^31 - 1", n);
  if (N * C == 0) return DF3D_OK;
  DF3D_HIP(hipMemsetAsync(grad_features, 0, (size_t)N * C * sizeof(float), stream));   // rows nobody refers to: exactly 0
  if (n == 0) return DF3D_OK;
  DF3D_CHECK_ARG(workspace, "group_points_stack_grad: null workspace");
  GradWs w;
  int rc = grad_layout(n, workspace, workspace_bytes, w, stream_);
  if (rc) return rc;
  hipLaunchKernelGGL(group_targets_kernel, dim3(cdiv(n, 256)), dim3(256), 0, stream, idx, idx_batch_cnt, features_batch_cnt, B,
                     M, nsample, N, w.target);
  DF3D_LAUNCH_CHECK();
  rc = df3d_dynamic_scatter_plan(w.target, n, 1, w.voxel_rows, w.p2v, w.count, w.offsets, w.ids, w.status, w.plan,
                                 w.plan_bytes, stream_);
  if (rc) return rc;
  // at most min(n, N) distinct rows; the count stays on the device (status[0])
  const long long vmax = n < N ? n : N;
  hipLaunchKernelGGL(group_grad_rows_kernel, dim3(cdiv(vmax * C, 256)), dim3(256), 0, stream, grad_out, w.voxel_rows, w.offsets,
                     w.ids, w.status, C, nsample, N, grad_features);
  DF3D_LAUNCH_CHECK();
  return DF3D_OK;
}

extern "C" int df3d_voxel_pool_fused(const float *rows_in, const float *xyz, long long n_rows, int C, const void *grid,
                                     const int32_t *perm, int batch, const int *shape, const float *new_xyz,
                                     const int32_t *new_coords, long long M, const int *range, float radius, int nsample,
                                     const float *w_pos, int pool_method, float *pooled, int32_t *idx, uint8_t *empty,
                                     void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  DF3D_CHECK_ARG(rows_in && xyz && grid && shape && new_xyz && new_coords && range && w_pos && pooled,
                 "voxel_pool_fused: null argument");
  DF3D_CHECK_ARG(C == 16 || C == 32 || C == 64, "voxel_pool_fused: C = %d, the kernel serves 16, 32 and 64 channels", C);
  DF3D_CHECK_ARG(pool_method == 0 || pool_method == 1, "voxel_pool_fused: pool method must be 0 (max_pool) or 1 (avg_pool)");
  DF3D_CHECK_ARG(nsample >= 1 && nsample <= VP_MAX_NSAMPLE, "voxel_pool_fused: nsample %d is above the limit of %d", nsample,
                 VP_MAX_NSAMPLE);
  DF3D_CHECK_ARG(((uintptr_t)rows_in | (uintptr_t)w_pos | (uintptr_t)pooled) % 16 == 0,
                 "voxel_pool_fused: rows_in, w_pos and pooled must be 16-byte aligned");
  QueryGeom q;
  int rc = fill_geom(q, "voxel_pool_fused", batch, shape, range, radius, nsample, n_rows, M);
  if (rc) return rc;
  if (M == 0) return DF3D_OK;
  GridHeader h = grid_layout(batch, shape);
  DirectoryLookup lk;
  lk.g = grid_view(grid, h);
  lk.perm = perm;
  const dim3 gridDim3(cdiv(M, VQ_BLOCK / VQ_GROUP)), block(VQ_BLOCK);
#define DF3D_VP_LAUNCH(CC, AVG)                                                                                              \
  hipLaunchKernelGGL((voxel_pool_fused_kernel<CC, AVG>), gridDim3, block, 0, stream, lk, q, rows_in, xyz, new_xyz, new_coords, \
                     M, w_pos, pooled, idx, empty)
  if (C == 16) {
    if (pool_method) DF3D_VP_LAUNCH(16, true); else DF3D_VP_LAUNCH(16, false);
  } else if (C == 32) {
    if (pool_method) DF3D_VP_LAUNCH(32, true); else DF3D_VP_LAUNCH(32, false);
  } else {
    if (pool_method) DF3D_VP_LAUNCH(64, true); else DF3D_VP_LAUNCH(64, false);
  }
#undef DF3D_VP_LAUNCH
  DF3D_LAUNCH_CHECK();
  return DF3D_OK;
}
