// DynamicScatter on the device (df3d_hip.h: "Dynamic scatter"): a plan over per-point voxel coordinates, the ordered
// per-voxel reduce of point rows, and the gathers / scatters of its backward.
//
// Plan.  key(p) = the row of point p linearised over (max + 1) per column, first column most significant (64 bits; a
// product that needs more than 63 bits is reported, never wrapped); rows with a negative entry get the all-ones key.  A
// stable radix sort of (key, p) puts equal rows next to each other with their point ids ascending, invalid rows last; the
// heads of the runs, scanned, number the voxels in ascending lexicographic order.  Nothing of size N passes through the host;
// the host reads {M, overflow} once.
//
// Reduce.  Lanes of a wave are (point slot, channel): G = the power of two >= min(C, 64) channel lanes, P = 64 / G slots.
// A voxel of n <= DS_LONG points belongs to one wave: slot s adds the points s, s + P, s + 2P, ... of the voxel's ascending
// list in that order and the P partial sums are added by a halving tree.  A longer voxel is taken by the four waves of the
// block together (4P slots, the same strided order, the same tree, then the four wave sums left to right through LDS).
// Which path a voxel takes and the order inside it depend on (n, C) alone, so a sum repeats bit for bit.  No floating-point
// atomics anywhere; every valid point row is read once.
#include <rocprim/device/device_radix_sort.hpp>

#include "common.h"

namespace df3d {
namespace {

constexpr unsigned long long DS_INVALID = ~0ull;
constexpr int DS_LONG = 64;          // voxels with more points are reduced by the whole block
constexpr int DS_VPB = 16;           // voxels per block of the reduce
constexpr int DS_WAVES = 4;

struct DsDims {
  unsigned long long d[4];           // max + 1 per column (0: no valid row)
  int overflow;
};

// per-column maximum over the valid rows (maxs[] starts at -1)
__global__ __launch_bounds__(256) void ds_colmax_kernel(const int32_t *__restrict__ coors, long long n, int ndim,
                                                        int *__restrict__ maxs) {
  int m[4] = {-1, -1, -1, -1};
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (long long)gridDim.x * blockDim.x) {
    int r[4];
    bool ok = true;
    for (int k = 0; k < ndim; ++k) r[k] = coors[p * ndim + k], ok = ok && r[k] >= 0;
    if (ok)
      for (int k = 0; k < ndim; ++k) m[k] = max(m[k], r[k]);
  }
  for (int k = 0; k < ndim; ++k) {
    int v = m[k];
    for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d));
    if ((threadIdx.x & 63) == 0 && v >= 0) atomicMax(&maxs[k], v);
  }
}

__device__ __forceinline__ DsDims ds_dims(const int *__restrict__ maxs, int ndim) {
  DsDims r;
  unsigned long long prod = 1;
  r.overflow = 0;
  for (int k = 0; k < 4; ++k) r.d[k] = 1;
  for (int k = 0; k < ndim; ++k) {
    r.d[k] = (unsigned long long)((long long)maxs[k] + 1);
    if (__umul64hi(prod, r.d[k]) != 0) r.overflow = 1;
    prod *= r.d[k];
    if (prod >> 63) r.overflow = 1;
  }
  return r;
}

__global__ __launch_bounds__(256) void ds_keys_kernel(const int32_t *__restrict__ coors, long long n, int ndim,
                                                      const int *__restrict__ maxs, unsigned long long *__restrict__ keys,
                                                      int32_t *__restrict__ ids, int32_t *__restrict__ status) {
  const DsDims dm = ds_dims(maxs, ndim);
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p == 0) status[1] = dm.overflow;
  if (p >= n) return;
  unsigned long long key = 0;
  bool ok = !dm.overflow;
  for (int k = 0; k < ndim; ++k) {
    const int c = coors[p * ndim + k];
    ok = ok && c >= 0;
    key = key * dm.d[k] + (unsigned long long)(unsigned)c;
  }
  keys[p] = ok ? key : DS_INVALID;
  ids[p] = (int32_t)p;
}

__global__ __launch_bounds__(256) void ds_heads_kernel(const unsigned long long *__restrict__ keys, long long n,
                                                       uint32_t *__restrict__ flag) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned long long k = keys[i];
  flag[i] = (k != DS_INVALID && (i == 0 || keys[i - 1] != k)) ? 1u : 0u;
}

// rank[i] = number of run heads before sorted position i
__global__ __launch_bounds__(256) void ds_fill_kernel(const unsigned long long *__restrict__ keys,
                                                      const int32_t *__restrict__ ids, const uint32_t *__restrict__ rank,
                                                      const uint32_t *__restrict__ total, long long n, int ndim,
                                                      const int *__restrict__ maxs, int32_t *__restrict__ voxel_coors,
                                                      int32_t *__restrict__ map, int32_t *__restrict__ offsets,
                                                      int32_t *__restrict__ status) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) offsets[0] = 0, status[0] = (int32_t)*total;
  if (i >= n) return;
  const unsigned long long k = keys[i];
  const int p = ids[i];
  if (k == DS_INVALID) {
    map[p] = -1;
    return;
  }
  const bool head = i == 0 || keys[i - 1] != k;
  const bool tail = i == n - 1 || keys[i + 1] != k;
  const int v = (int)rank[i] - (head ? 0 : 1);
  map[p] = v;
  if (tail) offsets[v + 1] = (int32_t)(i + 1);
  if (head) {
    const DsDims dm = ds_dims(maxs, ndim);
    unsigned long long rest = k;
    for (int c = ndim - 1; c >= 0; --c) {
      voxel_coors[(long long)v * ndim + c] = (int32_t)(rest % dm.d[c]);
      rest /= dm.d[c];
    }
  }
}

__global__ __launch_bounds__(256) void ds_counts_kernel(const int32_t *__restrict__ offsets, const uint32_t *__restrict__ total,
                                                        long long n, int32_t *__restrict__ counts) {
  const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (v < n && v < (long long)*total) counts[v] = offsets[v + 1] - offsets[v];
}

// ---------------------------------------------------------------------------------------------------------- reduce
enum { DS_SUM = 0, DS_MEAN = 1, DS_MAX = 2 };

template <typename T>
__device__ __forceinline__ T ds_shfl_down(T v, int d) {
  return __shfl_down(v, d);
}

template <typename T, int MODE>
__device__ __forceinline__ T ds_op(T a, T b) {
  return MODE == DS_MAX ? (b > a ? b : a) : a + b;
}

// partial of the points b + slot, b + slot + stride, ... below e, for channel c (act: the lane has a channel)
template <typename T, int MODE>
__device__ __forceinline__ T ds_strided(const T *__restrict__ feats, const int32_t *__restrict__ ids, int b, int e, int slot,
                                        int stride, int C, int c, bool act) {
  T acc = MODE == DS_MAX ? -(T)INFINITY : (T)0;
  int i = b + slot;
  // four independent row loads in flight per slot; they are added in ascending order
  for (; i + 3 * stride < e; i += 4 * stride) {
    const int p0 = ids[i], p1 = ids[i + stride], p2 = ids[i + 2 * stride], p3 = ids[i + 3 * stride];
    T x0 = 0, x1 = 0, x2 = 0, x3 = 0;
    if (act) {
      x0 = feats[(long long)p0 * C + c], x1 = feats[(long long)p1 * C + c];
      x2 = feats[(long long)p2 * C + c], x3 = feats[(long long)p3 * C + c];
    }
    acc = ds_op<T, MODE>(ds_op<T, MODE>(ds_op<T, MODE>(ds_op<T, MODE>(acc, x0), x1), x2), x3);
  }
  for (; i < e; i += stride) {
    const int p0 = ids[i];
    const T x0 = act ? feats[(long long)p0 * C + c] : (T)0;
    acc = ds_op<T, MODE>(acc, x0);
  }
  return acc;
}

template <typename T, int MODE>
__global__ __launch_bounds__(64 * DS_WAVES) void ds_reduce_kernel(const T *__restrict__ feats, int C,
                                                                  const int32_t *__restrict__ ids,
                                                                  const int32_t *__restrict__ offsets, int M, int lg,
                                                                  T *__restrict__ out) {
  __shared__ T part[DS_WAVES][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int G = 1 << lg, P = 64 >> lg;
  const int slot = lane >> lg, c0 = lane & (G - 1);
  const int vbase = blockIdx.x * DS_VPB;
  const int vend = min(vbase + DS_VPB, M);
  for (int cc = 0; cc < C; cc += G) {
    const int c = cc + c0;
    const bool act = c < C;
    // voxels of one wave
    for (int v = vbase + wave; v < vend; v += DS_WAVES) {
      const int b = offsets[v], e = offsets[v + 1];
      if (e - b > DS_LONG) continue;
      T acc = ds_strided<T, MODE>(feats, ids, b, e, slot, P, C, c, act);
      for (int d = P >> 1; d >= 1; d >>= 1) acc = ds_op<T, MODE>(acc, ds_shfl_down(acc, d << lg));
      if (slot == 0 && act) out[(long long)v * C + c] = MODE == DS_MEAN ? acc / (T)(e - b) : acc;
    }
    // voxels of the whole block (every thread sees the same v, b, e: the barriers are uniform)
    for (int v = vbase; v < vend; ++v) {
      const int b = offsets[v], e = offsets[v + 1];
      if (e - b <= DS_LONG) continue;
      T acc = ds_strided<T, MODE>(feats, ids, b, e, wave * P + slot, DS_WAVES * P, C, c, act);
      for (int d = P >> 1; d >= 1; d >>= 1) acc = ds_op<T, MODE>(acc, ds_shfl_down(acc, d << lg));
      if (slot == 0) part[wave][c0] = acc;
      __syncthreads();
      if (wave == 0 && slot == 0 && act) {
        T r = part[0][c0];
        for (int w = 1; w < DS_WAVES; ++w) r = ds_op<T, MODE>(r, part[w][c0]);
        out[(long long)v * C + c] = MODE == DS_MEAN ? r / (T)(e - b) : r;
      }
      __syncthreads();
    }
  }
}

// out[p] = rows[map[p]] (/ count[map[p]] when counts is given), zero rows for map[p] < 0
template <typename T>
__global__ __launch_bounds__(256) void ds_gather_kernel(const T *__restrict__ rows, const int32_t *__restrict__ map,
                                                        const int32_t *__restrict__ counts, long long total, int C,
                                                        T *__restrict__ out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const long long p = i / C;
  const int c = (int)(i - p * C);
  const int v = map[p];
  T r = 0;
  if (v >= 0) {
    r = rows[(long long)v * C + c];
    if (counts) r = r / (T)counts[v];
  }
  out[i] = r;
}

// arg[v, c] = lowest point index whose feature equals the voxel's maximum (arg starts at INT_MAX)
template <typename T>
__global__ __launch_bounds__(256) void ds_argmax_kernel(const T *__restrict__ feats, const T *__restrict__ vfeats,
                                                        const int32_t *__restrict__ map, long long total, int C,
                                                        int32_t *__restrict__ arg) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const long long p = i / C;
  const int c = (int)(i - p * C);
  const int v = map[p];
  if (v < 0) return;
  if (feats[i] == vfeats[(long long)v * C + c]) atomicMin(&arg[(long long)v * C + c], (int32_t)p);
}

template <typename T>
__global__ __launch_bounds__(256) void ds_max_scatter_kernel(const T *__restrict__ grad_v, const int32_t *__restrict__ arg,
                                                             long long total, int C, long long n, T *__restrict__ grad_feats) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % C);
  const long long p = arg[i];
  if (p < n) grad_feats[p * C + c] = grad_v[i];
}

struct PlanWs {
  int *maxs;
  unsigned long long *keys_in, *keys_out;
  int32_t *ids_in;
  uint32_t *flag, *total;
  void *scan, *sort;
  size_t scan_bytes, sort_bytes, bytes;
};

int plan_layout(long long n, void *base, size_t have, PlanWs &w, hipStream_t stream) {
  size_t sort_bytes = 0;
  hipError_t e = rocprim::radix_sort_pairs<rocprim::default_config, unsigned long long *, unsigned long long *, int32_t *,
                                           int32_t *>(nullptr, sort_bytes, nullptr, nullptr, nullptr, nullptr, (size_t)n, 0,
                                                      64, stream, false);
  if (e != hipSuccess) {
    set_error("radix sort workspace query failed: %s", hipGetErrorString(e));
    return DF3D_EHIP;
  }
  w.sort_bytes = sort_bytes;
  w.scan_bytes = scan_scratch_bytes((size_t)n);
  size_t need = 0;
  need = arena_need(need, 4 * sizeof(int));
  need = arena_need(need, (size_t)n * 8);
  need = arena_need(need, (size_t)n * 8);
  need = arena_need(need, (size_t)n * 4);
  need = arena_need(need, (size_t)n * 4);
  need = arena_need(need, 4);
  need = arena_need(need, w.scan_bytes);
  need = arena_need(need, w.sort_bytes);
  w.bytes = need + 256;
  if (!base) return DF3D_OK;
  Arena a(base, have);
  w.maxs = a.take<int>(4);
  w.keys_in = a.take<unsigned long long>((size_t)n);
  w.keys_out = a.take<unsigned long long>((size_t)n);
  w.ids_in = a.take<int32_t>((size_t)n);
  w.flag = a.take<uint32_t>((size_t)n);
  w.total = a.take<uint32_t>(1);
  w.scan = a.take<char>(w.scan_bytes ? w.scan_bytes : 1);
  w.sort = a.take<char>(w.sort_bytes ? w.sort_bytes : 1);
  if (!w.maxs || !w.keys_in || !w.keys_out || !w.ids_in || !w.flag || !w.total || !w.scan || !w.sort) {
    set_error("dynamic_scatter_plan: workspace too small (%zu bytes given, %zu needed)", have, w.bytes);
    return DF3D_ENOMEM;
  }
  return DF3D_OK;
}

template <typename T>
int reduce_launch(const T *feats, int C, const int32_t *ids, const int32_t *offsets, int M, int reduce, T *out,
                  hipStream_t stream) {
  int lg = 0;
  while ((1 << lg) < C && lg < 6) ++lg;
  const dim3 grid(cdiv(M, DS_VPB)), block(64 * DS_WAVES);
  if (reduce == DS_SUM)
    hipLaunchKernelGGL((ds_reduce_kernel<T, DS_SUM>), grid, block, 0, stream, feats, C, ids, offsets, M, lg, out);
  else if (reduce == DS_MEAN)
    hipLaunchKernelGGL((ds_reduce_kernel<T, DS_MEAN>), grid, block, 0, stream, feats, C, ids, offsets, M, lg, out);
  else
    hipLaunchKernelGGL((ds_reduce_kernel<T, DS_MAX>), grid, block, 0, stream, feats, C, ids, offsets, M, lg, out);
  DF3D_LAUNCH_CHECK();
  return DF3D_OK;
}

template <typename T>
int max_backward_launch(const T *feats, const T *vfeats, const T *grad_v, long long n, int M, int C, const int32_t *map,
                        int32_t *arg, T *grad_feats, hipStream_t stream) {
  DF3D_HIP(hipMemsetAsync(grad_feats, 0, (size_t)n * C * sizeof(T), stream));
  if (M == 0) return DF3D_OK;
  DF3D_HIP(hipMemsetAsync(arg, 0x7f, (size_t)M * C * sizeof(int32_t), stream));      // 0x7f7f7f7f > any point index
  hipLaunchKernelGGL((ds_argmax_kernel<T>), dim3(cdiv(n * C, 256)), dim3(256), 0, stream, feats, vfeats, map, n * C, C, arg);
  DF3D_LAUNCH_CHECK();
  hipLaunchKernelGGL((ds_max_scatter_kernel<T>), dim3(cdiv((long long)M * C, 256)), dim3(256), 0, stream, grad_v, arg,
                     (long long)M * C, C, n, grad_feats);
  DF3D_LAUNCH_CHECK();
  return DF3D_OK;
}

}  // namespace
}  // namespace df3d

using namespace df3d;

extern "C" size_t df3d_dynamic_scatter_plan_workspace_bytes(long long num_points, void *stream) {
  if (num_points <= 0 || num_points >= (1ll << 31)) return 0;
  PlanWs w;
  if (plan_layout(num_points, nullptr, 0, w, (hipStream_t)stream) != DF3D_OK) return 0;
  return w.bytes;
}

extern "C" int df3d_dynamic_scatter_plan(const int32_t *coors, long long num_points, int ndim, int32_t *voxel_coors,
                                         int32_t *point2voxel_map, int32_t *voxel_points_count, int32_t *offsets,
                                         int32_t *point_ids, int32_t *status, void *workspace, size_t workspace_bytes,
                                         void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  DF3D_CHECK_ARG(num_points > 0 && num_points < (1ll << 31), "dynamic_scatter_plan: 1 <= num_points < 2^31 (got %lld)",
                 num_points);
  DF3D_CHECK_ARG(ndim >= 1 && ndim <= 4, "dynamic_scatter_plan: coors must have 1..4 columns (got %d)", ndim);
  DF3D_CHECK_ARG(coors && voxel_coors && point2voxel_map && voxel_points_count && offsets && point_ids && status && workspace,
                 "dynamic_scatter_plan: null pointer");
  const long long n = num_points;
  PlanWs w;
  int rc = plan_layout(n, workspace, workspace_bytes, w, stream);
  if (rc != DF3D_OK) return rc;
  DF3D_HIP(hipMemsetAsync(w.maxs, 0xff, 4 * sizeof(int), stream));
  const int nb = cdiv(n, 256);
  hipLaunchKernelGGL(ds_colmax_kernel, dim3(nb < 1024 ? nb : 1024), dim3(256), 0, stream, coors, n, ndim, w.maxs);
  DF3D_LAUNCH_CHECK();
  hipLaunchKernelGGL(ds_keys_kernel, dim3(nb), dim3(256), 0, stream, coors, n, ndim, w.maxs, w.keys_in, w.ids_in, status);
  DF3D_LAUNCH_CHECK();
  size_t sort_bytes = w.sort_bytes;
  DF3D_HIP(rocprim::radix_sort_pairs(w.sort, sort_bytes, w.keys_in, w.keys_out, w.ids_in, point_ids, (size_t)n, 0, 64, stream,
                                     false));
  hipLaunchKernelGGL(ds_heads_kernel, dim3(nb), dim3(256), 0, stream, w.keys_out, n, w.flag);
  DF3D_LAUNCH_CHECK();
  rc = exclusive_scan_u32(w.flag, w.flag, (size_t)n, w.total, w.scan, w.scan_bytes, stream);
  if (rc != DF3D_OK) return rc;
  hipLaunchKernelGGL(ds_fill_kernel, dim3(nb), dim3(256), 0, stream, w.keys_out, point_ids, w.flag, w.total, n, ndim, w.maxs,
                     voxel_coors, point2voxel_map, offsets, status);
  DF3D_LAUNCH_CHECK();
  hipLaunchKernelGGL(ds_counts_kernel, dim3(nb), dim3(256), 0, stream, offsets, w.total, n, voxel_points_count);
  DF3D_LAUNCH_CHECK();
  return DF3D_OK;
}

extern "C" int df3d_dynamic_scatter_reduce(const void *feats, int is_double, int channels, const int32_t *point_ids,
                                           const int32_t *offsets, int num_voxels, int reduce, void *out, void *stream) {
  DF3D_CHECK_ARG(reduce >= DS_SUM && reduce <= DS_MAX, "dynamic_scatter_reduce: reduce must be 0 (sum), 1 (mean) or 2 (max)");
  DF3D_CHECK_ARG(channels >= 1 && num_voxels >= 1, "dynamic_scatter_reduce: channels and num_voxels must be positive");
  DF3D_CHECK_ARG(feats && point_ids && offsets && out, "dynamic_scatter_reduce: null pointer");
  if (is_double)
    return reduce_launch<double>((const double *)feats, channels, point_ids, offsets, num_voxels, reduce, (double *)out,
                                 (hipStream_t)stream);
  return reduce_launch<float>((const float *)feats, channels, point_ids, offsets, num_voxels, reduce, (float *)out,
                              (hipStream_t)stream);
}

extern "C" int df3d_voxel_to_point(const void *voxel_rows, int is_double, int channels, const int32_t *point2voxel_map,
                                   const int32_t *divide_by_count, long long num_points, void *out, void *stream) {
  DF3D_CHECK_ARG(channels >= 1 && num_points >= 1, "voxel_to_point: channels and num_points must be positive");
  DF3D_CHECK_ARG(point2voxel_map && out, "voxel_to_point: null pointer");
  const long long total = num_points * channels;
  if (is_double)
    hipLaunchKernelGGL((ds_gather_kernel<double>), dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const double *)voxel_rows, point2voxel_map, divide_by_count, total, channels, (double *)out);
  else
    hipLaunchKernelGGL((ds_gather_kernel<float>), dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const float *)voxel_rows, point2voxel_map, divide_by_count, total, channels, (float *)out);
  DF3D_LAUNCH_CHECK();
  return DF3D_OK;
}

extern "C" int df3d_dynamic_scatter_max_backward(const void *feats, const void *voxel_feats, const void *grad_voxel_feats,
                                                 int is_double, long long num_points, int num_voxels, int channels,
                                                 const int32_t *point2voxel_map, int32_t *arg_workspace, void *grad_feats,
                                                 void *stream) {
  DF3D_CHECK_ARG(channels >= 1 && num_points >= 1 && num_voxels >= 0, "dynamic_scatter_max_backward: bad sizes");
  DF3D_CHECK_ARG(feats && point2voxel_map && grad_feats && (num_voxels == 0 || (voxel_feats && grad_voxel_feats && arg_workspace)),
                 "dynamic_scatter_max_backward: null pointer");
  if (is_double)
    return max_backward_launch<double>((const double *)feats, (const double *)voxel_feats, (const double *)grad_voxel_feats,
                                       num_points, num_voxels, channels, point2voxel_map, arg_workspace, (double *)grad_feats,
                                       (hipStream_t)stream);
  return max_backward_launch<float>((const float *)feats, (const float *)voxel_feats, (const float *)grad_voxel_feats,
                                    num_points, num_voxels, channels, point2voxel_map, arg_workspace, (float *)grad_feats,
                                    (hipStream_t)stream);
}
