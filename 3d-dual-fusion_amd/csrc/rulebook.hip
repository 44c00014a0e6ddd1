// Sparse-convolution rulebooks for gfx950.
//
// The reference (TF/mmdet3d/ops/spconv/include/spconv/indice.cu.h:24-203, spconv_ops.h:27-141)
// fills a dense int32 grid of B*Z*Y*X cells with -1 on every call (340 MB per sample at
// 0.075 m), enumerates neighbours with per-offset atomic counters (non-deterministic pair
// order) and, for strided convs, sorts 27*N candidate outputs with torch::_unique.
//
// Here a voxel set is indexed by an *occupancy directory*: one bit per cell plus an
// exclusive popcount prefix per 64-cell word (12 B per 64 cells = 16 MB per sample at
// 41x1440x1440).  rank(cell) = prefix[word] + popc(bits below) is
//   * a two-read lookup "which row holds voxel (b,z,y,x)" (through `perm` when the rows are
//     not in flat-index order, as after voxelisation), and
//   * for a strided conv, the sorted, duplicate-free list of active outputs for free (the
//     order the reference's GPU path gets from its device sort) - no sort, no hash probing.
// The conv kernels consume an output-stationary neighbour table nbr[K][N_out] (int32,
// -1 = no input), which is deterministic by construction (no atomics in its values).
// The reference-format rulebook (indice_pairs[K,2,N], indice_num[K]) is derived from it
// on request for API parity.
//
// Algorithmic bytes: 16*N_in (read idx) + 8*R (pairs) + 16*N_out; the nbr
// table costs 4*K*N_out instead of 8*R.  All kernels are HBM/latency bound.
#include "common.h"

namespace df3d {

GridHeader grid_layout(int batch, const int *shape) {
  GridHeader h;
  h.batch = batch;
  h.shape[0] = shape[0];
  h.shape[1] = shape[1];
  h.shape[2] = shape[2];
  h.ncells = (unsigned long long)batch * shape[0] * shape[1] * shape[2];
  h.nwords = (h.ncells + 63) / 64;
  size_t off = align_up(sizeof(GridHeader), 256);
  h.off_bits = off;
  off = align_up(off + h.nwords * 8, 256);
  h.off_prefix = off;
  off = align_up(off + h.nwords * 4, 256);
  h.off_total = off;
  off = align_up(off + 64, 256);
  h.off_scratch = off;
  h.scratch_bytes = scan_scratch_bytes(h.nwords);
  return h;
}

struct Shape3 {
  int v[3];
};

__global__ __launch_bounds__(256) void grid_setbits_kernel(const int32_t *__restrict__ ind, int n, Shape3 shp,
                                                           long long vol, unsigned long long *__restrict__ bits) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t *p = ind + (size_t)i * 4;
  long long flat = (long long)p[0] * vol + ((long long)p[1] * shp.v[1] + p[2]) * shp.v[2] + p[3];
  atomicOr(&bits[flat >> 6], 1ull << (flat & 63));
}

__global__ __launch_bounds__(256) void grid_perm_kernel(const int32_t *__restrict__ ind, int n, GridView g,
                                                        int32_t *__restrict__ perm) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t *p = ind + (size_t)i * 4;
  long long flat = (long long)p[0] * g.vol + ((long long)p[1] * g.shape[1] + p[2]) * g.shape[2] + p[3];
  perm[grid_rank(g, flat)] = i;
}

struct ConvGeom {
  int ks[3], st[3], pad[3], dil[3];
  int in_shape[3], out_shape[3];
  int K;
};

// nbr[k][o] for o in [0,n): input cell = out*stride - pad + k*dil
__global__ __launch_bounds__(256) void neighbors_kernel(GridView g, const int32_t *__restrict__ perm,
                                                        const int32_t *__restrict__ out_ind, int n, ConvGeom cg,
                                                        int32_t *__restrict__ nbr) {
  long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)n * cg.K) return;
  int k = (int)(t / n);
  int o = (int)(t - (long long)k * n);
  const int32_t *p = out_ind + (size_t)o * 4;
  int kx = k % cg.ks[2];
  int kt = k / cg.ks[2];
  int ky = kt % cg.ks[1];
  int kz = kt / cg.ks[1];
  int z = p[1] * cg.st[0] - cg.pad[0] + kz * cg.dil[0];
  int y = p[2] * cg.st[1] - cg.pad[1] + ky * cg.dil[1];
  int x = p[3] * cg.st[2] - cg.pad[2] + kx * cg.dil[2];
  int r = -1;
  if (z >= 0 && z < g.shape[0] && y >= 0 && y < g.shape[1] && x >= 0 && x < g.shape[2]) {
    long long flat = (long long)p[0] * g.vol + ((long long)z * g.shape[1] + y) * g.shape[2] + x;
    r = grid_rank(g, flat);
    if (r >= 0 && perm) r = perm[r];
  }
  nbr[t] = r;
}

// mark every output cell touched by an input voxel: out = (in + pad - k*dil) / stride when divisible
__global__ __launch_bounds__(256) void conv_mark_kernel(const int32_t *__restrict__ ind, int n, ConvGeom cg,
                                                        long long out_vol, unsigned long long *__restrict__ bits) {
  // one thread per (voxel, kz, ky): the kx taps land in the same or the next 64-cell word, so they are merged
  // into one mask before the (same-address, serialising) atomic
  const int KZY = cg.ks[0] * cg.ks[1];
  long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)n * KZY) return;
  int i = (int)(t / KZY);
  int kzy = (int)(t - (long long)i * KZY);
  const int32_t *p = ind + (size_t)i * 4;
  int kk[2] = {kzy / cg.ks[1], kzy % cg.ks[1]};
  int o[2];
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    int num = p[1 + d] + cg.pad[d] - kk[d] * cg.dil[d];
    if (num < 0 || (num % cg.st[d]) != 0) return;
    o[d] = num / cg.st[d];
    if (o[d] >= cg.out_shape[d]) return;
  }
  const long long row = (long long)p[0] * out_vol + ((long long)o[0] * cg.out_shape[1] + o[1]) * cg.out_shape[2];
  long long cur = -1;
  unsigned long long mask = 0ull;
  for (int kx = 0; kx < cg.ks[2]; ++kx) {
    int num = p[3] + cg.pad[2] - kx * cg.dil[2];
    if (num < 0 || (num % cg.st[2]) != 0) continue;
    int ox = num / cg.st[2];
    if (ox >= cg.out_shape[2]) continue;
    long long flat = row + ox;
    if ((flat >> 6) != cur) {
      if (mask) atomicOr(&bits[cur], mask);
      cur = flat >> 6;
      mask = 0ull;
    }
    mask |= 1ull << (flat & 63);
  }
  if (mask) atomicOr(&bits[cur], mask);
}

// Transposed convolution (geometry.h:88-142): input voxel `in` writes, through kernel index c, the output cell
// in*stride - pad + c*dil.  One thread per (voxel, cz, cy), the cx taps merged per 64-cell word as above.
__global__ __launch_bounds__(256) void conv_mark_transpose_kernel(const int32_t *__restrict__ ind, int n, ConvGeom cg,
                                                                  long long out_vol,
                                                                  unsigned long long *__restrict__ bits) {
  const int KZY = cg.ks[0] * cg.ks[1];
  long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)n * KZY) return;
  int i = (int)(t / KZY);
  int kzy = (int)(t - (long long)i * KZY);
  const int32_t *p = ind + (size_t)i * 4;
  int kk[2] = {kzy / cg.ks[1], kzy % cg.ks[1]};
  int o[2];
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    o[d] = p[1 + d] * cg.st[d] - cg.pad[d] + kk[d] * cg.dil[d];
    if (o[d] < 0 || o[d] >= cg.out_shape[d]) return;
  }
  const long long row = (long long)p[0] * out_vol + ((long long)o[0] * cg.out_shape[1] + o[1]) * cg.out_shape[2];
  long long cur = -1;
  unsigned long long mask = 0ull;
  for (int kx = 0; kx < cg.ks[2]; ++kx) {
    int ox = p[3] * cg.st[2] - cg.pad[2] + kx * cg.dil[2];
    if (ox < 0 || ox >= cg.out_shape[2]) continue;
    long long flat = row + ox;
    if ((flat >> 6) != cur) {
      if (mask) atomicOr(&bits[cur], mask);
      cur = flat >> 6;
      mask = 0ull;
    }
    mask |= 1ull << (flat & 63);
  }
  if (mask) atomicOr(&bits[cur], mask);
}

// nbr[k][o] of a transposed convolution: the input cell (out + pad - c*dil) / stride when divisible (at most one per
// kernel index, as for the forward convolution)
__global__ __launch_bounds__(256) void neighbors_transpose_kernel(GridView g, const int32_t *__restrict__ perm,
                                                                  const int32_t *__restrict__ out_ind, int n, ConvGeom cg,
                                                                  int32_t *__restrict__ nbr) {
  long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)n * cg.K) return;
  int k = (int)(t / n);
  int o = (int)(t - (long long)k * n);
  const int32_t *p = out_ind + (size_t)o * 4;
  int c[3];
  c[2] = k % cg.ks[2];
  int kt = k / cg.ks[2];
  c[1] = kt % cg.ks[1];
  c[0] = kt / cg.ks[1];
  int in[3];
  bool ok = true;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    int num = p[1 + d] + cg.pad[d] - c[d] * cg.dil[d];
    if (num < 0 || (num % cg.st[d]) != 0) ok = false;
    in[d] = num / cg.st[d];
    if (in[d] >= g.shape[d]) ok = false;
  }
  int r = -1;
  if (ok) {
    long long flat = (long long)p[0] * g.vol + ((long long)in[0] * g.shape[1] + in[1]) * g.shape[2] + in[2];
    r = grid_rank(g, flat);
    if (r >= 0 && perm) r = perm[r];
  }
  nbr[t] = r;
}

// one thread per 64-cell word: emit the coordinates of its set bits at prefix[word]...
__global__ __launch_bounds__(256) void grid_enumerate_kernel(GridView g, unsigned long long nwords,
                                                             int32_t *__restrict__ out_ind, int cap) {
  unsigned long long w = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= nwords) return;
  unsigned long long bits = g.bits[w];
  if (!bits) return;
  uint32_t r = g.prefix[w];
  // decode the word's first cell once (the only divisions), then walk the set bits with carries
  const long long flat0 = (long long)(w << 6);
  const long long yx = (long long)g.shape[1] * g.shape[2];
  int bb = (int)(flat0 / g.vol);
  long long rem = flat0 - (long long)bb * g.vol;
  int z = (int)(rem / yx);
  rem -= (long long)z * yx;
  int y = (int)(rem / g.shape[2]);
  int x = (int)(rem - (long long)y * g.shape[2]);
  int prev = 0;
  while (bits) {
    int b = __ffsll((long long)bits) - 1;
    bits &= bits - 1;
    x += b - prev;
    prev = b;
    while (x >= g.shape[2]) {
      x -= g.shape[2];
      if (++y == g.shape[1]) {
        y = 0;
        if (++z == g.shape[0]) {
          z = 0;
          ++bb;
        }
      }
    }
    if ((int)r < cap) *(int4 *)(out_ind + (size_t)r * 4) = make_int4(bb, z, y, x);
    ++r;
  }
}

__global__ __launch_bounds__(256) void nbr_flag_kernel(const int32_t *__restrict__ nbr, size_t n,
                                                       uint32_t *__restrict__ flag) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) flag[i] = nbr[i] >= 0 ? 1u : 0u;
}

// pairs[k][0][j] = nbr[k][o], pairs[k][1][j] = o with j = rank of o among valid entries of row k
__global__ __launch_bounds__(256) void nbr_compact_kernel(const int32_t *__restrict__ nbr,
                                                          const uint32_t *__restrict__ excl, int K, int n_out,
                                                          int n_in, const uint32_t *__restrict__ total, int32_t *__restrict__ pairs,
                                                          int32_t *__restrict__ num) {
  size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t n = (size_t)K * n_out;
  if (t >= n) return;
  int k = (int)(t / n_out);
  int o = (int)(t - (size_t)k * n_out);
  uint32_t seg0 = excl[(size_t)k * n_out];
  int v = nbr[t];
  if (v >= 0) {
    uint32_t j = excl[t] - seg0;
    if ((int)j < n_in) {
      pairs[((size_t)k * 2 + 0) * n_in + j] = v;
      pairs[((size_t)k * 2 + 1) * n_in + j] = o;
    }
  }
  if (o == 0) {
    uint32_t seg1 = (k + 1 < K) ? excl[(size_t)(k + 1) * n_out] : *total;
    num[k] = (int32_t)(seg1 - seg0);
  }
}

struct NumArr {
  int v[DF3D_MAX_KVOL];
};
__global__ __launch_bounds__(256) void pairs_to_nbr_kernel(const int32_t *__restrict__ pairs, NumArr num, int K,
                                                           int n_in, int n_out, int32_t *__restrict__ nbr) {
  size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)K * n_in) return;
  int k = (int)(t / n_in);
  int j = (int)(t - (size_t)k * n_in);
  if (j >= num.v[k]) return;
  int i = pairs[((size_t)k * 2 + 0) * n_in + j];
  int o = pairs[((size_t)k * 2 + 1) * n_in + j];
  if (o >= 0 && o < n_out) nbr[(size_t)k * n_out + o] = i;
}

static int fill_geom(ConvGeom &cg, const int *ks, const int *st, const int *pad, const int *dil, const int *in_shape,
                     const int *out_shape) {
  cg.K = 1;
  for (int d = 0; d < 3; ++d) {
    cg.ks[d] = ks[d];
    cg.st[d] = st ? st[d] : 1;
    cg.pad[d] = pad ? pad[d] : ks[d] / 2;
    cg.dil[d] = dil ? dil[d] : 1;
    cg.in_shape[d] = in_shape ? in_shape[d] : 0;
    cg.out_shape[d] = out_shape ? out_shape[d] : 0;
    cg.K *= ks[d];
  }
  return cg.K;
}

}  // namespace df3d

using namespace df3d;

extern "C" size_t df3d_grid_bytes(int batch, const int *shape) {
  if (batch <= 0 || !shape || shape[0] <= 0 || shape[1] <= 0 || shape[2] <= 0) return 0;
  GridHeader h = grid_layout(batch, shape);
  return h.off_scratch + h.scratch_bytes + 256;
}

static int grid_finish(void *grid, const GridHeader &h, hipStream_t stream) {
  unsigned long long *bits = (unsigned long long *)((char *)grid + h.off_bits);
  uint32_t *prefix = (uint32_t *)((char *)grid + h.off_prefix);
  uint32_t *total = (uint32_t *)((char *)grid + h.off_total);
  return exclusive_scan_popc64(bits, prefix, (size_t)h.nwords, total, (char *)grid + h.off_scratch, h.scratch_bytes,
                               stream);
}

extern "C" int df3d_grid_build(const int32_t *indices, int n, int batch, const int *shape, void *grid,
                               size_t grid_bytes, int32_t *perm, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  DF3D_CHECK_ARG(batch > 0 && shape && n >= 0, "grid_build: bad arguments");
  GridHeader h = grid_layout(batch, shape);
  if (grid_bytes < h.off_scratch + h.scratch_bytes) {
    set_error("grid_build: grid blob too small (%zu < %zu)", grid_bytes, h.off_scratch + h.scratch_bytes);
    return DF3D_ENOMEM;
  }
  unsigned long long *bits = (unsigned long long *)((char *)grid + h.off_bits);
  DF3D_HIP(hipMemsetAsync(bits, 0, (size_t)h.nwords * 8, stream));
  Shape3 s3 = {{shape[0], shape[1], shape[2]}};
  long long vol = (long long)shape[0] * shape[1] * shape[2];
  if (n > 0)
    hipLaunchKernelGGL(grid_setbits_kernel, dim3(cdiv(n, 256)), dim3(256), 0, stream, indices, n, s3, vol, bits);
  int rc = grid_finish(grid, h, stream);
  if (rc) return rc;
  if (perm && n > 0) {
    GridView g = grid_view(grid, h);
    hipLaunchKernelGGL(grid_perm_kernel, dim3(cdiv(n, 256)), dim3(256), 0, stream, indices, n, g, perm);
  }
  DF3D_LAUNCH_CHECK();
  return DF3D_OK;
}

extern "C" int df3d_subm_neighbors(const void *grid, const int32_t *perm, const int32_t *indices, int n, int batch,
                                   const int *shape, const int *ksize, const int *dilation, int32_t *nbr,
                                   void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  // (an empty voxel set comes with null row pointers: legal, nothing to write)
  DF3D_CHECK_ARG(grid && shape && ksize && n >= 0 && (n == 0 || (indices && nbr)), "subm_neighbors: null argument");
  ConvGeom cg;
  int K = fill_geom(cg, ksize, nullptr, nullptr, dilation, shape, shape);
  DF3D_CHECK_ARG(K <= DF3D_MAX_KVOL, "subm_neighbors: kernel volume %d > %d", K, DF3D_MAX_KVOL);
  for (int d = 0; d < 3; ++d) {
    DF3D_CHECK_ARG(ksize[d] % 2 == 1, "subm_neighbors: even kernel size");
    cg.pad[d] = (ksize[d] / 2) * cg.dil[d];
    // spconv_ops.h:76-79 uses pad = k/2 irrespective of dilation; identical for dilation 1,
    // which is all the reference's backbones use.
    DF3D_CHECK_ARG(cg.dil[d] == 1, "subm_neighbors: dilation != 1 is not supported");
  }
  if (n == 0) return DF3D_OK;
  GridHeader h = grid_layout(batch, shape);
  GridView g = grid_view(grid, h);
  long long total = (long long)n * K;
  hipLaunchKernelGGL(neighbors_kernel, dim3(cdiv(total, 256)), dim3(256), 0, stream, g, perm, indices, n, cg, nbr);
  DF3D_LAUNCH_CHECK();
  return DF3D_OK;
}

extern "C" int df3d_conv_out_indices(const int32_t *indices, int n, int batch, const int *in_shape,
                                     const int *out_shape, const int *ksize, const int *stride, const int *padding,
                                     const int *dilation, void *out_grid, size_t out_grid_bytes,
                                     int32_t *out_indices, int out_cap, int32_t *num_out, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  DF3D_CHECK_ARG(out_grid && out_indices && num_out && n >= 0 && (n == 0 || indices), "conv_out_indices: null argument");
  ConvGeom cg;
  int K = fill_geom(cg, ksize, stride, padding, dilation, in_shape, out_shape);
  DF3D_CHECK_ARG(K <= DF3D_MAX_KVOL, "conv_out_indices: kernel volume %d > %d", K, DF3D_MAX_KVOL);
  for (int d = 0; d < 3; ++d) DF3D_CHECK_ARG(cg.dil[d] == 1 && cg.st[d] >= 1, "conv_out_indices: dilation != 1");
  GridHeader h = grid_layout(batch, out_shape);
  if (out_grid_bytes < h.off_scratch + h.scratch_bytes) {
    set_error("conv_out_indices: grid blob too small");
    return DF3D_ENOMEM;
  }
  unsigned long long *bits = (unsigned long long *)((char *)out_grid + h.off_bits);
  DF3D_HIP(hipMemsetAsync(bits, 0, (size_t)h.nwords * 8, stream));
  long long out_vol = (long long)out_shape[0] * out_shape[1] * out_shape[2];
  if (n > 0) {
    long long total = (long long)n * cg.ks[0] * cg.ks[1];
    hipLaunchKernelGGL(conv_mark_kernel, dim3(cdiv(total, 256)), dim3(256), 0, stream, indices, n, cg, out_vol, bits);
  }
  int rc = grid_finish(out_grid, h, stream);
  if (rc) return rc;
  GridView g = grid_view(out_grid, h);
  hipLaunchKernelGGL(grid_enumerate_kernel, dim3(cdiv((long long)h.nwords, 256)), dim3(256), 0, stream, g, h.nwords,
                     out_indices, out_cap);
  DF3D_HIP(hipMemcpyAsync(num_out, (char *)out_grid + h.off_total, sizeof(int32_t), hipMemcpyDeviceToDevice, stream));
  DF3D_LAUNCH_CHECK();
  return DF3D_OK;
}

extern "C" int df3d_conv_transpose_out_indices(const int32_t *indices, int n, int batch, const int *in_shape,
                                               const int *out_shape, const int *ksize, const int *stride,
                                               const int *padding, const int *dilation, void *out_grid,
                                               size_t out_grid_bytes, int32_t *out_indices, int out_cap,
                                               int32_t *num_out, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  DF3D_CHECK_ARG(out_grid && out_indices && num_out && n >= 0 && (n == 0 || indices),
                 "conv_transpose_out_indices: null argument");
  ConvGeom cg;
  int K = fill_geom(cg, ksize, stride, padding, dilation, in_shape, out_shape);
  DF3D_CHECK_ARG(K <= DF3D_MAX_KVOL, "conv_transpose_out_indices: kernel volume %d > %d", K, DF3D_MAX_KVOL);
  for (int d = 0; d < 3; ++d) DF3D_CHECK_ARG(cg.dil[d] >= 1 && cg.st[d] >= 1, "conv_transpose_out_indices: bad stride / dilation");
  GridHeader h = grid_layout(batch, out_shape);
  if (out_grid_bytes < h.off_scratch + h.scratch_bytes) {
    set_error("conv_transpose_out_indices: grid blob too small");
    return DF3D_ENOMEM;
  }
  unsigned long long *bits = (unsigned long long *)((char *)out_grid + h.off_bits);
  DF3D_HIP(hipMemsetAsync(bits, 0, (size_t)h.nwords * 8, stream));
  long long out_vol = (long long)out_shape[0] * out_shape[1] * out_shape[2];
  if (n > 0) {
    long long total = (long long)n * cg.ks[0] * cg.ks[1];
    hipLaunchKernelGGL(conv_mark_transpose_kernel, dim3(cdiv(total, 256)), dim3(256), 0, stream, indices, n, cg, out_vol,
                       bits);
  }
  int rc = grid_finish(out_grid, h, stream);
  if (rc) return rc;
  GridView g = grid_view(out_grid, h);
  hipLaunchKernelGGL(grid_enumerate_kernel, dim3(cdiv((long long)h.nwords, 256)), dim3(256), 0, stream, g, h.nwords,
                     out_indices, out_cap);
  DF3D_HIP(hipMemcpyAsync(num_out, (char *)out_grid + h.off_total, sizeof(int32_t), hipMemcpyDeviceToDevice, stream));
  DF3D_LAUNCH_CHECK();
  return DF3D_OK;
}

extern "C" int df3d_conv_transpose_neighbors(const void *in_grid, const int32_t *in_perm, const int32_t *out_indices,
                                             int n_out, int batch, const int *in_shape, const int *ksize,
                                             const int *stride, const int *padding, const int *dilation, int32_t *nbr,
                                             void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  DF3D_CHECK_ARG(in_grid && n_out >= 0 && (n_out == 0 || (out_indices && nbr)), "conv_transpose_neighbors: null argument");
  ConvGeom cg;
  int K = fill_geom(cg, ksize, stride, padding, dilation, in_shape, nullptr);
  DF3D_CHECK_ARG(K <= DF3D_MAX_KVOL, "conv_transpose_neighbors: kernel volume %d > %d", K, DF3D_MAX_KVOL);
  if (n_out == 0) return DF3D_OK;
  GridHeader h = grid_layout(batch, in_shape);
  GridView g = grid_view(in_grid, h);
  long long total = (long long)n_out * K;
  hipLaunchKernelGGL(neighbors_transpose_kernel, dim3(cdiv(total, 256)), dim3(256), 0, stream, g, in_perm, out_indices,
                     n_out, cg, nbr);
  DF3D_LAUNCH_CHECK();
  return DF3D_OK;
}

extern "C" int df3d_conv_neighbors(const void *in_grid, const int32_t *in_perm, const int32_t *out_indices,
                                   int n_out, int batch, const int *in_shape, const int *ksize, const int *stride,
                                   const int *padding, const int *dilation, int32_t *nbr, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  DF3D_CHECK_ARG(in_grid && n_out >= 0 && (n_out == 0 || (out_indices && nbr)), "conv_neighbors: null argument");
  ConvGeom cg;
  int K = fill_geom(cg, ksize, stride, padding, dilation, in_shape, nullptr);
  DF3D_CHECK_ARG(K <= DF3D_MAX_KVOL, "conv_neighbors: kernel volume %d > %d", K, DF3D_MAX_KVOL);
  if (n_out == 0) return DF3D_OK;
  GridHeader h = grid_layout(batch, in_shape);
  GridView g = grid_view(in_grid, h);
  long long total = (long long)n_out * K;
  hipLaunchKernelGGL(neighbors_kernel, dim3(cdiv(total, 256)), dim3(256), 0, stream, g, in_perm, out_indices, n_out,
                     cg, nbr);
  DF3D_LAUNCH_CHECK();
  return DF3D_OK;
}

extern "C" size_t df3d_nbr_to_pairs_workspace_bytes(int kvol, int n_out) {
  size_t n = (size_t)kvol * (size_t)n_out;
  size_t b = 0;
  b = arena_need(b, n * 4);
  b = arena_need(b, 64);
  b = arena_need(b, scan_scratch_bytes(n));
  return b + 256;
}

extern "C" int df3d_nbr_to_pairs(const int32_t *nbr, int kvol, int n_out, int n_in, int32_t *indice_pairs,
                                 int32_t *indice_num, void *workspace, size_t workspace_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  DF3D_CHECK_ARG(indice_num && kvol > 0 && kvol <= DF3D_MAX_KVOL && n_out >= 0 && n_in >= 0 && (nbr || n_out == 0) &&
                     (indice_pairs || n_in == 0),
                 "nbr_to_pairs: bad args");
  if (n_in > 0) DF3D_HIP(hipMemsetAsync(indice_pairs, 0xff, (size_t)kvol * 2 * (size_t)n_in * 4, stream));
  DF3D_HIP(hipMemsetAsync(indice_num, 0, (size_t)kvol * 4, stream));
  size_t n = (size_t)kvol * n_out;
  if (n == 0) return DF3D_OK;
  Arena ar(workspace, workspace_bytes);
  uint32_t *excl = ar.take<uint32_t>(n);
  uint32_t *total = ar.take<uint32_t>(16);
  size_t ssz = scan_scratch_bytes(n);
  void *sscr = ar.take<char>(ssz);
  if (!sscr) {
    set_error("nbr_to_pairs: workspace too small");
    return DF3D_ENOMEM;
  }
  hipLaunchKernelGGL(nbr_flag_kernel, dim3(cdiv((long long)n, 256)), dim3(256), 0, stream, nbr, n, excl);
  int rc = exclusive_scan_u32(excl, excl, n, total, sscr, ssz, stream);
  if (rc) return rc;
  hipLaunchKernelGGL(nbr_compact_kernel, dim3(cdiv((long long)n, 256)), dim3(256), 0, stream, nbr, excl, kvol, n_out,
                     n_in, total, indice_pairs, indice_num);
  DF3D_LAUNCH_CHECK();
  return DF3D_OK;
}

extern "C" int df3d_pairs_to_nbr(const int32_t *indice_pairs, const int32_t *indice_num_host, int kvol, int n_in,
                                 int n_out, int32_t *nbr, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  DF3D_CHECK_ARG(indice_num_host && kvol > 0 && kvol <= DF3D_MAX_KVOL && n_in >= 0 && n_out >= 0 && (nbr || n_out == 0) &&
                     (indice_pairs || n_in == 0),
                 "pairs_to_nbr: bad args");
  if (n_out > 0) DF3D_HIP(hipMemsetAsync(nbr, 0xff, (size_t)kvol * (size_t)n_out * 4, stream));
  if (n_in == 0 || n_out == 0) return DF3D_OK;
  NumArr na;
  for (int k = 0; k < DF3D_MAX_KVOL; ++k) na.v[k] = k < kvol ? indice_num_host[k] : 0;
  size_t n = (size_t)kvol * n_in;
  hipLaunchKernelGGL(pairs_to_nbr_kernel, dim3(cdiv((long long)n, 256)), dim3(256), 0, stream, indice_pairs, na, kvol,
                     n_in, n_out, nbr);
  DF3D_LAUNCH_CHECK();
  return DF3D_OK;
}
