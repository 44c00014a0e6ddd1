// The point side of PV-RCNN (VR/pcdet/ops/pointnet2/pointnet2_stack, VR/pcdet/models/backbones_3d/pfe): the stacked ball
// query, one scale of StackSAModuleMSG in eval mode as one kernel, and the bilinear BEV sample of VoxelSetAbstraction with
// its ordered backward.
//
// Ball query.  The reference (src/ball_query_gpu.cu:16-66) gives one THREAD a centre and walks the centre's frame row by
// row.  Here one WAVE owns a centre and takes 64 consecutive rows per step (coalesced 12-byte reads): `__ballot` of the
// hits, a prefix popcount below the lane ranks them in row order, and the loop ends (wave-uniformly) after the step in which
// the count reaches nsample.  d2 = ((dx*dx) + (dy*dy)) + (dz*dz) in float32 with every operation rounded on its own
// (contraction is off for this file), d2 < radius * radius: the accepted set is the reference's, whatever the compiler.
// The per-frame starts are summed on the device from the two count arrays (B <= 255), nothing is read back.
//
// Fused scale.  pooled[m, :] = max_s relu(W2 . relu(rows_in[idx[m, s]] + Wx . (xyz[idx[m, s]] - new_xyz[m]) + b1) + b2):
// the wave that found the ball keeps its rows in LDS, builds the hidden activations [nsample x C1] in registers as the A
// operand of v_mfma_f32_16x16x4_f32 (lane = (sample l % 16, channel quarter l / 16): the quarter g owns the channels
// [g * C1 / 4, (g + 1) * C1 / 4), a permutation of the reduction index that makes the gather 16-byte loads), multiplies
// by W2 (exact fp32 products, fp32 accumulation) and takes the max over the samples: over the 4 rows of a lane's
// accumulator, the sample tiles, then the four lane groups.  Slots past the hit count repeat the first hit (neutral for the
// max); an empty ball runs the same arithmetic on zero features and zero offsets, as the reference does.  Nothing of size
// M * C * nsample is written.
//
// BEV sample.  bilinear_interpolate_torch, expression for expression, one thread per (keypoint, channel), NCHW read in
// place.  Backward: the 4 * M (pixel, weight) contributions are sorted by pixel (the stable plan of dynscatter.hip) and
// every pixel sums its own in ascending keypoint order: no float atomics, the same bits on every run.
#include "common.h"

#pragma clang fp contract(off)

namespace df3d {
namespace {

constexpr int SP_WAVES = 4;            // centres per workgroup (one wave each)
constexpr int SP_BLOCK = 64 * SP_WAVES;
constexpr int SP_MAX_NSAMPLE = 64;     // a step's hits (at most 64) never rank past slot 2 * 64
constexpr int SP_MAX_BATCH = 255;

// the frame of stacked centre `m` and that frame's rows of xyz (ball_query_gpu.cu:27-46); counts are read as they are on
// the device, clipped so that no row outside [0, N) is ever addressed
__device__ __forceinline__ void sp_frame(const int32_t *__restrict__ new_cnt, const int32_t *__restrict__ cnt, int B, long long m,
                                         long long N, long long &start, int &n) {
  int b = 0;
  long long end = new_cnt[0];
  for (int k = 1; k < B; ++k) {
    if (m < end) break;
    end += new_cnt[k];
    b = k;
  }
  start = 0;
  for (int k = 0; k < b; ++k) start += cnt[k] > 0 ? cnt[k] : 0;
  long long nn = cnt[b] > 0 ? cnt[b] : 0;
  if (start > N) start = N;
  if (start + nn > N) nn = N - start;
  n = (int)nn;
}

// The scan of one centre by its wave; n, nsample and the centre are wave-uniform.  emit(slot, k) is called by the lane that
// found hit number `slot` (< nsample) at frame row k.  Returns min(hits, nsample) in every lane.
template <class Emit>
__device__ __forceinline__ int sp_scan(const float *__restrict__ xyz, int n, float nx, float ny, float nz, float radius2,
                                       int nsample, Emit emit) {
  const int lane = threadIdx.x & 63;
  int cnt = 0;
  for (int base = 0; base < n && cnt < nsample; base += 64) {
    const int k = base + lane;
    bool hit = false;
    if (k < n) {
      const float dx = nx - xyz[(long long)k * 3 + 0];
      const float dy = ny - xyz[(long long)k * 3 + 1];
      const float dz = nz - xyz[(long long)k * 3 + 2];
      const float d2 = (dx * dx + dy * dy) + dz * dz;
      hit = d2 < radius2;
    }
    const unsigned long long mask = __ballot(hit);
    const int slot = cnt + __popcll(mask & ((1ull << lane) - 1ull));
    if (hit && slot < nsample) emit(slot, k);
    cnt += __popcll(mask);
  }
  return cnt < nsample ? cnt : nsample;
}

__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_xor(v, d, 64);
    v = o > v ? o : v;
  }
  return v;
}

__global__ __launch_bounds__(SP_BLOCK) void ball_query_stack_kernel(const float *__restrict__ xyz,
                                                                    const int32_t *__restrict__ xyz_cnt, long long N,
                                                                    const float *__restrict__ new_xyz,
                                                                    const int32_t *__restrict__ new_cnt, long long M, int B,
                                                                    float radius2, int nsample, int32_t *__restrict__ idx) {
  const long long m = (long long)blockIdx.x * SP_WAVES + (threadIdx.x >> 6);
  if (m >= M) return;                  // whole waves leave; no barrier below
  const int lane = threadIdx.x & 63;
  long long start;
  int n;
  sp_frame(new_cnt, xyz_cnt, B, m, N, start, n);
  const float nx = new_xyz[m * 3 + 0], ny = new_xyz[m * 3 + 1], nz = new_xyz[m * 3 + 2];
  int32_t *out = idx + m * nsample;
  int first = -1;
  const int cnt = sp_scan(xyz + start * 3, n, nx, ny, nz, radius2, nsample, [&](int slot, int k) {
    out[slot] = k;
    if (slot == 0) first = k;
  });
  first = wave_max(first);             // rows are >= 0: the lane that wrote slot 0 wins
  // the first hit fills every slot before the later hits overwrite theirs (ball_query_gpu.cu:55-60); an empty ball is -1
  // in slot 0 and leaves the other slots as the caller allocated them
  if (cnt == 0) {
    if (lane == 0) out[0] = -1;
    return;
  }
  for (int s = cnt + lane; s < nsample; s += 64) out[s] = first;
}

// ---- fused scale.  wpos [C1, 4] = (wx, wy, wz, b1); w2 [C2, C1]; b2 [C2]
template <int C1, int C2, int NS>
__global__ __launch_bounds__(SP_BLOCK) void stack_sa_fused_kernel(const float *__restrict__ rows_in,
                                                                  const float *__restrict__ xyz,
                                                                  const int32_t *__restrict__ xyz_cnt, long long N,
                                                                  const float *__restrict__ new_xyz,
                                                                  const int32_t *__restrict__ new_cnt, long long M, int B,
                                                                  float radius2, const float *__restrict__ wpos,
                                                                  const float *__restrict__ w2, const float *__restrict__ b2,
                                                                  float *__restrict__ pooled, int32_t *__restrict__ idx,
                                                                  uint8_t *__restrict__ empty) {
  constexpr int KS = C1 / 4;           // hidden channels of a lane group
  constexpr int NT = NS / 16;          // sample tiles
  constexpr int CT = C2 / 16;          // output channel tiles
  __shared__ int32_t s_idx[SP_WAVES][NS];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long m = (long long)blockIdx.x * SP_WAVES + wave;
  const bool live = m < M;
  long long start = 0;
  int n = 0;
  float nx = 0.f, ny = 0.f, nz = 0.f;
  if (live) {
    sp_frame(new_cnt, xyz_cnt, B, m, N, start, n);
    nx = new_xyz[m * 3 + 0], ny = new_xyz[m * 3 + 1], nz = new_xyz[m * 3 + 2];
  }
  int32_t *slots = s_idx[wave];
  const int cnt = sp_scan(xyz + start * 3, n, nx, ny, nz, radius2, NS, [&](int slot, int k) { slots[slot] = k; });
  __syncthreads();
  if (!live) return;
  const int g = lane >> 4, col = lane & 15;
  // A operand: hidden activations of sample (tile t, col), channels g * KS + j
  float a[NT][KS];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int s = t * 16 + col;
    float px = 0.f, py = 0.f, pz = 0.f;
    float f[KS];
#pragma unroll
    for (int j = 0; j < KS; ++j) f[j] = 0.f;
    if (cnt > 0) {
      const long long row = start + slots[s < cnt ? s : 0];
      px = xyz[row * 3 + 0] - nx, py = xyz[row * 3 + 1] - ny, pz = xyz[row * 3 + 2] - nz;
      if (rows_in) {
#pragma unroll
        for (int j = 0; j < KS; j += 4) {
          const f32x4 v = *(const f32x4 *)(rows_in + row * C1 + g * KS + j);
          f[j] = v[0], f[j + 1] = v[1], f[j + 2] = v[2], f[j + 3] = v[3];
        }
      }
    }
#pragma unroll
    for (int j = 0; j < KS; ++j) {
      const f32x4 w = *(const f32x4 *)(wpos + (size_t)(g * KS + j) * 4);
      a[t][j] = fmaxf((f[j] + ((w[0] * px + w[1] * py) + w[2] * pz)) + w[3], 0.f);
    }
  }
  f32x4 acc[NT][CT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[t][ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
#pragma unroll
    for (int j = 0; j < KS; j += 4) {
      // B operand: W2[ct * 16 + col][g * KS + j .. + 3]
      const f32x4 b = *(const f32x4 *)(w2 + (size_t)(ct * 16 + col) * C1 + g * KS + j);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int t = 0; t < NT; ++t)
          acc[t][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][j + i], b[i], acc[t][ct], 0, 0, 0);
    }
  }
  // lane (samples 4 g + r of every tile, output channel ct * 16 + col): max over its rows, then over the lane groups
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    float v = acc[0][ct][0];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) v = fmaxf(v, acc[t][ct][r]);
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    v = fmaxf(v, __shfl_xor(v, 32, 64));
    // x -> relu(x + b2) is monotone: the max of the sums first, bias and ReLU once
    if (g == 0) pooled[m * C2 + ct * 16 + col] = fmaxf(v + b2[ct * 16 + col], 0.f);
  }
  if (idx && lane < NS) idx[m * NS + lane] = cnt > 0 ? slots[lane < cnt ? lane : 0] : 0;
  if (empty && lane == 0) empty[m] = cnt == 0;
}

// ---- BEV sample
struct BevGeom {
  int B, C, H, W;
  float range_x, range_y, voxel_x, voxel_y, stride;
};

// the four corners (y0 x0, y1 x0, y0 x1, y1 x1: Ia, Ib, Ic, Id of bilinear_interpolate_torch) of keypoint row kp.  The
// reference clamps floor(x) and floor(x) + 1 to the map FIRST and takes the weights from the clamped corners
// (voxel_set_abstraction.py:27-40: outside the map both corners coincide and the two weights cancel), and so does this.
// Returns the frame, -1 when it is none of 0 .. B-1.
__device__ __forceinline__ int bev_corners(const BevGeom &q, const float *__restrict__ kp, float w[4], int off[4]) {
  const float bf = kp[0];
  const float x = __fdiv_rn(__fdiv_rn(kp[1] - q.range_x, q.voxel_x), q.stride);
  const float y = __fdiv_rn(__fdiv_rn(kp[2] - q.range_y, q.voxel_y), q.stride);
  const float xf = floorf(x), yf = floorf(y);
  // (a NaN coordinate clamps to 0: fmaxf returns the other operand)
  const float x0 = fminf(fmaxf(xf, 0.f), (float)(q.W - 1)), x1 = fminf(fmaxf(xf + 1.f, 0.f), (float)(q.W - 1));
  const float y0 = fminf(fmaxf(yf, 0.f), (float)(q.H - 1)), y1 = fminf(fmaxf(yf + 1.f, 0.f), (float)(q.H - 1));
  w[0] = (x1 - x) * (y1 - y);
  w[1] = (x1 - x) * (y - y0);
  w[2] = (x - x0) * (y1 - y);
  w[3] = (x - x0) * (y - y0);
  const int ix0 = (int)x0, ix1 = (int)x1, iy0 = (int)y0, iy1 = (int)y1;
  off[0] = iy0 * q.W + ix0;
  off[1] = iy1 * q.W + ix0;
  off[2] = iy0 * q.W + ix1;
  off[3] = iy1 * q.W + ix1;
  return bf >= 0.f && bf < (float)q.B ? (int)bf : -1;
}

__global__ __launch_bounds__(256) void bev_interpolate_kernel(BevGeom q, const float *__restrict__ keypoints, long long M,
                                                              const float *__restrict__ bev, float *__restrict__ out) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= M * q.C) return;
  const long long m = t / q.C;
  const int c = (int)(t % q.C);
  float w[4];
  int off[4];
  const int b = bev_corners(q, keypoints + m * 4, w, off);
  float v = 0.f;
  if (b >= 0) {
    const float *im = bev + ((long long)b * q.C + c) * q.H * q.W;
    v = ((im[off[0]] * w[0] + im[off[1]] * w[1]) + im[off[2]] * w[2]) + im[off[3]] * w[3];
  }
  out[t] = v;
}

// target pixel b * H * W + y * W + x of contribution 4 m + corner, -1 for a keypoint of no frame
__global__ __launch_bounds__(256) void bev_targets_kernel(BevGeom q, const float *__restrict__ keypoints, long long M,
                                                          int32_t *__restrict__ target) {
  const long long m = (long long)blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  float w[4];
  int off[4];
  const int b = bev_corners(q, keypoints + m * 4, w, off);
#pragma unroll
  for (int i = 0; i < 4; ++i) target[m * 4 + i] = b >= 0 ? b * q.H * q.W + off[i] : -1;
}

// one thread per (referenced pixel, channel): the pixel's contributions in ascending (keypoint, corner) order
__global__ __launch_bounds__(256) void bev_grad_pixels_kernel(BevGeom q, const float *__restrict__ grad_out,
                                                              const float *__restrict__ keypoints,
                                                              const int32_t *__restrict__ pixels,
                                                              const int32_t *__restrict__ offsets,
                                                              const int32_t *__restrict__ ids,
                                                              const int32_t *__restrict__ status, float *__restrict__ grad_bev) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long v = t / q.C;
  const int c = (int)(t % q.C);
  if (v >= status[0]) return;
  const int pix = pixels[v];
  const int hw = q.H * q.W;
  if (pix < 0 || pix >= q.B * hw) return;
  float acc = 0.f;
  for (int p = offsets[v], e = offsets[v + 1]; p < e; ++p) {
    const int id = ids[p];
    float w[4];
    int off[4];
    bev_corners(q, keypoints + (long long)(id >> 2) * 4, w, off);
    acc += grad_out[(long long)(id >> 2) * q.C + c] * w[id & 3];
  }
  grad_bev[((long long)(pix / hw) * q.C + c) * hw + pix % hw] = acc;
}

struct BevGradWs {
  int32_t *target, *pixels, *p2v, *count, *offsets, *ids, *status;
  void *plan;
  size_t plan_bytes, bytes;
};

int bev_grad_layout(long long n, void *ws, size_t ws_bytes, BevGradWs &w, void *stream) {
  w.plan_bytes = df3d_dynamic_scatter_plan_workspace_bytes(n, stream);
  if (w.plan_bytes == 0) {
    set_error("bev_interpolate_grad: no plan workspace for %lld contributions (1 <= 4 * M < 2^31)", n);
    return DF3D_EINVAL;
  }
  WsLayout l;
  const size_t o_target = l.take((size_t)n * 4), o_pixels = l.take((size_t)n * 4), o_p2v = l.take((size_t)n * 4),
               o_count = l.take((size_t)n * 4), o_offsets = l.take((size_t)(n + 1) * 4), o_ids = l.take((size_t)n * 4),
               o_status = l.take(2 * 4), o_plan = l.take(w.plan_bytes);
  w.bytes = l.total();
  if (!ws) return DF3D_OK;
  if (ws_bytes < w.bytes) {
    set_error("bev_interpolate_grad: workspace too small (%zu < %zu)", ws_bytes, w.bytes);
    return DF3D_ENOMEM;
  }
  char *p = (char *)ws;
  w.target = (int32_t *)(p + o_target), w.pixels = (int32_t *)(p + o_pixels), w.p2v = (int32_t *)(p + o_p2v);
  w.count = (int32_t *)(p + o_count), w.offsets = (int32_t *)(p + o_offsets), w.ids = (int32_t *)(p + o_ids);
  w.status = (int32_t *)(p + o_status), w.plan = p + o_plan;
  return DF3D_OK;
}

int bev_geom(BevGeom &q, const char *what, long long M, int B, int C, int H, int W, float range_x, float range_y, float voxel_x,
             float voxel_y, float stride) {
  DF3D_CHECK_ARG(M >= 0 && B >= 1 && C >= 1 && H >= 1 && W >= 1, "%s: bad sizes", what);
  DF3D_CHECK_ARG((long long)B * H * W < (1ll << 31) && M * C < (1ll << 40), "%s: B * H * W must be below 2^31 and M * C below 2^40",
                 what);
  DF3D_CHECK_ARG(voxel_x > 0.f && voxel_y > 0.f && stride > 0.f, "%s: voxel size and stride must be positive", what);
  q.B = B, q.C = C, q.H = H, q.W = W;
  q.range_x = range_x, q.range_y = range_y, q.voxel_x = voxel_x, q.voxel_y = voxel_y, q.stride = stride;
  return DF3D_OK;
}

int stack_args(const char *what, long long N, long long M, int B, float radius, int nsample) {
  DF3D_CHECK_ARG(B >= 1 && B <= SP_MAX_BATCH, "%s: B = %d outside 1..%d frames", what, B, SP_MAX_BATCH);
  DF3D_CHECK_ARG(nsample >= 1 && nsample <= SP_MAX_NSAMPLE, "%s: nsample %d is above the limit of %d", what, nsample,
                 SP_MAX_NSAMPLE);
  DF3D_CHECK_ARG(N >= 0 && N < (1ll << 31) && M >= 0 && M < (1ll << 31), "%s: bad sizes", what);
  DF3D_CHECK_ARG(radius >= 0.f, "%s: negative radius", what);
  return DF3D_OK;
}

}  // namespace
}  // namespace df3d

using namespace df3d;

extern "C" int df3d_ball_query_stack(const float *xyz, const int32_t *xyz_batch_cnt, long long N, const float *new_xyz,
                                     const int32_t *new_xyz_batch_cnt, long long M, int B, float radius, int nsample,
                                     int32_t *idx, void *stream) {
  DF3D_CHECK_ARG(xyz && xyz_batch_cnt && new_xyz && new_xyz_batch_cnt && idx, "ball_query_stack: null argument");
  int rc = stack_args("ball_query_stack", N, M, B, radius, nsample);
  if (rc) return rc;
  if (M == 0) return DF3D_OK;
  hipLaunchKernelGGL(ball_query_stack_kernel, dim3(cdiv(M, SP_WAVES)), dim3(SP_BLOCK), 0, (hipStream_t)stream, xyz,
                     xyz_batch_cnt, N, new_xyz, new_xyz_batch_cnt, M, B, radius * radius, nsample, idx);
  DF3D_LAUNCH_CHECK();
  return DF3D_OK;
}

extern "C" int df3d_stack_sa_fused_supported(int C1, int C2, int nsample) {
  return (C1 == 16 || C1 == 32 || C1 == 64) && (C2 == 16 || C2 == 32 || C2 == 64) && (nsample == 16 || nsample == 32);
}

extern "C" int df3d_stack_sa_fused(const float *rows_in, const float *xyz, const int32_t *xyz_batch_cnt, long long N,
                                   const float *new_xyz, const int32_t *new_xyz_batch_cnt, long long M, int B, float radius,
                                   int nsample, int C1, int C2, const float *w_pos, const float *w2, const float *b2,
                                   float *pooled, int32_t *idx, uint8_t *empty, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  DF3D_CHECK_ARG(xyz && xyz_batch_cnt && new_xyz && new_xyz_batch_cnt && w_pos && w2 && b2 && pooled,
                 "stack_sa_fused: null argument");
  DF3D_CHECK_ARG(df3d_stack_sa_fused_supported(C1, C2, nsample),
                 "stack_sa_fused: C1 = %d, C2 = %d, nsample = %d: the kernel serves 16, 32 and 64 channels and 16 or 32 samples",
                 C1, C2, nsample);
  DF3D_CHECK_ARG(((uintptr_t)rows_in | (uintptr_t)w_pos | (uintptr_t)w2) % 16 == 0,
                 "stack_sa_fused: rows_in, w_pos and w2 must be 16-byte aligned");
  int rc = stack_args("stack_sa_fused", N, M, B, radius, nsample);
  if (rc) return rc;
  if (M == 0) return DF3D_OK;
  const dim3 grid(cdiv(M, SP_WAVES)), block(SP_BLOCK);
  const float radius2 = radius * radius;
#define DF3D_SP_LAUNCH(A, Bc, S)                                                                                               \
  hipLaunchKernelGGL((stack_sa_fused_kernel<A, Bc, S>), grid, block, 0, stream, rows_in, xyz, xyz_batch_cnt, N, new_xyz,      \
                     new_xyz_batch_cnt, M, B, radius2, w_pos, w2, b2, pooled, idx, empty)
#define DF3D_SP_C2(A, S)                       \
  do {                                         \
    if (C2 == 16) DF3D_SP_LAUNCH(A, 16, S);    \
    else if (C2 == 32) DF3D_SP_LAUNCH(A, 32, S); \
    else DF3D_SP_LAUNCH(A, 64, S);             \
  } while (0)
#define DF3D_SP_C1(S)                  \
  do {                                 \
    if (C1 == 16) DF3D_SP_C2(16, S);   \
    else if (C1 == 32) DF3D_SP_C2(32, S); \
    else DF3D_SP_C2(64, S);            \
  } while (0)
  if (nsample == 16) DF3D_SP_C1(16); else DF3D_SP_C1(32);
#undef DF3D_SP_C1
#undef DF3D_SP_C2
#undef DF3D_SP_LAUNCH
  DF3D_LAUNCH_CHECK();
  return DF3D_OK;
}

extern "C" int df3d_bev_interpolate(const float *keypoints, long long M, const float *bev, int B, int C, int H, int W,
                                    float range_x, float range_y, float voxel_x, float voxel_y, float stride, float *out,
                                    void *stream) {
  DF3D_CHECK_ARG(keypoints && bev && out, "bev_interpolate: null argument");
  BevGeom q;
  int rc = bev_geom(q, "bev_interpolate", M, B, C, H, W, range_x, range_y, voxel_x, voxel_y, stride);
  if (rc) return rc;
  if (M == 0) return DF3D_OK;
  hipLaunchKernelGGL(bev_interpolate_kernel, dim3(cdiv(M * C, 256)), dim3(256), 0, (hipStream_t)stream, q, keypoints, M, bev,
                     out);
  DF3D_LAUNCH_CHECK();
  return DF3D_OK;
}

extern "C" size_t df3d_bev_interpolate_grad_workspace_bytes(long long M, void *stream) {
  if (M <= 0 || M * 4 >= (1ll << 31)) return 0;
  BevGradWs w;
  if (bev_grad_layout(M * 4, nullptr, 0, w, stream) != DF3D_OK) return 0;
  return w.bytes;
}

extern "C" int df3d_bev_interpolate_grad(const float *grad_out, const float *keypoints, long long M, int B, int C, int H, int W,
                                         float range_x, float range_y, float voxel_x, float voxel_y, float stride,
                                         float *grad_bev, void *workspace, size_t workspace_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  DF3D_CHECK_ARG(grad_out && keypoints && grad_bev, "bev_interpolate_grad: null argument");
  BevGeom q;
  int rc = bev_geom(q, "bev_interpolate_grad", M, B, C, H, W, range_x, range_y, voxel_x, voxel_y, stride);
  if (rc) return rc;
  const long long n = M * 4;
  DF3D_CHECK_ARG(n < (1ll << 31), "bev_interpolate_grad: 4 * M = %lld is above the limit of 2^31 - 1", n);
  DF3D_HIP(hipMemsetAsync(grad_bev, 0, (size_t)B * C * H * W * sizeof(float), stream));   // pixels nobody samples: exactly 0
  if (n == 0) return DF3D_OK;
  DF3D_CHECK_ARG(workspace, "bev_interpolate_grad: null workspace");
  BevGradWs w;
  rc = bev_grad_layout(n, workspace, workspace_bytes, w, stream_);
  if (rc) return rc;
  hipLaunchKernelGGL(bev_targets_kernel, dim3(cdiv(M, 256)), dim3(256), 0, stream, q, keypoints, M, w.target);
  DF3D_LAUNCH_CHECK();
  rc = df3d_dynamic_scatter_plan(w.target, n, 1, w.pixels, w.p2v, w.count, w.offsets, w.ids, w.status, w.plan, w.plan_bytes,
                                 stream_);
  if (rc) return rc;
  // at most min(n, B * H * W) distinct pixels; the count stays on the device (status[0])
  const long long vmax = n < (long long)B * H * W ? n : (long long)B * H * W;
  hipLaunchKernelGGL(bev_grad_pixels_kernel, dim3(cdiv(vmax * C, 256)), dim3(256), 0, stream, q, grad_out, keypoints, w.pixels,
                     w.offsets, w.ids, w.status, grad_bev);
  DF3D_LAUNCH_CHECK();
  return DF3D_OK;
}
