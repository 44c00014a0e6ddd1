// Regression branches of the CenterPoint head at the object centres only (the loss-only head path).
//
// A no-grad evaluation of the detection losses (csrc/loss.hip) reads the heat maps densely, but the 30 regression maps
// (reg / height / dim / rot / vel of six tasks) only at the <= batch * max_objs object slots of each task, and only where
// the slot's mask is set.  The dense head computes every one of them on all 180 x 180 pixels: first convs 64 -> 64 per
// branch, BatchNorm fold, ReLU, final 3 x 3 conv 64 -> k.  Here the same two convolutions run for the object centres alone:
//   mid[j][c] = relu(scale_c * (bias_c + sum_tap sum_ci s1[p + off(j) + off(tap)][ci] * W1[tap][ci][c]) + shift_c)
//               at the 9 sites j of the 3 x 3 window around the centre p (0 where the site lies outside the map),
//   pred[code] = b2 + sum_j sum_c mid[j][c] * W2[j][c][code].
// Arithmetic of the maps it replaces: the first conv on v_mfma_f32_16x16x32_f16 over the two-part split rows of the
// shared conv's output and filters split once by the pack kernel below (A_lo W_hi + A_hi W_lo + A_hi W_hi, fp32
// accumulate, 2^-(SA + SW) in the epilogue: csrc/spconv_split.hip); the final conv in fp32 FMAs on the fp32 `mid`
// values (nothing is split here, so the kernel raises no range flag of its own).  Every sum has a fixed order, there
// are no atomics: two runs are bit-identical.
//
// Launch shape: grid (ceil(batch * max_objs / 7), branches, tasks) -- from the sizes alone, no count is read back.  A
// workgroup owns 7 consecutive slots of one task and one branch (7 x 9 = 63 site rows = four 16-row matrix tiles); it
// writes zeros and exits when none of its slots is live.  Otherwise it stages the 5 x 5 x 64 halo of each slot in LDS once,
// runs the [64 x 576] x [576 x 64] product with A fragments from LDS and B fragments streamed from L2 (147 KB per branch,
// one tap ahead in registers), keeps `mid` in LDS and finishes with the final conv of the centre pixels.
#include "common.h"

namespace df3d {

DF3D_SPLIT_OVERFLOW_TU(headloss)

constexpr int HR_SLOTS = 7;                    // slots per workgroup
constexpr int HR_ROWS = 64;                    // site rows per workgroup (HR_SLOTS * 9 = 63, one padding row)
constexpr int HR_C = 64;                       // channels of the shared rows and of every branch's first conv
constexpr int HR_PIX = 25;                     // 5 x 5 halo pixels per slot
constexpr int HR_PS = 17;                      // u32x4 per halo pixel in LDS: 16 (8 blocks of hi | lo) + 1 (bank shift)
constexpr int HR_MS = HR_C + 1;                // floats per `mid` row in LDS
constexpr int HR_BANK = 9 * 2 * 4 * 2 * 64;    // u32x4 per packed branch: [tap][kb][ct][hi|lo][lane]

struct RegressArgs {
  const u32x4 *s1;                             // split rows [B*H*W][16]
  df3d_head_targets target[DF3D_MAX_HEAD_TASKS];
  const u32x4 *w1;                             // [tasks * branches][HR_BANK]
  const float *bias1, *scale1, *shift1;        // [tasks * branches][64]
  const float *w2, *b2;                        // [tasks * branches][9][64][4], [tasks * branches][4]
  const int32_t *cols;                         // [tasks * branches][2] = (first code column, codes)
  float *pred;                                 // [tasks][B * M][DF3D_LOSS_MAX_CODES]
  int T, NB, B, H, W, M;
};

// W1 [branches][9][64][64] fp32 (tap, cin, cout) -> the B operand of every lane: [branch][tap][kb][ct][hi|lo][lane],
// lane (n, g) = column ct * 16 + n, channels kb * 32 + g * 8 + e
__global__ __launch_bounds__(256) void head_regress_pack_kernel(const float *__restrict__ w, size_t total,
                                                                u32x4 *__restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int lane = (int)(i & 63);
  size_t r = i >> 6;
  const int part = (int)(r & 1); r >>= 1;
  const int ct = (int)(r & 3); r >>= 2;
  const int kb = (int)(r & 1); r >>= 1;
  const int tap = (int)(r % 9);
  const size_t br = r / 9;
  const int col = ct * 16 + (lane & 15), ch0 = kb * 32 + (lane >> 4) * 8;
  const float *wb = w + ((br * 9 + tap) * HR_C + ch0) * HR_C + col;
  u32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    unsigned hi, lo;
    split_pair_w(wb[(size_t)(2 * e) * HR_C], wb[(size_t)(2 * e + 1) * HR_C], hi, lo);
    o[e] = part ? lo : hi;
  }
  out[i] = o;
}

__global__ __launch_bounds__(256) void head_regress_kernel(RegressArgs a) {
  __shared__ u32x4 s_halo[HR_SLOTS * HR_PIX * HR_PS];
  __shared__ float s_mid[HR_ROWS * HR_MS];
  __shared__ int s_cy[HR_SLOTS + 1], s_cx[HR_SLOTS + 1], s_b[HR_SLOTS + 1];
  __shared__ int s_valid[HR_ROWS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t = blockIdx.z, br = t * a.NB + blockIdx.y;
  const int slots = a.B * a.M, slot0 = blockIdx.x * HR_SLOTS, hw = a.H * a.W;
  const int col0 = a.cols[2 * br], ncol = a.cols[2 * br + 1];

  if (tid <= HR_SLOTS) {
    const int s = slot0 + tid;
    int cy = -1, cx = 0, b = 0;
    if (tid < HR_SLOTS && s < slots && a.target[t].mask[s]) {
      const long long ind = a.target[t].ind[s];
      if (ind >= 0 && ind < hw) cy = (int)(ind / a.W), cx = (int)(ind - (long long)cy * a.W), b = s / a.M;
    }
    s_cy[tid] = cy, s_cx[tid] = cx, s_b[tid] = b;
  }
  __syncthreads();
  bool any = false;
#pragma unroll
  for (int i = 0; i < HR_SLOTS; ++i) any = any || s_cy[i] >= 0;

  // code columns no branch of this task writes (the vel pair of an 8-code head): zeroed by the task's first branch
  unsigned mine = 0;
  for (int c = 0; c < ncol; ++c)
    if (col0 + c >= 0 && col0 + c < DF3D_LOSS_MAX_CODES) mine |= 1u << (col0 + c);
  if (blockIdx.y == 0) {
    unsigned covered = 0;
    for (int q = 0; q < a.NB; ++q) {
      const int c0 = a.cols[2 * (t * a.NB + q)], k = a.cols[2 * (t * a.NB + q) + 1];
      for (int c = 0; c < k; ++c)
        if (c0 + c >= 0 && c0 + c < DF3D_LOSS_MAX_CODES) covered |= 1u << (c0 + c);
    }
    const unsigned rest = ~covered & ((1u << DF3D_LOSS_MAX_CODES) - 1u);
    if (!any) mine |= rest;
    else if (tid < HR_SLOTS * DF3D_LOSS_MAX_CODES) {
      const int s = slot0 + tid / DF3D_LOSS_MAX_CODES, c = tid % DF3D_LOSS_MAX_CODES;
      if (s < slots && ((rest >> c) & 1u)) a.pred[((size_t)t * slots + s) * DF3D_LOSS_MAX_CODES + c] = 0.f;
    }
  }
  if (!any) {                                  // a dead workgroup: its columns of its slots are 0 (the loss multiplies by the mask)
    if (tid < HR_SLOTS * DF3D_LOSS_MAX_CODES) {
      const int s = slot0 + tid / DF3D_LOSS_MAX_CODES, c = tid % DF3D_LOSS_MAX_CODES;
      if (s < slots && ((mine >> c) & 1u)) a.pred[((size_t)t * slots + s) * DF3D_LOSS_MAX_CODES + c] = 0.f;
    }
    return;
  }

  // ---- the 5 x 5 halo of every slot (zero outside the map and for dead slots), which sites lie inside the map
  for (int it = tid; it < HR_SLOTS * HR_PIX * 16; it += 256) {
    const int slot = it / (HR_PIX * 16), rem = it - slot * (HR_PIX * 16), pix = rem >> 4, q = rem & 15;
    const int cy = s_cy[slot], y = cy + pix / 5 - 2, x = s_cx[slot] + pix % 5 - 2;
    u32x4 v = (u32x4){0u, 0u, 0u, 0u};
    if (cy >= 0 && y >= 0 && y < a.H && x >= 0 && x < a.W)
      v = a.s1[(((size_t)s_b[slot] * a.H + y) * a.W + x) * 16 + q];
    s_halo[(slot * HR_PIX + pix) * HR_PS + q] = v;
  }
  if (tid < HR_ROWS) {
    const int slot = tid / 9, j = tid - slot * 9;                      // (row 63: slot 7, the dead padding entry)
    const int cy = s_cy[slot], y = cy + j / 3 - 1, x = s_cx[slot] + j % 3 - 1;
    s_valid[tid] = cy >= 0 && y >= 0 && y < a.H && x >= 0 && x < a.W;
  }
  __syncthreads();

  // ---- first conv: wave = 16-column tile ct of the branch, four 16-row tiles; lane (n, g) = A row n / B column n, channels g * 8 ..
  const int n = lane & 15, g = lane >> 4, ct = wave;
  int abase[4];
#pragma unroll
  for (int rt = 0; rt < 4; ++rt) {
    const int row = rt * 16 + n, slot = row / 9, j = row - slot * 9;
    abase[rt] = (slot < HR_SLOTS ? slot * HR_PIX : 0) + (j / 3) * 5 + j % 3;   // halo pixel of the site's tap (0, 0)
  }
  const u32x4 *wl = a.w1 + (size_t)br * HR_BANK + ct * 128 + lane;     // + ((tap * 2 + kb) * 4) * 128 + part * 64
  f32x4 acc[4];
#pragma unroll
  for (int rt = 0; rt < 4; ++rt) acc[rt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  u32x4 bq[2][4];                                                     // [stage][kb * 2 + part]
#pragma unroll
  for (int i = 0; i < 4; ++i) bq[0][i] = wl[(i >> 1) * 512 + (i & 1) * 64];
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    if (tap + 1 < 9) {
#pragma unroll
      for (int i = 0; i < 4; ++i) bq[(tap + 1) & 1][i] = wl[((tap + 1) * 2 + (i >> 1)) * 512 + (i & 1) * 64];
    }
    const int poff = (tap / 3) * 5 + tap % 3;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      const u32x4 bh = bq[tap & 1][kb * 2], bl = bq[tap & 1][kb * 2 + 1];
#pragma unroll
      for (int rt = 0; rt < 4; ++rt) {
        const u32x4 *ap = s_halo + (abase[rt] + poff) * HR_PS + (kb * 4 + g) * 2;
        const u32x4 ah = ap[0], al = ap[1];
        acc[rt] = DF3D_MFMA_F16(al, bh, acc[rt]);
        acc[rt] = DF3D_MFMA_F16(ah, bl, acc[rt]);
        acc[rt] = DF3D_MFMA_F16(ah, bh, acc[rt]);
      }
    }
  }
  {
    const int col = ct * 16 + n;
    const float bi = a.bias1[br * HR_C + col], sc = a.scale1[br * HR_C + col], sh = a.shift1[br * HR_C + col];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = rt * 16 + g * 4 + r;
        const float v = fmaxf((acc[rt][r] * DF3D_ACC_UNSCALE + bi) * sc + sh, 0.f);
        s_mid[row * HR_MS + col] = s_valid[row] ? v : 0.f;
      }
  }
  __syncthreads();

  // ---- final conv of the centre pixels: 8 threads per (slot, code), 8 channels x 9 sites each, then a fixed butterfly
  const int o = tid >> 3, sub = tid & 7, slot = o >> 2, code = o & 3;
  float sum = 0.f;
  if (slot < HR_SLOTS) {
    const float *w2 = a.w2 + (size_t)br * 9 * HR_C * 4 + code;
    const float *m = s_mid + slot * 9 * HR_MS + sub * 8;
#pragma unroll
    for (int j = 0; j < 9; ++j)
#pragma unroll
      for (int c = 0; c < 8; ++c) sum += m[j * HR_MS + c] * w2[(j * HR_C + sub * 8 + c) * 4];
  }
  sum += __shfl_xor(sum, 1, 64);
  sum += __shfl_xor(sum, 2, 64);
  sum += __shfl_xor(sum, 4, 64);
  const int s = slot0 + slot, cc = col0 + code;
  if (sub == 0 && slot < HR_SLOTS && s < slots && code < ncol && cc >= 0 && cc < DF3D_LOSS_MAX_CODES)
    a.pred[((size_t)t * slots + s) * DF3D_LOSS_MAX_CODES + cc] = s_cy[slot] >= 0 ? sum + a.b2[br * 4 + code] : 0.f;
}

}  // namespace df3d

using namespace df3d;

extern "C" size_t df3d_head_regress_packed_bytes(int branches) {
  return branches > 0 ? (size_t)branches * HR_BANK * sizeof(u32x4) : 0;
}

extern "C" int df3d_head_regress_pack(const float *w1, int branches, void *packed, void *stream) {
  DF3D_CHECK_ARG(w1 && packed && branches >= 1, "head_regress_pack: bad argument");
  const size_t total = (size_t)branches * HR_BANK;
  hipLaunchKernelGGL(head_regress_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w1, total,
                     (u32x4 *)packed);
  DF3D_LAUNCH_CHECK();
  return DF3D_OK;
}

extern "C" int df3d_head_regress_at(const void *s1_split, int batch, int H, int W, const df3d_head_targets *targets,
                                    int ntasks, int max_objs, int branches, const void *w1_packed, const float *bias1,
                                    const float *scale1, const float *shift1, const float *w2, const float *b2,
                                    const int32_t *cols, float *pred, void *stream) {
  DF3D_CHECK_ARG(s1_split && targets && w1_packed && bias1 && scale1 && shift1 && w2 && b2 && cols && pred,
                 "head_regress_at: null argument");
  DF3D_CHECK_ARG(ntasks >= 1 && ntasks <= DF3D_MAX_HEAD_TASKS, "head_regress_at: 1..%d tasks", DF3D_MAX_HEAD_TASKS);
  DF3D_CHECK_ARG(branches >= 1 && branches <= 65535, "head_regress_at: bad branch count %d", branches);
  DF3D_CHECK_ARG(batch >= 1 && H >= 1 && W >= 1 && max_objs >= 0, "head_regress_at: bad sizes");
  DF3D_CHECK_ARG((long long)batch * H * W < 0x7fffffffLL && (long long)batch * max_objs < 0x7fffffffLL,
                 "head_regress_at: map or slot list too large");
  if (max_objs == 0) return DF3D_OK;
  RegressArgs a;
  a.s1 = (const u32x4 *)s1_split;
  for (int t = 0; t < DF3D_MAX_HEAD_TASKS; ++t) {
    a.target[t] = targets[t < ntasks ? t : 0];
    DF3D_CHECK_ARG(t >= ntasks || (targets[t].ind && targets[t].mask), "head_regress_at: task %d misses ind / mask", t);
  }
  a.w1 = (const u32x4 *)w1_packed;
  a.bias1 = bias1, a.scale1 = scale1, a.shift1 = shift1, a.w2 = w2, a.b2 = b2, a.cols = cols, a.pred = pred;
  a.T = ntasks, a.NB = branches, a.B = batch, a.H = H, a.W = W, a.M = max_objs;
  hipLaunchKernelGGL(head_regress_kernel, dim3(cdiv((long long)batch * max_objs, HR_SLOTS), branches, ntasks), dim3(256), 0,
                     (hipStream_t)stream, a);
  DF3D_LAUNCH_CHECK();
  return DF3D_OK;
}
