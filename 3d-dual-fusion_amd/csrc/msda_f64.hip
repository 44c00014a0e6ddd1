// Multi-scale deformable attention in float64 for gfx950: the second type of the reference's dispatch
// (AT_DISPATCH_FLOATING_TYPES, CP/det3d/models/model_utils/ops/src/cuda/ms_deform_attn_cuda.cu:64, :129), the one its
// acceptance script ops/test.py runs (allclose against the torch core in double, torch.autograd.gradcheck).
//
// Semantics = csrc/msda.hip (ms_deform_im2col_cuda.cuh:33-84, 237-299): h_im = loc_y * H - 0.5, w_im = loc_x * W - 0.5, a
// sample contributes iff -1 < h_im < H and -1 < w_im < W, corners outside the map read 0.  Every operation is fp64.
//
// This is a CHECKING path (gradcheck, a full-tensor float64 reference on the device), so the kernels are generic rather than
// tuned: any D >= 1, any L and P, no matrix cores, no LDS tiles.  What they must be is reproducible -- gradcheck runs the
// backward twice and compares bit for bit -- so the backward has NO floating-point atomics:
//   * grad_sampling_loc / grad_attn_weight belong to one (n, q, m, l, p): a group of G lanes (G a function of D alone) sums
//     the D channels as a strided per-lane loop followed by a fixed xor-shuffle tree;
//   * grad_value is a store pass plus a per-destination sum pass.  Every sampling point has up to four in-map corners =
//     contributions, each with the id ((q * L + l) * P + p) * 4 + corner, unique within its destination row (n, s, m):
//       1. msda64_corners_kernel<false> counts the contributions per row (integer atomics: the totals are order-free),
//       2. exclusive_scan_u32 (common.hip) turns the counts into segment offsets,
//       3. msda64_corners_kernel<true> writes every id into its row's segment (slot from an integer atomic: any order),
//       4. msda64_sort_small_kernel / msda64_sort_big_kernel put every segment in ascending id order,
//       5. msda64_gather_kernel walks the ordered segment of a row, lanes across the channels, sums
//          bilinear weight x attention weight x grad_output in that order and stores the row once (zeros for an empty row).
//     The sum of a row therefore depends on the inputs alone.  Work and memory: O(points + rows), each times D.
#include "common.h"

namespace df3d {

struct Msda64Args {
  const double *value;
  const int64_t *shapes, *lstart;
  const double *loc, *aw, *gout;
  double *out, *gvalue, *gloc, *gaw;
  int N, S, M, D, Lq, L, P;
  uint32_t *count, *cursor, *offset, *ids, *tmp, *big, *nbig;   // backward workspace (see msda64_layout)
  int npass;                                                     // 4-bit digit passes of msda64_sort_big_kernel (even)
};

// one sampling point against its level: the top-left pixel, the fractions and which of the four corners lie in the map
// (bit k of `in`: 0 = (h_low, w_low), 1 = (h_low, w_high), 2 = (h_high, w_low), 3 = (h_high, w_high)); pix0 = the top-left
// pixel's index among the S value rows.  A level that does not fit into [0, S) has its stray corners dropped, not written.
struct Msda64Point {
  long long pix0;
  int W, in;
  double lh, lw, Hd, Wd;
};
__device__ __forceinline__ bool msda64_point(const Msda64Args &a, int l, double lx, double ly, Msda64Point &p) {
  const long long H = a.shapes[l * 2], W = a.shapes[l * 2 + 1], start = a.lstart[l];
  p.Hd = (double)H, p.Wd = (double)W, p.W = (int)W, p.in = 0;
  const double h_im = ly * p.Hd - 0.5, w_im = lx * p.Wd - 0.5;
  if (!(h_im > -1.0 && w_im > -1.0 && h_im < p.Hd && w_im < p.Wd)) return false;
  const double hf = floor(h_im), wf = floor(w_im);
  const long long h_low = (long long)hf, w_low = (long long)wf;
  p.lh = h_im - hf, p.lw = w_im - wf;
  p.pix0 = start + h_low * W + w_low;
  const bool top = h_low >= 0, bottom = h_low + 1 <= H - 1, left = w_low >= 0, right = w_low + 1 <= W - 1;
  const long long S = a.S;
  if (top && left && p.pix0 >= 0 && p.pix0 < S) p.in |= 1;
  if (top && right && p.pix0 + 1 >= 0 && p.pix0 + 1 < S) p.in |= 2;
  if (bottom && left && p.pix0 + W >= 0 && p.pix0 + W < S) p.in |= 4;
  if (bottom && right && p.pix0 + W + 1 >= 0 && p.pix0 + W + 1 < S) p.in |= 8;
  return true;
}
__device__ __forceinline__ long long msda64_corner_pix(const Msda64Point &p, int k) { return p.pix0 + (k >> 1) * (long long)p.W + (k & 1); }
__device__ __forceinline__ double msda64_corner_weight(const Msda64Point &p, int k) {
  return ((k >> 1) ? p.lh : 1.0 - p.lh) * ((k & 1) ? p.lw : 1.0 - p.lw);
}

// ---- forward: one thread per output channel (any D); consecutive lanes read consecutive channels of a value row ----------
__global__ __launch_bounds__(256) void msda64_forward_kernel(Msda64Args a) {
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long total = (long long)a.N * a.Lq * a.M * a.D;
  if (gid >= total) return;
  const int c = (int)(gid % a.D);
  const long long qm = gid / a.D;
  const int m = (int)(qm % a.M);
  const long long b = qm / ((long long)a.M * a.Lq);
  const int LP = a.L * a.P;
  const double *loc = a.loc + qm * LP * 2, *aw = a.aw + qm * LP;
  const long long qstride = (long long)a.M * a.D;
  const double *vbase = a.value + b * a.S * qstride + (long long)m * a.D + c;
  double acc = 0.0;
  for (int lp = 0; lp < LP; ++lp) {
    Msda64Point p;
    if (!msda64_point(a, lp / a.P, loc[lp * 2], loc[lp * 2 + 1], p)) continue;
    double v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = (p.in >> k) & 1 ? vbase[msda64_corner_pix(p, k) * qstride] : 0.0;
    const double hh = 1.0 - p.lh, hw = 1.0 - p.lw;
    acc += ((hh * hw) * v[0] + (hh * p.lw) * v[1] + (p.lh * hw) * v[2] + (p.lh * p.lw) * v[3]) * aw[lp];
  }
  a.out[gid] = acc;
}

// ---- backward, the location / weight half: G lanes per (n, q, m), lane `sub` owns channels sub, sub + G, ... -------------
template <int G>
__global__ __launch_bounds__(256) void msda64_point_grad_kernel(Msda64Args a) {
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long groups = (long long)a.N * a.Lq * a.M;
  const bool live = gid / G < groups;
  const long long qm = live ? gid / G : groups - 1;              // (idle lanes of the last wave follow the shuffles)
  const int sub = (int)(gid % G);
  const int m = (int)(qm % a.M);
  const long long b = qm / ((long long)a.M * a.Lq);
  const int LP = a.L * a.P;
  const double *loc = a.loc + qm * LP * 2, *aw = a.aw + qm * LP, *g = a.gout + qm * a.D;
  const long long qstride = (long long)a.M * a.D;
  const double *vbase = a.value + b * a.S * qstride + (long long)m * a.D;
  for (int lp = 0; lp < LP; ++lp) {
    Msda64Point p;
    double sw = 0.0, sx = 0.0, sy = 0.0;
    if (msda64_point(a, lp / a.P, loc[lp * 2], loc[lp * 2 + 1], p)) {
      const double hh = 1.0 - p.lh, hw = 1.0 - p.lw, w = aw[lp];
      for (int c = sub; c < a.D; c += G) {
        double v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = (p.in >> k) & 1 ? vbase[msda64_corner_pix(p, k) * qstride + c] : 0.0;
        const double tg = g[c] * w;                              // top_grad * attention weight
        sw += g[c] * ((hh * hw) * v[0] + (hh * p.lw) * v[1] + (p.lh * hw) * v[2] + (p.lh * p.lw) * v[3]);
        sx += tg * (hh * (v[1] - v[0]) + p.lh * (v[3] - v[2]));
        sy += tg * (hw * (v[2] - v[0]) + p.lw * (v[3] - v[1]));
      }
    }
#pragma unroll
    for (int d = 1; d < G; d <<= 1) {                            // the same tree whatever the launch
      sw += __shfl_xor(sw, d, 64);
      sx += __shfl_xor(sx, d, 64);
      sy += __shfl_xor(sy, d, 64);
    }
    if (live && sub == 0) {
      a.gloc[(qm * LP + lp) * 2] = p.Wd * sx;
      a.gloc[(qm * LP + lp) * 2 + 1] = p.Hd * sy;
      a.gaw[qm * LP + lp] = sw;
    }
  }
}

// ---- backward, the value half ------------------------------------------------------------------------------------------------
// passes 1 and 3: a thread per sampling point (n, q, m, l, p).  FILL = false: ++count[row] per in-map corner; FILL = true: the
// corner's id into slot offset[row] + cursor[row]++ (the order inside a segment is whatever the atomics gave: sorted next)
template <bool FILL>
__global__ __launch_bounds__(256) void msda64_corners_kernel(Msda64Args a) {
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int LP = a.L * a.P;
  if (gid >= (long long)a.N * a.Lq * a.M * LP) return;
  const int lp = (int)(gid % LP);
  const long long qm = gid / LP;
  const int m = (int)(qm % a.M);
  const long long q = (qm / a.M) % a.Lq, b = qm / ((long long)a.M * a.Lq);
  Msda64Point p;
  if (!msda64_point(a, lp / a.P, a.loc[gid * 2], a.loc[gid * 2 + 1], p)) return;
  const uint32_t id0 = (uint32_t)(q * LP + lp) * 4u;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (!((p.in >> k) & 1)) continue;
    const long long row = (b * a.S + msda64_corner_pix(p, k)) * a.M + m;
    if (FILL)
      a.ids[a.offset[row] + atomicAdd(&a.cursor[row], 1u)] = id0 + (uint32_t)k;
    else
      atomicAdd(&a.count[row], 1u);
  }
}

// pass 4a: a thread per row.  A segment of <= MSDA64_SMALL ids (nearly all of them) is ranked by counting the smaller ids -- they
// are unique -- through `tmp` and copied back; a longer one is noted in `big` for msda64_sort_big_kernel (the order of that
// list decides only which workgroup sorts which segment).
constexpr uint32_t MSDA64_SMALL = 32;
__global__ __launch_bounds__(256) void msda64_sort_small_kernel(Msda64Args a) {
  const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= (long long)a.N * a.S * a.M) return;
  const uint32_t first = a.offset[row], c = a.offset[row + 1] - first;
  if (c < 2) return;
  if (c > MSDA64_SMALL) {
    a.big[atomicAdd(a.nbig, 1u)] = (uint32_t)row;
    return;
  }
  uint32_t *ids = a.ids + first, *tmp = a.tmp + first;
  for (uint32_t i = 0; i < c; ++i) {
    const uint32_t key = ids[i];
    uint32_t rank = 0;
    for (uint32_t j = 0; j < c; ++j) rank += ids[j] < key ? 1u : 0u;
    tmp[rank] = key;
  }
  for (uint32_t i = 0; i < c; ++i) ids[i] = tmp[i];
}

// pass 4b: a workgroup per long segment (thousands of ids where many queries look at one pixel): a least-significant-digit
// radix sort, 4 bits per pass, ids <-> tmp.  Thread t owns a contiguous piece of the segment; a pass counts the piece's digits
// in the thread's own LDS column, scans the 16 x 256 counters in (digit, thread) order and moves the piece in order: stable,
// linear in the ids, no atomics.  npass is even (the host rounds up), so the result ends in `ids`.
__global__ __launch_bounds__(256) void msda64_sort_big_kernel(Msda64Args a) {
  __shared__ uint32_t s_cnt[16 * 256 + 16];                      // [digit][thread] (+ one pad word per 256: the scan's stride)
  __shared__ uint32_t s_wave[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t nbig = *a.nbig;
  for (uint32_t bi = blockIdx.x; bi < nbig; bi += gridDim.x) {
    const long long row = a.big[bi];
    const uint32_t first = a.offset[row], c = a.offset[row + 1] - first;
    const uint32_t per = (c + 255u) / 256u, i0 = min((uint32_t)tid * per, c), i1 = min(i0 + per, c);
    uint32_t *src = a.ids + first, *dst = a.tmp + first;
    for (int pass = 0; pass < a.npass; ++pass) {
      const int shift = pass * 4;
      for (int d = 0; d < 16; ++d) s_cnt[d * 257 + tid] = 0u;
      for (uint32_t i = i0; i < i1; ++i) s_cnt[((src[i] >> shift) & 15u) * 257 + tid] += 1u;
      __syncthreads();
      // exclusive scan of the 4096 counters in (digit, thread) order: thread t takes counters 16 t .. 16 t + 15
      uint32_t mine = 0;
      for (int k = 0; k < 16; ++k) {
        const int e = tid * 16 + k;
        mine += s_cnt[(e >> 8) * 257 + (e & 255)];
      }
      uint32_t incl = mine;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
      }
      if (lane == 63) s_wave[wave] = incl;
      __syncthreads();
      uint32_t run = incl - mine;
      for (int w = 0; w < wave; ++w) run += s_wave[w];
      for (int k = 0; k < 16; ++k) {
        const int e = tid * 16 + k, at = (e >> 8) * 257 + (e & 255);
        const uint32_t n = s_cnt[at];
        s_cnt[at] = run;
        run += n;
      }
      __syncthreads();
      for (uint32_t i = i0; i < i1; ++i) {
        const uint32_t key = src[i], at = ((key >> shift) & 15u) * 257 + tid;
        dst[s_cnt[at]++] = key;                                  // (slots < c by construction: the counters sum to c)
      }
      __syncthreads();                                           // (also orders this pass's global stores before the next reads)
      uint32_t *t = src;
      src = dst, dst = t;
    }
  }
}

// pass 5: G lanes per destination row (n, s, m), lane `sub` owns channels sub, sub + G, ...; the row's contributions in
// ascending id order, one store per element
template <int G>
__global__ __launch_bounds__(256) void msda64_gather_kernel(Msda64Args a) {
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long row = gid / G;
  if (row >= (long long)a.N * a.S * a.M) return;
  const int sub = (int)(gid % G);
  const int m = (int)(row % a.M);
  const long long b = row / ((long long)a.M * a.S);
  const int LP = a.L * a.P;
  const uint32_t first = a.offset[row], last = a.offset[row + 1];
  for (int c = sub; c < a.D; c += G) {
    double acc = 0.0;
    for (uint32_t i = first; i < last; ++i) {
      const uint32_t id = a.ids[i];
      const int k = (int)(id & 3u), lp = (int)((id >> 2) % (uint32_t)LP);
      const long long q = (id >> 2) / (uint32_t)LP, qm = (b * a.Lq + q) * a.M + m;
      Msda64Point p;
      msda64_point(a, lp / a.P, a.loc[(qm * LP + lp) * 2], a.loc[(qm * LP + lp) * 2 + 1], p);
      acc += msda64_corner_weight(p, k) * (a.aw[qm * LP + lp] * a.gout[qm * a.D + c]);
    }
    a.gvalue[row * a.D + c] = acc;
  }
}

// the backward's workspace: what the contribution ids (uint32) and the segment offsets (uint32) hold bounds the shape
struct Msda64Layout {
  size_t rows, contrib, nbig_max, bytes;
  const char *limit;                                             // non-null: why the shape is not served
};
static Msda64Layout msda64_layout(long long N, long long S, long long M, long long Lq, long long L, long long P) {
  Msda64Layout w = {0, 0, 0, 0, nullptr};
  const long long cap = 0x7fffffffLL;
  // (products of positive ints: checked factor by factor so that nothing overflows 64 bits)
  long long rows = N, contrib = N;
  for (long long f : {S, M}) rows = rows > cap / f ? cap + 1 : rows * f;
  for (long long f : {Lq, M, L, P, 4LL}) contrib = contrib > cap / f ? cap + 1 : contrib * f;
  if (rows >= cap) {
    w.limit = "ms_deform_attn_backward_f64: N * S * M value rows exceed 2^31 - 2 (uint32 segment offsets)";
    return w;
  }
  if (contrib > cap) {
    w.limit = "ms_deform_attn_backward_f64: N * Lq * M * L * P * 4 contributions exceed 2^31 - 1 (uint32 ids and offsets)";
    return w;
  }
  w.rows = (size_t)rows, w.contrib = (size_t)contrib, w.nbig_max = w.contrib / (MSDA64_SMALL + 1) + 1;
  size_t b = 0;
  b = arena_need(b, (2 * w.rows + 1) * sizeof(uint32_t));        // count | cursor | nbig: zeroed by one memset
  b = arena_need(b, (w.rows + 1) * sizeof(uint32_t));            // offset (+ the total)
  b = arena_need(b, w.contrib * sizeof(uint32_t));               // ids
  b = arena_need(b, w.contrib * sizeof(uint32_t));               // tmp
  b = arena_need(b, w.nbig_max * sizeof(uint32_t));              // big
  b = arena_need(b, scan_scratch_bytes(w.rows));
  w.bytes = align_up(b, 256);
  return w;
}

}  // namespace df3d

using namespace df3d;

extern "C" int df3d_ms_deform_attn_forward_f64(const double *value, const int64_t *spatial_shapes,
                                               const int64_t *level_start_index, const double *sampling_loc,
                                               const double *attn_weight, int N, int S, int M, int D, int Lq, int L, int P,
                                               double *out, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  DF3D_CHECK_ARG(N >= 0 && S > 0 && M > 0 && D > 0 && Lq >= 0 && L > 0 && P > 0, "ms_deform_attn_forward_f64: bad sizes");
  DF3D_CHECK_ARG((long long)L * P <= 0x7fffffffLL / 2, "ms_deform_attn_forward_f64: L * P exceeds 2^30");
  if (N == 0 || Lq == 0) return DF3D_OK;                         // (empty tensors have null data pointers)
  DF3D_CHECK_ARG(value && spatial_shapes && level_start_index && sampling_loc && attn_weight && out,
                 "ms_deform_attn_forward_f64: null argument");
  const double total = (double)N * Lq * M * D;
  DF3D_CHECK_ARG(total <= 256.0 * 2147483647.0, "ms_deform_attn_forward_f64: N * Lq * M * D exceeds 2^39 (the grid)");
  Msda64Args a = {};
  a.value = value, a.shapes = spatial_shapes, a.lstart = level_start_index, a.loc = sampling_loc, a.aw = attn_weight, a.out = out;
  a.N = N, a.S = S, a.M = M, a.D = D, a.Lq = Lq, a.L = L, a.P = P;
  hipLaunchKernelGGL(msda64_forward_kernel, dim3(cdiv((long long)N * Lq * M * D, 256)), dim3(256), 0, stream, a);
  DF3D_LAUNCH_CHECK();
  return DF3D_OK;
}

extern "C" size_t df3d_ms_deform_attn_backward_f64_workspace_bytes(int N, int S, int M, int Lq, int L, int P) {
  if (N <= 0 || S <= 0 || M <= 0 || Lq <= 0 || L <= 0 || P <= 0) return 256;     // (nothing to sort; never a null workspace)
  const Msda64Layout w = msda64_layout(N, S, M, Lq, L, P);
  if (w.limit) {
    set_error("%s", w.limit);
    return 0;
  }
  return w.bytes;
}

extern "C" int df3d_ms_deform_attn_backward_f64(const double *value, const int64_t *spatial_shapes,
                                                const int64_t *level_start_index, const double *sampling_loc,
                                                const double *attn_weight, const double *grad_output, int N, int S, int M,
                                                int D, int Lq, int L, int P, double *grad_value, double *grad_sampling_loc,
                                                double *grad_attn_weight, void *workspace, size_t workspace_bytes,
                                                void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  DF3D_CHECK_ARG(N >= 0 && S > 0 && M > 0 && D > 0 && Lq >= 0 && L > 0 && P > 0, "ms_deform_attn_backward_f64: bad sizes");
  if (N == 0) return DF3D_OK;                                    // (empty tensors have null data pointers)
  DF3D_CHECK_ARG(value && spatial_shapes && level_start_index && grad_value, "ms_deform_attn_backward_f64: null argument");
  if (Lq == 0) {                                                 // no sampling point: every row is empty
    DF3D_HIP(hipMemsetAsync(grad_value, 0, (size_t)N * S * M * D * sizeof(double), stream));
    return DF3D_OK;
  }
  DF3D_CHECK_ARG(sampling_loc && attn_weight && grad_output && grad_sampling_loc && grad_attn_weight && workspace,
                 "ms_deform_attn_backward_f64: null argument");
  const Msda64Layout w = msda64_layout(N, S, M, Lq, L, P);
  DF3D_CHECK_ARG(!w.limit, "%s", w.limit);
  DF3D_CHECK_ARG(workspace_bytes >= w.bytes, "ms_deform_attn_backward_f64: workspace of %zu bytes, %zu needed", workspace_bytes,
                 w.bytes);
  Arena ar(workspace, workspace_bytes);
  uint32_t *zeroed = ar.take<uint32_t>(2 * w.rows + 1);
  uint32_t *offset = ar.take<uint32_t>(w.rows + 1);
  uint32_t *ids = ar.take<uint32_t>(w.contrib), *tmp = ar.take<uint32_t>(w.contrib), *big = ar.take<uint32_t>(w.nbig_max);
  const size_t scan_bytes = scan_scratch_bytes(w.rows);
  char *scan = ar.take<char>(scan_bytes);
  DF3D_CHECK_ARG(zeroed && offset && ids && tmp && big && scan, "ms_deform_attn_backward_f64: workspace too small");
  Msda64Args a = {};
  a.value = value, a.shapes = spatial_shapes, a.lstart = level_start_index, a.loc = sampling_loc, a.aw = attn_weight;
  a.gout = grad_output, a.gvalue = grad_value, a.gloc = grad_sampling_loc, a.gaw = grad_attn_weight;
  a.N = N, a.S = S, a.M = M, a.D = D, a.Lq = Lq, a.L = L, a.P = P;
  a.count = zeroed, a.cursor = zeroed + w.rows, a.nbig = zeroed + 2 * w.rows, a.offset = offset, a.ids = ids, a.tmp = tmp, a.big = big;
  unsigned long long keys = (unsigned long long)Lq * L * P * 4 - 1;  // the largest id
  int bits = 1;
  while (keys >>= 1) ++bits;
  a.npass = (bits + 3) / 4;
  a.npass += a.npass & 1;
  DF3D_HIP(hipMemsetAsync(zeroed, 0, (2 * w.rows + 1) * sizeof(uint32_t), stream));
  const long long points = (long long)(w.contrib / 4);
  hipLaunchKernelGGL(msda64_corners_kernel<false>, dim3(cdiv(points, 256)), dim3(256), 0, stream, a);
  DF3D_LAUNCH_CHECK();
  const int rc = exclusive_scan_u32(a.count, offset, w.rows, offset + w.rows, scan, scan_bytes, stream);
  if (rc != DF3D_OK) return rc;
  hipLaunchKernelGGL(msda64_corners_kernel<true>, dim3(cdiv(points, 256)), dim3(256), 0, stream, a);
  hipLaunchKernelGGL(msda64_sort_small_kernel, dim3(cdiv((long long)w.rows, 256)), dim3(256), 0, stream, a);
  const long long nbig_blocks = (long long)w.nbig_max < 2048 ? (long long)w.nbig_max : 2048;
  hipLaunchKernelGGL(msda64_sort_big_kernel, dim3((unsigned)nbig_blocks), dim3(256), 0, stream, a);
  DF3D_LAUNCH_CHECK();
  const long long groups = (long long)N * Lq * M;
#define DF3D_MSDA64_CASE(G)                                                                                              \
  hipLaunchKernelGGL(msda64_gather_kernel<G>, dim3(cdiv((long long)w.rows * G, 256)), dim3(256), 0, stream, a);          \
  hipLaunchKernelGGL(msda64_point_grad_kernel<G>, dim3(cdiv(groups * G, 256)), dim3(256), 0, stream, a);
  // lanes per row / per (query, head): a function of D alone, so the channel sums' order is one per D
  if (D <= 1) {
    DF3D_MSDA64_CASE(1)
  } else if (D <= 4) {
    DF3D_MSDA64_CASE(4)
  } else if (D <= 16) {
    DF3D_MSDA64_CASE(16)
  } else {
    DF3D_MSDA64_CASE(64)
  }
#undef DF3D_MSDA64_CASE
  DF3D_LAUNCH_CHECK();
  return DF3D_OK;
}
