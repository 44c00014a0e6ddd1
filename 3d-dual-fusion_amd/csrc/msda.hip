// Multi-scale deformable attention forward for gfx950.
//
// Semantics = the reference kernel ms_deformable_im2col_gpu_kernel
// (CP/det3d/models/model_utils/ops/src/cuda/ms_deform_im2col_cuda.cuh:237-299, bilinear
// helper :33-84): h_im = loc_h*H - 0.5, w_im = loc_w*W - 0.5; a sample contributes iff
// -1 < h_im < H and -1 < w_im < W; corners outside the map read 0;
// out[b,q,m,:] = sum_{l,p} w[b,q,m,l,p] * bilinear(value[b, level l, m, :]).
//
// The reference runs one thread per output CHANNEL (16 lanes repeat the same index math and
// share one 64-byte fetch) in 1024-thread blocks, chunked over the batch by im2col_step.
// Here a lane owns VEC=4 channels (one 16-byte load per corner), so D=16 needs 4 lanes per
// (query, head): a wave covers 16 (q, m) pairs = two whole queries of the 8-head layout, its
// 64 x 16 B stores are one contiguous 1 KiB segment, and the four lanes of a (q, m) group
// split the sampling points between them: each lane fetches one point's (x, y, w) and the
// group exchanges them with wave shuffles instead of re-reading them 16 times.
// Algorithmic bytes: min(N*S*M*D, N*Lq*M*L*P*4*D)*4 + N*Lq*M*L*P*3*4 +
// N*Lq*M*D*4.  Bound: HBM/L2 gather bandwidth (10 flop per fetched element).
#include "common.h"

namespace df3d {

struct MsdaArgs {
  const float *value;
  const int64_t *shapes, *lstart;
  const float *loc, *aw;
  float *out;
  int N, S, M, D, Lq, L, P;
};

// Fast path: D % 4 == 0 and (D/4) a power of two <= 16 (D = 4, 8, 16, 32, 64).
template <int LPG /*lanes per (q,m) group = D/4*/>
__global__ __launch_bounds__(256) void msda_vec4_kernel(MsdaArgs a) {
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;  // over N*Lq*M*LPG
  const long long total = (long long)a.N * a.Lq * a.M * LPG;
  const bool live = gid < total;
  const long long qm = live ? gid / LPG : (total - 1) / LPG;  // (b*Lq + q)*M + m
  const int sub = (int)(gid % LPG);
  const int m = (int)(qm % a.M);
  const int b = (int)(qm / ((long long)a.M * a.Lq));
  const int LP = a.L * a.P;
  const float *loc = a.loc + (size_t)qm * LP * 2;
  const float *aw = a.aw + (size_t)qm * LP;
  const int lane = threadIdx.x & 63;
  const int gbase = lane & ~(LPG - 1);
  const int qstride = a.M * a.D;
  f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int lp0 = 0; lp0 < LP; lp0 += LPG) {
    // lane `sub` of the group fetches point lp0+sub
    float mx = 0.f, my = 0.f, mw = 0.f;
    int lp = lp0 + sub;
    if (lp < LP) {
      mx = loc[lp * 2];
      my = loc[lp * 2 + 1];
      mw = aw[lp];
    }
    const int cnt = (LP - lp0) < LPG ? (LP - lp0) : LPG;
    for (int i = 0; i < cnt; ++i) {
      float lx = __shfl(mx, gbase + i, 64);
      float ly = __shfl(my, gbase + i, 64);
      float w = __shfl(mw, gbase + i, 64);
      int l = (lp0 + i) / a.P;
      int H = (int)a.shapes[l * 2], W = (int)a.shapes[l * 2 + 1];
      const float *vbase = a.value + ((size_t)b * a.S + (size_t)a.lstart[l]) * qstride + m * a.D + sub * 4;
      float h_im = ly * (float)H - 0.5f;
      float w_im = lx * (float)W - 0.5f;
      if (h_im > -1.f && w_im > -1.f && h_im < (float)H && w_im < (float)W) {
        int h_low = (int)floorf(h_im), w_low = (int)floorf(w_im);
        int h_high = h_low + 1, w_high = w_low + 1;
        float lh = h_im - (float)h_low, lw = w_im - (float)w_low;
        float hh = 1.f - lh, hw = 1.f - lw;
        f32x4 z = (f32x4){0.f, 0.f, 0.f, 0.f};
        f32x4 v1 = z, v2 = z, v3 = z, v4 = z;
        const size_t hs = (size_t)W * qstride;
        if (h_low >= 0 && w_low >= 0) v1 = *(const f32x4 *)(vbase + h_low * hs + (size_t)w_low * qstride);
        if (h_low >= 0 && w_high <= W - 1) v2 = *(const f32x4 *)(vbase + h_low * hs + (size_t)w_high * qstride);
        if (h_high <= H - 1 && w_low >= 0) v3 = *(const f32x4 *)(vbase + h_high * hs + (size_t)w_low * qstride);
        if (h_high <= H - 1 && w_high <= W - 1) v4 = *(const f32x4 *)(vbase + h_high * hs + (size_t)w_high * qstride);
        float w1 = hh * hw, w2 = hh * lw, w3 = lh * hw, w4 = lh * lw;
        acc += (w1 * v1 + w2 * v2 + w3 * v3 + w4 * v4) * w;
      }
    }
  }
  if (live) *(f32x4 *)(a.out + (size_t)qm * a.D + sub * 4) = acc;
}

// General path: one thread per output channel (any D).
__global__ __launch_bounds__(256) void msda_scalar_kernel(MsdaArgs a) {
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long total = (long long)a.N * a.Lq * a.M * a.D;
  if (gid >= total) return;
  const int c = (int)(gid % a.D);
  const long long qm = gid / a.D;
  const int m = (int)(qm % a.M);
  const int b = (int)(qm / ((long long)a.M * a.Lq));
  const int LP = a.L * a.P;
  const float *loc = a.loc + (size_t)qm * LP * 2;
  const float *aw = a.aw + (size_t)qm * LP;
  const int qstride = a.M * a.D;
  float acc = 0.f;
  for (int l = 0; l < a.L; ++l) {
    int H = (int)a.shapes[l * 2], W = (int)a.shapes[l * 2 + 1];
    const float *vbase = a.value + ((size_t)b * a.S + (size_t)a.lstart[l]) * qstride + m * a.D + c;
    for (int p = 0; p < a.P; ++p) {
      float lx = loc[(l * a.P + p) * 2], ly = loc[(l * a.P + p) * 2 + 1], w = aw[l * a.P + p];
      float h_im = ly * (float)H - 0.5f;
      float w_im = lx * (float)W - 0.5f;
      if (h_im > -1.f && w_im > -1.f && h_im < (float)H && w_im < (float)W) {
        int h_low = (int)floorf(h_im), w_low = (int)floorf(w_im);
        int h_high = h_low + 1, w_high = w_low + 1;
        float lh = h_im - (float)h_low, lw = w_im - (float)w_low;
        float hh = 1.f - lh, hw = 1.f - lw;
        float v1 = 0.f, v2 = 0.f, v3 = 0.f, v4 = 0.f;
        const size_t hs = (size_t)W * qstride;
        if (h_low >= 0 && w_low >= 0) v1 = vbase[h_low * hs + (size_t)w_low * qstride];
        if (h_low >= 0 && w_high <= W - 1) v2 = vbase[h_low * hs + (size_t)w_high * qstride];
        if (h_high <= H - 1 && w_low >= 0) v3 = vbase[h_high * hs + (size_t)w_low * qstride];
        if (h_high <= H - 1 && w_high <= W - 1) v4 = vbase[h_high * hs + (size_t)w_high * qstride];
        float w1 = hh * hw, w2 = hh * lw, w3 = lh * hw, w4 = lh * lw;
        acc += (w1 * v1 + w2 * v2 + w3 * v3 + w4 * v4) * w;
      }
    }
  }
  a.out[gid] = acc;
}


// ---------------------------------------------------------------------------------------------------------
// Backward.  Reference: ms_deformable_col2im_gpu_kernel* and
// ms_deform_attn_col2im_bilinear (ms_deform_im2col_cuda.cuh:87-232, 301-921): per (b, q, m, c) and sampling point
//   grad_value[corner]   += w_corner * attn * g                (atomics; four corners, zero outside the map)
//   grad_attn[b,q,m,l,p] += g * bilinear(value)                (sum over the D channels)
//   grad_loc[..,0]       += W * (dval/dw_im) * attn * g        (x), grad_loc[..,1] += H * (dval/dh_im) * attn * g (y)
// with dval/dh_im = -hw*v1 - lw*v2 + hw*v3 + lw*v4 and dval/dw_im = -hh*v1 + hh*v2 - lh*v3 + lh*v4.
// The reference has seven kernel variants that differ in how the channel sums are reduced (shared memory trees,
// block-size specialisations, global atomics for > 1024 channels).  Here the forward's layout is reused: a lane owns
// four channels, the D/4 lanes of a (q, m) group reduce the two location gradients and the weight gradient with
// wave shuffles (no LDS, no atomics for them), and the value gradient uses the hardware fp32 atomic add.
struct MsdaBwdArgs {
  const float *value;
  const int64_t *shapes, *lstart;
  const float *loc, *aw, *gout;
  float *gvalue, *gloc, *gaw;
  int N, S, M, D, Lq, L, P;
  unsigned char *nz;          // [N * Lq * M]: 1 = the group's upstream gradient is not all zero (binned path)
};

__device__ __forceinline__ void atomic_add4(float *p, f32x4 v) {
  unsafeAtomicAdd(p, v[0]);
  unsafeAtomicAdd(p + 1, v[1]);
  unsafeAtomicAdd(p + 2, v[2]);
  unsafeAtomicAdd(p + 3, v[3]);
}

// BINNED: the value gradient is accumulated by msda_bin_* below (LDS tiles); this kernel then only computes the location /
// weight gradients and notes which (query, head) groups carry a gradient at all (a.nz)
template <int LPG, bool BINNED = false>
__global__ __launch_bounds__(256) void msda_bwd_vec4_kernel(MsdaBwdArgs a) {
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long total = (long long)a.N * a.Lq * a.M * LPG;
  const bool live = gid < total;
  const long long qm = live ? gid / LPG : (total - 1) / LPG;
  const int sub = (int)(gid % LPG);
  const int m = (int)(qm % a.M);
  const int b = (int)(qm / ((long long)a.M * a.Lq));
  const int LP = a.L * a.P;
  const float *loc = a.loc + (size_t)qm * LP * 2;
  const float *aw = a.aw + (size_t)qm * LP;
  const int lane = threadIdx.x & 63;
  const int gbase = lane & ~(LPG - 1);
  const int qstride = a.M * a.D;
  f32x4 g = (f32x4){0.f, 0.f, 0.f, 0.f};
  if (live) g = *(const f32x4 *)(a.gout + (size_t)qm * a.D + sub * 4);
  // A (query, head) whose upstream gradient is all zero contributes nothing: every product below carries g.  The padded
  // rows of the zero-padded per-camera query lists are exactly that (nobody reads their outputs), and they all sample around
  // reference point (0, 0): ~8 k rows per image adding zeros to the same few cache lines of grad_value (the atomics of one line
  // serialise in the L2: 3.4 ms per call at the TransFusion training shape, 0.12 ms for the forward).
  int nz = (g[0] != 0.f) | (g[1] != 0.f) | (g[2] != 0.f) | (g[3] != 0.f);
#pragma unroll
  for (int d = 1; d < LPG; d <<= 1) nz |= __shfl_xor(nz, d, 64);
  const bool work = live && nz;
  if (BINNED && live && sub == 0) a.nz[qm] = (unsigned char)(nz != 0);
  for (int lp0 = 0; lp0 < LP; lp0 += LPG) {
    float mx = 0.f, my = 0.f, mw = 0.f;
    const int lp = lp0 + sub;
    if (lp < LP) {
      mx = loc[lp * 2];
      my = loc[lp * 2 + 1];
      mw = aw[lp];
    }
    float keep_x = 0.f, keep_y = 0.f, keep_w = 0.f;       // gradients of the point this lane fetched
    const int cnt = (LP - lp0) < LPG ? (LP - lp0) : LPG;
    for (int i = 0; i < cnt; ++i) {
      const float lx = __shfl(mx, gbase + i, 64), ly = __shfl(my, gbase + i, 64), w = __shfl(mw, gbase + i, 64);
      const int l = (lp0 + i) / a.P;
      const int H = (int)a.shapes[l * 2], W = (int)a.shapes[l * 2 + 1];
      const size_t off = ((size_t)b * a.S + (size_t)a.lstart[l]) * qstride + m * a.D + sub * 4;
      const float h_im = ly * (float)H - 0.5f, w_im = lx * (float)W - 0.5f;
      float px = 0.f, py = 0.f, pw = 0.f;
      if (work && h_im > -1.f && w_im > -1.f && h_im < (float)H && w_im < (float)W) {
        const int h_low = (int)floorf(h_im), w_low = (int)floorf(w_im);
        const int h_high = h_low + 1, w_high = w_low + 1;
        const float lh = h_im - (float)h_low, lw = w_im - (float)w_low;
        const float hh = 1.f - lh, hw = 1.f - lw;
        const f32x4 z = (f32x4){0.f, 0.f, 0.f, 0.f};
        f32x4 v1 = z, v2 = z, v3 = z, v4 = z;
        const size_t hs = (size_t)W * qstride;
        const f32x4 tg = g * w;                              // top_grad * attention weight
        const size_t o1 = off + h_low * hs + (size_t)w_low * qstride, o2 = off + h_low * hs + (size_t)w_high * qstride;
        const size_t o3 = off + h_high * hs + (size_t)w_low * qstride, o4 = off + h_high * hs + (size_t)w_high * qstride;
        if (h_low >= 0 && w_low >= 0) {
          v1 = *(const f32x4 *)(a.value + o1);
          if (!BINNED) atomic_add4(a.gvalue + o1, tg * (hh * hw));
        }
        if (h_low >= 0 && w_high <= W - 1) {
          v2 = *(const f32x4 *)(a.value + o2);
          if (!BINNED) atomic_add4(a.gvalue + o2, tg * (hh * lw));
        }
        if (h_high <= H - 1 && w_low >= 0) {
          v3 = *(const f32x4 *)(a.value + o3);
          if (!BINNED) atomic_add4(a.gvalue + o3, tg * (lh * hw));
        }
        if (h_high <= H - 1 && w_high <= W - 1) {
          v4 = *(const f32x4 *)(a.value + o4);
          if (!BINNED) atomic_add4(a.gvalue + o4, tg * (lh * lw));
        }
        const f32x4 val = (hh * hw) * v1 + (hh * lw) * v2 + (lh * hw) * v3 + (lh * lw) * v4;
        const f32x4 dh = hw * (v3 - v1) + lw * (v4 - v2), dw = hh * (v2 - v1) + lh * (v4 - v3);
        pw = hsum4(g * val);
        px = (float)W * hsum4(dw * tg);
        py = (float)H * hsum4(dh * tg);
      }
#pragma unroll
      for (int d = 1; d < LPG; d <<= 1) {                    // sum over the lanes (channel quads) of the group
        px += __shfl_xor(px, d, 64);
        py += __shfl_xor(py, d, 64);
        pw += __shfl_xor(pw, d, 64);
      }
      if (sub == i) {
        keep_x = px;
        keep_y = py;
        keep_w = pw;
      }
    }
    if (live && lp < LP) {
      a.gloc[((size_t)qm * LP + lp) * 2] = keep_x;
      a.gloc[((size_t)qm * LP + lp) * 2 + 1] = keep_y;
      a.gaw[(size_t)qm * LP + lp] = keep_w;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// Value gradient WITHOUT global atomics (msda_bin_*): L >= 1 levels with L * P <= 16, heads of 16 / 32 / 64 channels.  Round 6
// wrote it for one single-level map with 16-channel heads, DESIGN 7.7 widened it; both shapes run the ONE set of kernels below
// (df3d_ms_deform_attn_backward_binned is df3d_ms_deform_attn_backward_binned_ml with L = 1).  The col2im above issues 16 scalar
// fp32 atomics per lane and sampling point: 0.5 G atomics per call at the TransFusion training shape (24 maps x ~10 k queries x 8
// heads x 4 points x 4 corners x 16 channels), and the L2's atomic units retire ~80 G of them per second whatever their scope or
// spread (tools/debug/msda_bwd_probe.py: 5.0 ms with uniformly spread queries, 5.3 ms with a third of them on one pixel) -- 3 ms
// per layer in the step against 0.12 ms for the forward.  Accumulating tiles in LDS with ds_add_f32 (first attempt) retires
// ~0.4 lanes per clock and CU and collapses where thousands of queries share a pixel (the unseen voxels' reference point).
// The col2im of a tile IS a matrix product:  footprint[81 px][16 ch] = Wt[81 px][points] . G[points][16 ch],  Wt = the
// bilinear weights (four non-zeros per column), G = attention weight x upstream gradient -- dense in the accumulator, so a
// pile-up on one pixel costs nothing.  Hence:
//   1. the sampling points are counting-sorted by (map, level, 8 x 8 pixel tile of their top-left corner, head): LDS histograms
//      per workgroup, one range reservation per workgroup and bin (msda_bin_kernel, msda_bin_scan_kernel);
//   2. a WAVE per <= 512 points of a bin runs the product on v_mfma_f32_16x16x4_f32 (exact fp32 products): six 16-pixel row
//      tiles of the 9 x 9 footprint (tile + one-pixel halo: the four corners of a point stay inside), A operand = the weights
//      formed in registers from (footprint index, lh, lw), B operand = the gradient row, and stores its footprint as a slab;
//   3. a gather kernel adds the slabs of a tile and the halo row / column / corner of its three neighbours into grad_value:
//      every element written exactly once -- no atomics, no zero fill.
// A bin is a (level, tile, head): the levels' tiles are numbered one level after the other (tbase), every level has its own map
// size, tile row length and first pixel, and grad_value [N][S][M][D] is written exactly once because the levels tile S without
// gaps (checked on the host: df3d_ms_deform_attn_backward_plan).  A head of D = 16 * NS channels is NS column slices of the same
// product: the A operand (the bilinear weights) is formed once per point and row tile and multiplies NS gradient rows, the
// slab is [81][D].
//
// ORDERED (df3d_ms_deform_attn_backward_binned_ml(..., ordered = 1)): the scatter of msda_bin_kernel leaves the points of a bin
// in the order in which lanes and workgroups won LDS / global integer atomics, and the fp32 sums of the accumulate kernel follow
// that order.  msda_bin_sort_kernel puts every bin's packed ids (q << 4 | lp, unique within a bin) in ascending order first; the
// work items are then every MB_CHUNK ids of that sequence, so grad_value is a function of the inputs alone.  A workgroup per
// bin: <= 64 ids are ranked by counting inside one wave, <= 1024 go through a bitonic network in LDS, and a larger bin (the
// pile-up on the unseen voxels' reference point: thousands to tens of thousands of ids) is written out from a bit directory --
// one bit per possible id in 256 Ki-id windows, set with LDS integer atomics, read back in order with a popcount scan: linear
// in the ids (the network's log^2 passes over 8192 ids cost more than the rest of the backward at the training shape).
constexpr int MB_T = 8, MB_FOOT = (MB_T + 1) * (MB_T + 1), MB_CHUNK = 512, MB_D = 16;
constexpr int MB_LMAX = 16, MS_WORDS = 8192, MS_WINDOW = MS_WORDS * 32, MS_NETWORK = 1024;
#define MS_PHYS(i) ((i) + ((i) >> 5))                         // (a thread walks 32 consecutive words: one pad word per 32)

// Everything below is per MAP n (blockIdx.y): bins, point ranges, work items and slabs are numbered within the map, so no
// prefix sum crosses maps (nbm = tiles * M bins, ppm = Lq * M * LP point slots, mw = nbm + ppm / MB_CHUNK + 1 work items).
struct MsdaMlArgs {
  const float *loc, *aw, *gout;
  const unsigned char *nz;
  float *gvalue;
  int N, S, M, D, Lq, L, P, LP, nbm, mw;
  int H[MB_LMAX], W[MB_LMAX], tx[MB_LMAX], start[MB_LMAX], tbase[MB_LMAX + 1];   // per level; tbase: first tile of the level
  unsigned *count, *cursor, *offset;                          // [N][nbm]: points of a bin; scatter cursor; first point slot
  unsigned *binw;                                             // [N][nbm + 1]: first work item of a bin
  unsigned *nwork;                                            // [N]
  unsigned *work;                                             // [N][mw][3]: (bin, first, last)
  const unsigned *items;                                      // what the accumulate kernel reads (the ordered copy if there is one)
  unsigned *scattered, *sorted;                               // [N][ppm] each: the scatter's output; the ordered copy
  float *slabs;                                               // [N][mw][MB_FOOT][D]: the work items' footprints
};
// what the scan kernel reads and writes of the above
struct MsdaScanArgs {
  unsigned *count, *offset, *binw, *nwork, *work;
  int nbm, mw;
};

__device__ __forceinline__ bool mb_point_hw(int H, int W, float lx, float ly, int &hl, int &wl, float &lh, float &lw) {
  const float h_im = ly * (float)H - 0.5f, w_im = lx * (float)W - 0.5f;
  const bool in = h_im > -1.f && w_im > -1.f && h_im < (float)H && w_im < (float)W;
  hl = (int)floorf(h_im), wl = (int)floorf(w_im);
  lh = h_im - (float)hl, lw = w_im - (float)wl;
  return in;
}
// ONE_LEVEL (a compile-time copy of L == 1) folds the level of a point or tile and the index into the per-level arrays to
// constants in the bin, accumulate and reduce kernels: found at run time they cost the single-level training shape 15 us per call,
// 12 of them in the accumulate kernel
template <bool ONE_LEVEL>
__device__ __forceinline__ int mb_level_of_tile(const MsdaMlArgs &a, int tile) {
  if (ONE_LEVEL) return 0;
  int l = 0;
  while (l + 1 < a.L && tile >= a.tbase[l + 1]) ++l;
  return l;
}

// pass 1 (SCATTER = false): points per (level, tile, head) of map blockIdx.y; pass 2 (SCATTER = true): the points' packed ids
// into their bin's range.  A thread owns one (q, m) group and walks its L * P points; the level of a point decides map size
// and tile numbering.
template <bool SCATTER, bool ONE_LEVEL>
__global__ __launch_bounds__(256) void msda_bin_kernel(MsdaMlArgs a) {
  extern __shared__ unsigned mb_hist[];                      // [nbm] counts, then (scatter) [nbm] bases
  const int n = blockIdx.y, tid = threadIdx.x, nbm = a.nbm;
  for (int t = tid; t < nbm; t += 256) mb_hist[t] = 0u;
  __syncthreads();
  const long long g = (long long)blockIdx.x * 256 + tid;     // (q, m) of this map
  const bool live = g < (long long)a.Lq * a.M && a.nz[(size_t)n * a.Lq * a.M + g];
  const int m = (int)(g % a.M);
  const float *loc = a.loc + ((size_t)n * a.Lq * a.M + (size_t)(live ? g : 0)) * a.LP * 2;
  unsigned rank[16];
  int bin[16];
#pragma unroll 1
  for (int lp = 0; lp < a.LP; ++lp) {
    bin[lp & 15] = -1;
    if (!live) continue;
    const int l = ONE_LEVEL ? 0 : lp / a.P;
    int hl, wl;
    float lh, lw;
    if (!mb_point_hw(a.H[l], a.W[l], loc[lp * 2], loc[lp * 2 + 1], hl, wl, lh, lw)) continue;
    const int t = (a.tbase[l] + (max(hl, 0) / MB_T) * a.tx[l] + max(wl, 0) / MB_T) * a.M + m;
    bin[lp & 15] = t;
    rank[lp & 15] = atomicAdd(&mb_hist[t], 1u);
  }
  __syncthreads();
  if (!SCATTER) {
    for (int t = tid; t < nbm; t += 256)
      if (mb_hist[t]) atomicAdd(&a.count[(size_t)n * nbm + t], mb_hist[t]);
    return;
  }
  unsigned *base = mb_hist + nbm;
  for (int t = tid; t < nbm; t += 256)
    base[t] = mb_hist[t] ? a.offset[(size_t)n * nbm + t] + atomicAdd(&a.cursor[(size_t)n * nbm + t], mb_hist[t]) : 0u;
  __syncthreads();
  if (!live) return;
  const unsigned q = (unsigned)(g / a.M);
  unsigned *items = a.scattered + (size_t)n * a.Lq * a.M * a.LP;
  for (int lp = 0; lp < a.LP; ++lp)
    if (bin[lp & 15] >= 0) items[base[bin[lp & 15]] + rank[lp & 15]] = (q << 4) | (unsigned)lp;
}

// exclusive scan of one map's bin counts + its work list: a bin with c points becomes ceil(c / MB_CHUNK) work items.  1024
// threads, <= 8 consecutive bins per thread (nbm <= 7680), the (points, work items) pair scanned through wave shuffles.
__global__ __launch_bounds__(1024) void msda_bin_scan_kernel(MsdaScanArgs a) {
  __shared__ unsigned long long s_wave[16];
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nbm = a.nbm;
  const int per = (nbm + 1023) / 1024, b0 = min(tid * per, nbm), b1 = min(b0 + per, nbm);
  const unsigned *count = a.count + (size_t)n * nbm;
  unsigned c[8];
  unsigned long long mine = 0;                                 // low word: points; high word: work items
  for (int b = b0, k = 0; b < b1; ++b, ++k) {
    c[k] = count[b];
    mine += (unsigned long long)c[k] | ((unsigned long long)((c[k] + MB_CHUNK - 1) / MB_CHUNK) << 32);
  }
  unsigned long long incl = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long up = __shfl_up(incl, d);
    if (lane >= d) incl += up;
  }
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  unsigned long long before = incl - mine;
  for (int w = 0; w < wave; ++w) before += s_wave[w];
  unsigned run = (unsigned)before, wrun = (unsigned)(before >> 32);
  unsigned *offset = a.offset + (size_t)n * nbm, *binw = a.binw + (size_t)n * (nbm + 1), *work = a.work + (size_t)n * a.mw * 3;
  for (int b = b0, k = 0; b < b1; ++b, ++k) {
    offset[b] = run;
    binw[b] = wrun;
    for (unsigned s0 = 0; s0 < c[k]; s0 += MB_CHUNK, ++wrun)
      work[wrun * 3] = b, work[wrun * 3 + 1] = run + s0, work[wrun * 3 + 2] = run + min(s0 + (unsigned)MB_CHUNK, c[k]);
    run += c[k];
  }
  if (tid == 1023) binw[nbm] = wrun, a.nwork[n] = wrun;
}

// a workgroup = one bin of map blockIdx.y: its ids from `scattered` to `sorted`, ascending (see ORDERED above).  Two launches
// over the bins: BIG = false takes the bins of <= MS_NETWORK ids (nearly all of them) with 4 KB of LDS, BIG = true the rest with
// the 33 KB of the bit directory -- one kernel for both holds every small bin to the large ones' four workgroups per CU.
template <bool BIG>
__global__ __launch_bounds__(256) void msda_bin_sort_kernel(MsdaMlArgs a) {
  constexpr int WORDS = BIG ? MS_WORDS : MS_NETWORK;
  __shared__ unsigned s[WORDS + WORDS / 32];
  __shared__ unsigned s_wave[4];
  const int n = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t bi = (size_t)n * a.nbm + blockIdx.x, first = (size_t)n * a.Lq * a.M * a.LP + a.offset[bi];
  const unsigned c = a.count[bi];
  const unsigned *src = a.scattered + first;
  unsigned *dst = a.sorted + first;
  if (c == 0 || BIG != (c > (unsigned)MS_NETWORK)) return;
  if (!BIG && c <= 64) {                                       // rank = the number of smaller ids (one wave, no LDS)
    if (wave) return;
    const unsigned key = (unsigned)lane < c ? src[lane] : 0xffffffffu;
    unsigned rank = 0;
    for (unsigned j = 0; j < c; ++j) rank += (unsigned)__shfl(key, (int)j, 64) < key ? 1u : 0u;
    if ((unsigned)lane < c) dst[rank] = key;
    return;
  }
  if (!BIG) {                                                  // bitonic network over the next power of two (pad = ~0 > any id)
    unsigned n2 = 128;
    while (n2 < c) n2 <<= 1;
    for (unsigned i = tid; i < n2; i += 256) s[i] = i < c ? src[i] : 0xffffffffu;
    __syncthreads();
    for (unsigned k = 2; k <= n2; k <<= 1)
      for (unsigned j = k >> 1; j > 0; j >>= 1) {
        for (unsigned i = tid; i < n2; i += 256) {
          const unsigned p = i ^ j;
          if (p > i) {
            const unsigned x = s[i], y = s[p];
            if ((x > y) == ((i & k) == 0u)) s[i] = y, s[p] = x;
          }
        }
        __syncthreads();
      }
    for (unsigned i = tid; i < c; i += 256) dst[i] = s[i];
    return;
  }
  const unsigned nkeys = (unsigned)a.Lq << 4;                  // (Lq <= 2^20 in ordered mode: no overflow, <= 64 windows)
  unsigned done = 0;
  for (unsigned k0 = 0; k0 < nkeys; k0 += MS_WINDOW) {
    for (int i = tid; i < WORDS + WORDS / 32; i += 256) s[i] = 0u;
    __syncthreads();
    for (unsigned i = tid; i < c; i += 256) {
      const unsigned k = src[i] - k0;                          // (an id below the window wraps to a large number)
      if (k < (unsigned)MS_WINDOW) atomicOr(&s[MS_PHYS(k >> 5)], 1u << (k & 31u));
    }
    __syncthreads();
    const unsigned w0 = tid * 32;                              // this thread's 32 words = 1024 ids of the window
    unsigned mine = 0;
    for (unsigned w = 0; w < 32; ++w) mine += __popc(s[MS_PHYS(w0 + w)]);
    unsigned incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned up = __shfl_up(incl, d);
      if (lane >= d) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    unsigned run = done + incl - mine;
    for (int w = 0; w < wave; ++w) run += s_wave[w];
    done += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    for (unsigned w = 0; w < 32; ++w) {
      unsigned bits = s[MS_PHYS(w0 + w)];
      while (bits) {
        dst[run++] = k0 + ((w0 + w) << 5) + (unsigned)(__ffs(bits) - 1);
        bits &= bits - 1u;
      }
    }
    __syncthreads();                                           // (s and s_wave are rewritten by the next window)
  }
}

// a wave = one work item: <= MB_CHUNK points of one (map, level, tile, head), NS slices of 16 channels.  MFMA operand layout
// (v_mfma_f32_16x16x4_f32): lane (i = lane & 15, k = lane >> 4) holds A[i][k] and B[k][i]; the accumulator of row tile rt holds
// footprint pixels rt * 16 + 4 * (lane >> 4) + r of channel lane & 15 of the slice.  Four points per matrix instruction, sixteen
// per loop pass; the ids of pass k + 2 and the locations / weights / gradient rows of pass k + 1 are in flight while pass k
// multiplies.
template <int NS>
struct MbPoints {
  float lx[4], ly[4], aw[4], g[4][NS];
};
template <int NS, bool ONE_LEVEL>
__global__ __launch_bounds__(256) void msda_bin_accumulate_kernel(MsdaMlArgs a) {
  constexpr int D = NS * 16;
  const int n = blockIdx.y, lane = threadIdx.x & 63, wid = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wid >= (int)a.nwork[n]) return;
  const unsigned *work = a.work + ((size_t)n * a.mw + wid) * 3;
  const unsigned bin = work[0], first = work[1], last = work[2];
  const int tg = bin / a.M, m = bin - tg * a.M, lv = mb_level_of_tile<ONE_LEVEL>(a, tg), t = tg - a.tbase[lv];
  const int H = a.H[lv], W = a.W[lv], tx = a.tx[lv];
  const int y0 = (t / tx) * MB_T, x0 = (t % tx) * MB_T;
  const int i16 = lane & 15, kg = lane >> 4;
  const unsigned *items = a.items + (size_t)n * a.Lq * a.M * a.LP;
  auto load_ids = [&](unsigned i0, unsigned(&id)[4]) {
#pragma unroll
    for (int u = 0; u < 4; ++u) id[u] = items[min(i0 + 4 * u + kg, last - 1)];
  };
  auto load_points = [&](const unsigned(&id)[4], MbPoints<NS> &v) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const size_t qm = ((size_t)n * a.Lq + (id[u] >> 4)) * a.M + m, lp = id[u] & 15u;
      const float2 l = *(const float2 *)(a.loc + (qm * a.LP + lp) * 2);
      v.lx[u] = l.x, v.ly[u] = l.y;
      v.aw[u] = a.aw[qm * a.LP + lp];
#pragma unroll
      for (int s = 0; s < NS; ++s) v.g[u][s] = a.gout[qm * D + s * 16 + i16];
    }
  };
  f32x4 acc[NS][6];
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int rt = 0; rt < 6; ++rt) acc[s][rt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  int prow[6], pcol[6];                                        // footprint row / column of this lane's pixel in row tile rt
#pragma unroll
  for (int rt = 0; rt < 6; ++rt) prow[rt] = (rt * 16 + i16) / (MB_T + 1), pcol[rt] = (rt * 16 + i16) % (MB_T + 1);
  unsigned id[4];
  MbPoints<NS> cur, nxt;
  load_ids(first, id);
  load_points(id, cur);
  load_ids(first + 16, id);
  for (unsigned i0 = first; i0 < last; i0 += 16) {
    load_points(id, nxt);
    load_ids(i0 + 32, id);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      int hl, wl;
      float lh, lw;
      mb_point_hw(H, W, cur.lx[u], cur.ly[u], hl, wl, lh, lw);  // (in bounds: it was binned)
      const float scale = i0 + 4 * u + kg < last ? cur.aw[u] : 0.f;
      const int ry = hl - y0, rx = wl - x0, ry1 = ry + 1, rx1 = rx + 1;      // footprint row / column of the top-left corner
      const float wt = hl >= 0 ? 1.f - lh : 0.f, wb = hl + 1 <= H - 1 ? lh : 0.f;
      const float wl_ = wl >= 0 ? 1.f - lw : 0.f, wr = wl + 1 <= W - 1 ? lw : 0.f;
#pragma unroll
      for (int rt = 0; rt < 6; ++rt) {
        float wy = prow[rt] == ry ? wt : 0.f, wx = pcol[rt] == rx ? wl_ : 0.f;
        wy = prow[rt] == ry1 ? wb : wy;
        wx = pcol[rt] == rx1 ? wr : wx;
        const float wgt = wy * wx;                             // the A operand: once per point and row tile, NS products
#pragma unroll
        for (int s = 0; s < NS; ++s)
          acc[s][rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wgt, cur.g[u][s] * scale, acc[s][rt], 0, 0, 0);
      }
    }
    cur = nxt;
  }
  float *slab = a.slabs + ((size_t)n * a.mw + wid) * MB_FOOT * D;
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int rt = 0; rt < 6; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int px = rt * 16 + 4 * kg + r;
        if (px < MB_FOOT) slab[px * D + s * 16 + i16] = acc[s][rt][r];
      }
}

// grad_value of one (map, level, tile): every pixel of the tile's 8 x 8 interior = the sum of that pixel over the tile's own
// work items + the halo row / column / corner of the tiles above, to the left and above-left, head by head.  A pure gather:
// M * D channels per pixel, the level's pixels start at a.start[level].
template <bool ONE_LEVEL>
__global__ __launch_bounds__(256) void msda_bin_reduce_kernel(MsdaMlArgs a) {
  const int n = blockIdx.y, tg = blockIdx.x, lv = mb_level_of_tile<ONE_LEVEL>(a, tg), t = tg - a.tbase[lv];
  const int H = a.H[lv], W = a.W[lv], tx = a.tx[lv];
  const int tyi = t / tx, txi = t - tyi * tx, y0 = tyi * MB_T, x0 = txi * MB_T;
  const int D = a.D, C = a.M * D, C4 = C / 4;
  const unsigned *binw = a.binw + (size_t)n * (a.nbm + 1);
  const float *slabs = a.slabs + (size_t)n * a.mw * MB_FOOT * D;
  for (int i = threadIdx.x; i < MB_T * MB_T * C4; i += 256) {
    const int px = i / C4, c = (i - px * C4) * 4, ly = px / MB_T, lx = px - ly * MB_T, m = c / D, cc = c - m * D;
    if (y0 + ly >= H || x0 + lx >= W) continue;
    f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
    auto add = [&](int b, int fy, int fx) {
      const unsigned w0 = binw[b], w1 = binw[b + 1];
      for (unsigned w = w0; w < w1; ++w)
        acc += *(const f32x4 *)(slabs + ((size_t)w * MB_FOOT + fy * (MB_T + 1) + fx) * D + cc);
    };
    add(tg * a.M + m, ly, lx);
    if (ly == 0 && tyi > 0) add((tg - tx) * a.M + m, MB_T, lx);
    if (lx == 0 && txi > 0) add((tg - 1) * a.M + m, ly, MB_T);
    if (ly == 0 && lx == 0 && tyi > 0 && txi > 0) add((tg - tx - 1) * a.M + m, MB_T, MB_T);
    *(f32x4 *)(a.gvalue + ((size_t)n * a.S + (size_t)a.start[lv] + (size_t)(y0 + ly) * W + x0 + lx) * C + c) = acc;
  }
}

// any D: one thread per channel, global atomics for all three gradients (the reference's fallback,
// ms_deform_im2col_cuda.cuh:818-921)
__global__ __launch_bounds__(256) void msda_bwd_scalar_kernel(MsdaBwdArgs a) {
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long total = (long long)a.N * a.Lq * a.M * a.D;
  if (gid >= total) return;
  const int c = (int)(gid % a.D);
  const long long qm = gid / a.D;
  const int m = (int)(qm % a.M);
  const int b = (int)(qm / ((long long)a.M * a.Lq));
  const int LP = a.L * a.P;
  const int qstride = a.M * a.D;
  const float g = a.gout[gid];
  for (int lp = 0; lp < LP; ++lp) {
    const int l = lp / a.P;
    const int H = (int)a.shapes[l * 2], W = (int)a.shapes[l * 2 + 1];
    const float lx = a.loc[((size_t)qm * LP + lp) * 2], ly = a.loc[((size_t)qm * LP + lp) * 2 + 1];
    const float w = a.aw[(size_t)qm * LP + lp];
    const float h_im = ly * (float)H - 0.5f, w_im = lx * (float)W - 0.5f;
    if (!(h_im > -1.f && w_im > -1.f && h_im < (float)H && w_im < (float)W)) continue;
    const int h_low = (int)floorf(h_im), w_low = (int)floorf(w_im), h_high = h_low + 1, w_high = w_low + 1;
    const float lh = h_im - (float)h_low, lw = w_im - (float)w_low, hh = 1.f - lh, hw = 1.f - lw;
    const size_t off = ((size_t)b * a.S + (size_t)a.lstart[l]) * qstride + m * a.D + c, hs = (size_t)W * qstride;
    float v1 = 0.f, v2 = 0.f, v3 = 0.f, v4 = 0.f;
    const float tg = g * w;
    if (h_low >= 0 && w_low >= 0) {
      v1 = a.value[off + h_low * hs + (size_t)w_low * qstride];
      unsafeAtomicAdd(a.gvalue + off + h_low * hs + (size_t)w_low * qstride, tg * hh * hw);
    }
    if (h_low >= 0 && w_high <= W - 1) {
      v2 = a.value[off + h_low * hs + (size_t)w_high * qstride];
      unsafeAtomicAdd(a.gvalue + off + h_low * hs + (size_t)w_high * qstride, tg * hh * lw);
    }
    if (h_high <= H - 1 && w_low >= 0) {
      v3 = a.value[off + h_high * hs + (size_t)w_low * qstride];
      unsafeAtomicAdd(a.gvalue + off + h_high * hs + (size_t)w_low * qstride, tg * lh * hw);
    }
    if (h_high <= H - 1 && w_high <= W - 1) {
      v4 = a.value[off + h_high * hs + (size_t)w_high * qstride];
      unsafeAtomicAdd(a.gvalue + off + h_high * hs + (size_t)w_high * qstride, tg * lh * lw);
    }
    unsafeAtomicAdd(a.gaw + (size_t)qm * LP + lp, g * (hh * hw * v1 + hh * lw * v2 + lh * hw * v3 + lh * lw * v4));
    unsafeAtomicAdd(a.gloc + ((size_t)qm * LP + lp) * 2, (float)W * tg * (hh * (v2 - v1) + lh * (v4 - v3)));
    unsafeAtomicAdd(a.gloc + ((size_t)qm * LP + lp) * 2 + 1, (float)H * tg * (hw * (v3 - v1) + lw * (v4 - v2)));
  }
}

}  // namespace df3d

using namespace df3d;

extern "C" int df3d_ms_deform_attn_forward(const float *value, const int64_t *spatial_shapes,
                                           const int64_t *level_start_index, const float *sampling_loc,
                                           const float *attn_weight, int N, int S, int M, int D, int Lq, int L, int P,
                                           float *out, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  DF3D_CHECK_ARG(value && spatial_shapes && level_start_index && sampling_loc && attn_weight && out,
                 "ms_deform_attn_forward: null argument");
  DF3D_CHECK_ARG(N >= 0 && S > 0 && M > 0 && D > 0 && Lq >= 0 && L > 0 && P > 0, "ms_deform_attn_forward: bad sizes");
  if (N == 0 || Lq == 0) return DF3D_OK;
  MsdaArgs a = {value, spatial_shapes, level_start_index, sampling_loc, attn_weight, out, N, S, M, D, Lq, L, P};
  int lpg = (D % 4 == 0) ? D / 4 : 0;
  long long total;
  switch (lpg) {
#define DF3D_MSDA_CASE(G)                                                                                     \
  case G:                                                                                                     \
    total = (long long)N * Lq * M * G;                                                                        \
    hipLaunchKernelGGL(msda_vec4_kernel<G>, dim3(cdiv(total, 256)), dim3(256), 0, stream, a);                 \
    break;
    DF3D_MSDA_CASE(1)
    DF3D_MSDA_CASE(2)
    DF3D_MSDA_CASE(4)
    DF3D_MSDA_CASE(8)
    DF3D_MSDA_CASE(16)
#undef DF3D_MSDA_CASE
    default:
      total = (long long)N * Lq * M * D;
      hipLaunchKernelGGL(msda_scalar_kernel, dim3(cdiv(total, 256)), dim3(256), 0, stream, a);
  }
  DF3D_LAUNCH_CHECK();
  return DF3D_OK;
}

extern "C" int df3d_ms_deform_attn_backward(const float *value, const int64_t *spatial_shapes,
                                            const int64_t *level_start_index, const float *sampling_loc,
                                            const float *attn_weight, const float *grad_output, int N, int S, int M, int D,
                                            int Lq, int L, int P, float *grad_value, float *grad_sampling_loc,
                                            float *grad_attn_weight, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  DF3D_CHECK_ARG(N >= 0 && S > 0 && M > 0 && D > 0 && Lq >= 0 && L > 0 && P > 0, "ms_deform_attn_backward: bad sizes");
  if (N == 0) return DF3D_OK;
  DF3D_CHECK_ARG(value && spatial_shapes && level_start_index && grad_value, "ms_deform_attn_backward: null argument");
  DF3D_HIP(hipMemsetAsync(grad_value, 0, (size_t)N * S * M * D * sizeof(float), stream));
  if (Lq == 0) return DF3D_OK;
  DF3D_CHECK_ARG(sampling_loc && attn_weight && grad_output && grad_sampling_loc && grad_attn_weight,
                 "ms_deform_attn_backward: null argument");
  MsdaBwdArgs a = {value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_output,
                   grad_value, grad_sampling_loc, grad_attn_weight, N, S, M, D, Lq, L, P, nullptr};
  const int lpg = (D % 4 == 0) ? D / 4 : 0;
  long long total;
  switch (lpg) {
#define DF3D_MSDA_BWD_CASE(G)                                                                                 \
  case G:                                                                                                     \
    total = (long long)N * Lq * M * G;                                                                        \
    hipLaunchKernelGGL(msda_bwd_vec4_kernel<G>, dim3(cdiv(total, 256)), dim3(256), 0, stream, a);             \
    break;
    DF3D_MSDA_BWD_CASE(1)
    DF3D_MSDA_BWD_CASE(2)
    DF3D_MSDA_BWD_CASE(4)
    DF3D_MSDA_BWD_CASE(8)
    DF3D_MSDA_BWD_CASE(16)
#undef DF3D_MSDA_BWD_CASE
    default: {
      const size_t nlp = (size_t)N * Lq * M * L * P;
      DF3D_HIP(hipMemsetAsync(grad_sampling_loc, 0, nlp * 2 * sizeof(float), stream));
      DF3D_HIP(hipMemsetAsync(grad_attn_weight, 0, nlp * sizeof(float), stream));
      total = (long long)N * Lq * M * D;
      hipLaunchKernelGGL(msda_bwd_scalar_kernel, dim3(cdiv(total, 256)), dim3(256), 0, stream, a);
    }
  }
  DF3D_LAUNCH_CHECK();
  return DF3D_OK;
}
// ---- binned backward, any number of levels / heads of 16, 32, 64 channels / ordered: see msda_bin_* above ---------------------
// What serves a shape.  Host only (no HIP call).  mode: 0 = default, 1 = atomic, 2 = ordered ("sorted").  -> 0 atomic kernels,
// 1 binned, 2 binned + ordered, -1 ordered asked for and not served (df3d_last_error names the limit that failed).
static const char *mb_limit(int N, int S, int M, int D, int Lq, int L, int P, const int64_t *hw, const int64_t *start, bool ordered,
                            char *buf, size_t nbuf) {
#define MB_LIMIT(cond, ...)             \
  if (!(cond)) {                        \
    snprintf(buf, nbuf, __VA_ARGS__);   \
    return buf;                         \
  }
  MB_LIMIT(D == 16 || D == 32 || D == 64, "head width D = %d (served: 16, 32, 64)", D);
  MB_LIMIT(L >= 1 && P >= 1 && (long long)L * P <= 16, "L * P = %d * %d points per query and head (limit 16)", L, P);
  MB_LIMIT(N <= 65535, "N = %d maps (limit 65535)", N);
  MB_LIMIT(Lq < (1 << 28) && (long long)Lq * M * L * P < (1LL << 31), "Lq = %d queries (limits: Lq < 2^28, Lq * M * L * P < 2^31)", Lq);
  MB_LIMIT(!ordered || Lq <= (1 << 20), "Lq = %d queries (limit of the ordered pass: 2^20)", Lq);
  long long tiles = 0, pixels = 0;
  for (int l = 0; l < L; ++l) {
    const long long H = hw[l * 2], W = hw[l * 2 + 1];
    MB_LIMIT(H > 0 && W > 0 && H < (1 << 24) && W < (1 << 24), "level %d is %lld x %lld", l, H, W);
    MB_LIMIT(start[l] == pixels, "level_start_index[%d] = %lld, not the %lld pixels of the levels before it (grad_value is "
             "written once: the levels must tile S without gaps)", l, (long long)start[l], pixels);
    tiles += ((H + MB_T - 1) / MB_T) * ((W + MB_T - 1) / MB_T);
    pixels += H * W;
    MB_LIMIT(tiles * M <= 7680, "M * tiles = %d * %lld bins up to level %d (limit 7680: the LDS histogram)", M, tiles, l);
  }
  MB_LIMIT(pixels == S, "S = %d pixels per map, the levels hold %lld (grad_value is written once: no pixel outside the levels)", S,
           pixels);
#undef MB_LIMIT
  return nullptr;
}

extern "C" int df3d_ms_deform_attn_backward_plan(int N, int S, int M, int D, int Lq, int L, int P, const int64_t *level_hw,
                                                 const int64_t *level_start, int mode) {
  if (mode == 1) return 0;
  char buf[256];
  const bool sane = N >= 0 && S > 0 && M > 0 && D > 0 && Lq >= 0 && L > 0 && P > 0 && level_hw && level_start && mode >= 0 && mode <= 2;
  const char *why = sane ? mb_limit(N, S, M, D, Lq, L, P, level_hw, level_start, mode == 2, buf, sizeof buf) : "bad sizes / null argument";
  if (!why) return mode == 2 ? 2 : 1;
  if (mode != 2) return 0;
  set_error("ms_deform_attn_backward: the ordered value gradient does not serve %s", why);
  return -1;
}

// The workspace of a call, carved in this order; `bytes` is what the ..._workspace_bytes functions return.
struct MbLayout {
  size_t nbm, ppm, mw;                                         // per map: bins, point slots, work items (upper bound)
  size_t nz, count, cursor, offset, binw, nwork, work, scattered, sorted, bytes;   // byte offsets of the pieces; the total
};
static MbLayout mb_layout(int N, int M, int Lq, int L, int P, const int64_t *hw, bool ordered) {
  MbLayout w = {};
  size_t tiles = 0;
  for (int l = 0; l < L; ++l) tiles += (size_t)cdiv((int)hw[l * 2], MB_T) * cdiv((int)hw[l * 2 + 1], MB_T);
  w.nbm = tiles * M, w.ppm = (size_t)Lq * M * L * P, w.mw = w.nbm + w.ppm / MB_CHUNK + 1;
  const size_t n = (size_t)N;
  WsLayout l;
  w.nz = l.take(n * Lq * M);
  w.count = l.take(n * w.nbm * 4);
  w.cursor = l.take(n * w.nbm * 4);                            // (adjacent to `count`: one memset up to `offset` clears both)
  w.offset = l.take(n * w.nbm * 4);
  w.binw = l.take(n * (w.nbm + 1) * 4);
  w.nwork = l.take(n * 4);
  w.work = l.take(n * w.mw * 12);
  w.scattered = l.take(n * w.ppm * 4);
  if (ordered) w.sorted = l.take(n * w.ppm * 4);
  w.bytes = l.total();
  return w;
}

// The launches of a call: heads of DD channels, ONE_LEVEL = (L == 1).  One memset before them, six kernels (eight when ordered).
template <int DD, bool ONE_LEVEL>
static void mb_launch(const MsdaBwdArgs &g, const MsdaMlArgs &b, const MsdaScanArgs &sc, hipStream_t stream) {
  const long long total = (long long)b.N * b.Lq * b.M * (DD / 4);
  const dim3 bgrid(cdiv((long long)b.Lq * b.M, 256), b.N), wgrid(cdiv(b.mw, 4), b.N), sgrid(b.nbm, b.N);
  // location / weight gradients + the groups that carry a gradient (the gather half of the col2im)
  hipLaunchKernelGGL((msda_bwd_vec4_kernel<DD / 4, true>), dim3(cdiv(total, 256)), dim3(256), 0, stream, g);
  hipLaunchKernelGGL((msda_bin_kernel<false, ONE_LEVEL>), bgrid, dim3(256), b.nbm * 4, stream, b);
  hipLaunchKernelGGL(msda_bin_scan_kernel, dim3(b.N), dim3(1024), 0, stream, sc);
  hipLaunchKernelGGL((msda_bin_kernel<true, ONE_LEVEL>), bgrid, dim3(256), b.nbm * 8, stream, b);
  if (b.sorted) {
    hipLaunchKernelGGL(msda_bin_sort_kernel<false>, sgrid, dim3(256), 0, stream, b);
    hipLaunchKernelGGL(msda_bin_sort_kernel<true>, sgrid, dim3(256), 0, stream, b);
  }
  hipLaunchKernelGGL((msda_bin_accumulate_kernel<DD / 16, ONE_LEVEL>), wgrid, dim3(256), 0, stream, b);
  hipLaunchKernelGGL(msda_bin_reduce_kernel<ONE_LEVEL>, dim3(b.tbase[MB_LMAX], b.N), dim3(256), 0, stream, b);   // (a workgroup per tile)
}

// Both entries from here on (`who` names the caller in the messages); the shape has passed the caller's own checks.
static int mb_backward(const char *who, const float *value, const int64_t *spatial_shapes, const int64_t *level_start_index,
                       const float *sampling_loc, const float *attn_weight, const float *grad_output, const int64_t *level_hw,
                       const int64_t *level_start, int N, int S, int M, int D, int Lq, int L, int P, int ordered, float *grad_value,
                       float *grad_sampling_loc, float *grad_attn_weight, void *workspace, size_t workspace_bytes, float *slabs,
                       hipStream_t stream) {
  if (N == 0) return DF3D_OK;
  DF3D_CHECK_ARG(value && spatial_shapes && level_start_index && grad_value, "%s: null argument", who);
  if (Lq == 0) {
    DF3D_HIP(hipMemsetAsync(grad_value, 0, (size_t)N * S * M * D * sizeof(float), stream));
    return DF3D_OK;
  }
  DF3D_CHECK_ARG(sampling_loc && attn_weight && grad_output && grad_sampling_loc && grad_attn_weight && workspace && slabs,
                 "%s: null argument", who);
  const MbLayout w = mb_layout(N, M, Lq, L, P, level_hw, ordered != 0);
  DF3D_CHECK_ARG(workspace_bytes >= w.bytes, "%s: workspace too small", who);
  char *ws = (char *)workspace;
  DF3D_HIP(hipMemsetAsync(ws + w.count, 0, w.offset - w.count, stream));
  MsdaBwdArgs g = {value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_output,
                   grad_value, grad_sampling_loc, grad_attn_weight, N, S, M, D, Lq, L, P, (unsigned char *)(ws + w.nz)};
  MsdaMlArgs b = {};
  b.loc = sampling_loc, b.aw = attn_weight, b.gout = grad_output, b.nz = g.nz, b.gvalue = grad_value;
  b.N = N, b.S = S, b.M = M, b.D = D, b.Lq = Lq, b.L = L, b.P = P, b.LP = L * P, b.nbm = (int)w.nbm, b.mw = (int)w.mw;
  int tiles = 0;
  for (int l = 0; l < L; ++l) {
    b.H[l] = (int)level_hw[l * 2], b.W[l] = (int)level_hw[l * 2 + 1], b.tx[l] = cdiv(b.W[l], MB_T), b.start[l] = (int)level_start[l];
    b.tbase[l] = tiles;
    tiles += b.tx[l] * cdiv(b.H[l], MB_T);
  }
  for (int l = L; l <= MB_LMAX; ++l) b.tbase[l] = tiles;
  b.count = (unsigned *)(ws + w.count), b.cursor = (unsigned *)(ws + w.cursor), b.offset = (unsigned *)(ws + w.offset);
  b.binw = (unsigned *)(ws + w.binw), b.nwork = (unsigned *)(ws + w.nwork), b.work = (unsigned *)(ws + w.work);
  b.scattered = (unsigned *)(ws + w.scattered), b.sorted = ordered ? (unsigned *)(ws + w.sorted) : nullptr;
  b.items = ordered ? b.sorted : b.scattered, b.slabs = slabs;
  const MsdaScanArgs sc = {b.count, b.offset, b.binw, b.nwork, b.work, b.nbm, b.mw};
  switch (D) {
#define DF3D_MSDA_BIN_CASE(DD)                                                                 \
  case DD:                                                                                     \
    L == 1 ? mb_launch<DD, true>(g, b, sc, stream) : mb_launch<DD, false>(g, b, sc, stream);   \
    break;
    DF3D_MSDA_BIN_CASE(16)
    DF3D_MSDA_BIN_CASE(32)
    DF3D_MSDA_BIN_CASE(64)
#undef DF3D_MSDA_BIN_CASE
  }
  DF3D_LAUNCH_CHECK();
  return DF3D_OK;
}

extern "C" size_t df3d_ms_deform_attn_backward_binned_ml_workspace_bytes(int N, int M, int Lq, int L, int P, const int64_t *level_hw,
                                                                         int ordered) {
  if (!level_hw || N < 0 || M <= 0 || Lq < 0 || L <= 0 || P <= 0) return 0;
  return mb_layout(N, M, Lq, L, P, level_hw, ordered != 0).bytes;
}
/* + the work items' footprints: N * mw * 81 * D floats, mw = tiles * M + Lq * M * L * P / 512 + 1 work items per map */
extern "C" size_t df3d_ms_deform_attn_backward_binned_ml_slab_bytes(int N, int M, int D, int Lq, int L, int P, const int64_t *level_hw) {
  if (!level_hw || N < 0 || M <= 0 || D <= 0 || Lq < 0 || L <= 0 || P <= 0) return 0;
  return (size_t)N * mb_layout(N, M, Lq, L, P, level_hw, false).mw * MB_FOOT * D * 4;
}

extern "C" int df3d_ms_deform_attn_backward_binned_ml(const float *value, const int64_t *spatial_shapes, const int64_t *level_start_index,
                                                      const float *sampling_loc, const float *attn_weight, const float *grad_output,
                                                      const int64_t *level_hw, const int64_t *level_start, int N, int M, int D, int Lq,
                                                      int L, int P, int ordered, float *grad_value, float *grad_sampling_loc,
                                                      float *grad_attn_weight, void *workspace, size_t workspace_bytes, float *slabs,
                                                      void *stream) {
  DF3D_CHECK_ARG(N >= 0 && M > 0 && D > 0 && Lq >= 0 && L > 0 && P > 0 && level_hw && level_start,
                 "ms_deform_attn_backward_binned_ml: bad sizes / null level arrays");
  long long S = 0;
  for (int l = 0; l < L && l < MB_LMAX; ++l) S += level_hw[l * 2] * level_hw[l * 2 + 1];
  char buf[256];
  const char *why = S > 0 && S < (1LL << 31) ? mb_limit(N, (int)S, M, D, Lq, L, P, level_hw, level_start, ordered != 0, buf, sizeof buf)
                                              : "bad level sizes";
  DF3D_CHECK_ARG(!why, "ms_deform_attn_backward_binned_ml: not served: %s", why);
  return mb_backward("ms_deform_attn_backward_binned_ml", value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_output,
                     level_hw, level_start, N, (int)S, M, D, Lq, L, P, ordered, grad_value, grad_sampling_loc, grad_attn_weight, workspace,
                     workspace_bytes, slabs, (hipStream_t)stream);
}

// ---- the single-level entry (one map [N, H * W, M, 16]; round 6): its own argument checks, then the above with L = 1 ----------
extern "C" size_t df3d_ms_deform_attn_backward_binned_workspace_bytes(int N, int M, int Lq, int LP, int H, int W) {
  const int64_t level_hw[2] = {H, W};
  return mb_layout(N, M, Lq, 1, LP, level_hw, false).bytes;
}
extern "C" size_t df3d_ms_deform_attn_backward_binned_slab_bytes(int N, int M, int D, int Lq, int LP, int H, int W) {
  (void)D;
  const int64_t level_hw[2] = {H, W};
  return (size_t)N * mb_layout(N, M, Lq, 1, LP, level_hw, false).mw * MB_FOOT * MB_D * 4;
}

extern "C" int df3d_ms_deform_attn_backward_binned(const float *value, const int64_t *spatial_shapes, const int64_t *level_start_index,
                                                   const float *sampling_loc, const float *attn_weight, const float *grad_output,
                                                   int N, int M, int D, int Lq, int P, int H, int W, float *grad_value,
                                                   float *grad_sampling_loc, float *grad_attn_weight, void *workspace,
                                                   size_t workspace_bytes, float *slabs, void *stream) {
  DF3D_CHECK_ARG(N >= 0 && M > 0 && D > 0 && Lq >= 0 && P > 0 && H > 0 && W > 0, "ms_deform_attn_backward_binned: bad sizes");
  DF3D_CHECK_ARG(D == MB_D && P <= 16 && Lq < (1 << 28), "ms_deform_attn_backward_binned: head width %d / %d points not served", D, P);
  const int tiles = cdiv(W, MB_T) * cdiv(H, MB_T);
  DF3D_CHECK_ARG((size_t)tiles * M <= 7680, "ms_deform_attn_backward_binned: %d tiles x %d heads exceed the LDS budget", tiles, M);
  DF3D_CHECK_ARG(N <= 65535 && (long long)Lq * M * P < (1LL << 31), "ms_deform_attn_backward_binned: %d maps x %d queries", N, Lq);
  const int64_t level_hw[2] = {H, W}, level_start[1] = {0};
  return mb_backward("ms_deform_attn_backward_binned", value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_output,
                     level_hw, level_start, N, H * W, M, D, Lq, 1, P, 0, grad_value, grad_sampling_loc, grad_attn_weight, workspace,
                     workspace_bytes, slabs, (hipStream_t)stream);
}
