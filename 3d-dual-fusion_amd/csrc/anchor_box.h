// The anchor table and the residual box coder of the Voxel-RCNN units: proposals.hip, anchorloss.hip,
// roiloss.hip.  Anchors are never materialised: an anchor is (x shift of its set at column x, y shift of its set at row y,
// its row of the per-anchor table).  The coder is VR/pcdet/utils/box_coder_utils.py (ResidualCoder) evaluated operation by
// operation in the scalar type T (float: the reference's arithmetic; double: the loss values): the includer sets
// `#pragma clang fp contract(off)` in front of the include, as for bev_overlap.h (a pragma here would run on into the includer).
#pragma once
#include "common.h"

namespace df3d {

// An anchor's index within a frame is pix * A + an.  The proposal keys pack it into this many bits ([frame 8 | 0 0 |
// ~ordered(logit) 32 | index 22]: topk.hip orders the low 54 bits of a segment), so every entry refuses more anchors.
constexpr int ANCHOR_INDEX_BITS = 22;

struct AnchorTab {
  const float *x_shifts, *y_shifts;      // [S][W], [S][H]
  int batch, H, W, A, S;
  int set[DF3D_MAX_ANCHORS];
  float anchor[DF3D_MAX_ANCHORS][5];     // centre z, dx, dy, dz, rotation
};

// the limits of every entry that takes the table; `what` names the entry point
static inline int anchor_check(const df3d_anchor_cfg *c, const char *what) {
  DF3D_CHECK_ARG(c->batch > 0 && c->H > 0 && c->W > 0, "%s: bad map size", what);
  DF3D_CHECK_ARG(c->batch <= 255, "%s: at most 255 frames (got %d)", what, c->batch);
  DF3D_CHECK_ARG(c->num_anchors > 0 && c->num_anchors <= DF3D_MAX_ANCHORS, "%s: 1..%d anchors per location (DF3D_MAX_ANCHORS)",
                 what, DF3D_MAX_ANCHORS);
  DF3D_CHECK_ARG(c->num_sets > 0 && c->num_sets <= DF3D_MAX_ANCHORS, "%s: 1..%d anchor sets", what, DF3D_MAX_ANCHORS);
  DF3D_CHECK_ARG((long long)c->H * c->W * c->num_anchors <= (1ll << ANCHOR_INDEX_BITS), "%s: at most 2^%d anchors per frame (H*W*A)",
                 what, ANCHOR_INDEX_BITS);
  for (int a = 0; a < c->num_anchors; ++a)
    DF3D_CHECK_ARG(c->anchor_set[a] >= 0 && c->anchor_set[a] < c->num_sets, "%s: anchor %d names set %d of %d", what, a,
                   c->anchor_set[a], c->num_sets);
  return DF3D_OK;
}

static inline void anchor_fill(AnchorTab &t, const df3d_anchor_cfg *c, const float *x_shifts, const float *y_shifts) {
  t.x_shifts = x_shifts, t.y_shifts = y_shifts;
  t.batch = c->batch, t.H = c->H, t.W = c->W, t.A = c->num_anchors, t.S = c->num_sets;
  for (int i = 0; i < c->num_anchors; ++i) {
    t.set[i] = c->anchor_set[i];
    for (int e = 0; e < 5; ++e) t.anchor[i][e] = c->anchor[i][e];
  }
}

// anchor index within a frame -> pixel and anchor of the pixel
__device__ __forceinline__ void anchor_split(const AnchorTab &t, int idx, int &pix, int &an) {
  pix = idx / t.A, an = idx - pix * t.A;
}

// anchor `an` of pixel `pix` (inside the map): its centre (xa, ya); returns its table row
__device__ __forceinline__ const float *anchor_at(const AnchorTab &t, int pix, int an, float &xa, float &ya) {
  const int y = pix / t.W, x = pix - y * t.W, s = t.set[an];
  xa = t.x_shifts[s * t.W + x], ya = t.y_shifts[s * t.H + y];
  return t.anchor[an];
}

// ---- ResidualCoder (sqrt / log / exp / fmax of a float are HIP's overloads onto sqrtf / logf / expf / fmaxf) -----------------
// encode_torch (:13-43) of box g (x, y, z, dx, dy, dz, heading) against one anchor; every size is clamped at 1e-5.  The RoI
// users pass zeros for the centre and the rotation (v - 0 is v, the sign of a zero included).
template <class T>
__device__ __forceinline__ void residual_encode(const float *g, T xa, T ya, T za, T dxa, T dya, T dza, T ra, T *t) {
  dxa = fmax(dxa, T(1e-5)), dya = fmax(dya, T(1e-5)), dza = fmax(dza, T(1e-5));
  const T dxg = fmax((T)g[3], T(1e-5)), dyg = fmax((T)g[4], T(1e-5)), dzg = fmax((T)g[5], T(1e-5));
  const T diag = sqrt(dxa * dxa + dya * dya);
  t[0] = ((T)g[0] - xa) / diag, t[1] = ((T)g[1] - ya) / diag, t[2] = ((T)g[2] - za) / dza;
  t[3] = log(dxg / dxa), t[4] = log(dyg / dya), t[5] = log(dzg / dza);
  t[6] = (T)g[6] - ra;
}

// decode_torch (:45-77) without the anchor's centre and rotation: offsets g[0..2] and sizes g[3..5], nothing clamped; returns
// the anchor's BEV diagonal.  For a caller that goes on in the anchor's own frame (adding a zero centre would turn a -0 offset
// into +0).
template <class T>
__device__ __forceinline__ T residual_decode_local(const float *t, T dxa, T dya, T dza, T *g) {
  const T diag = sqrt(dxa * dxa + dya * dya);
  g[0] = (T)t[0] * diag, g[1] = (T)t[1] * diag, g[2] = (T)t[2] * dza;
  g[3] = exp((T)t[3]) * dxa, g[4] = exp((T)t[4]) * dya, g[5] = exp((T)t[5]) * dza;
  return diag;
}

// decode_torch of residuals t against one anchor
template <class T>
__device__ __forceinline__ void residual_decode(const float *t, T xa, T ya, T za, T dxa, T dya, T dza, T ra, T *g) {
  residual_decode_local(t, dxa, dya, dza, g);
  g[0] = g[0] + xa, g[1] = g[1] + ya, g[2] = g[2] + za;
  g[6] = (T)t[6] + ra;
}

}  // namespace df3d
