// Voxel-RCNN second-stage training: the proposal targets and the RCNN losses on the device.
//
// Reference: VR/pcdet/models/roi_heads/target_assigner/proposal_target_layer.py loops over frames in Python: a per-class loop
// of boxes_iou3d_gpu calls, three nonzero() compactions, a host np.random.permutation and two torch.randint draws sized by
// counts read back to the host; roi_head_template.py:104-231 then transforms the sampled ground truth and builds the three
// losses with fg_sum.item(), a boolean-mask gather, a decode, a rotation and two boxes_to_corners_3d.
//
// df3d_roi_targets -- ONE launch, one workgroup per frame, nothing read back:
//   valid GT count and the frame's GT rows into LDS -> per RoI the best overlap and its row (3-D IoU in double on the
//   clipping of bev_overlap.h, rounded once to float32) -> the three lists in ascending RoI index (per-thread runs of
//   consecutive RoIs + a prefix over the 256 run counts) -> the sampled RoI of every slot as a function of the caller's
//   draws (stable rank of the fg keys, floor(u * n) into the lists) -> gather, masks, labels and the canonical transform.
// df3d_rcnn_loss / df3d_rcnn_loss_grad -- the three losses fused: one thread per sampled RoI, fp64 partials per workgroup at
//   fixed positions and an ordered final sum that also leaves the two normalisers (valid, fg_sum) on the device; the
//   gradient kernel reads them and the upstream gradients from device memory and writes every element of both gradients.
#include <cstring>

#include "common.h"

#pragma clang fp contract(off)         // before the shared device code: the three headers rely on it
#include "anchor_box.h"
#include "bev_overlap.h"
#include "loss_terms.h"

namespace df3d {

constexpr int MAX_ROIS = DF3D_ROI_MAX_ROIS, MAX_SAMPLES = DF3D_ROI_MAX_SAMPLES, MAX_GT = DF3D_ROI_MAX_GT;
constexpr double PI_D = 3.14159265358979323846, TWO_PI_D = 2.0 * 3.14159265358979323846;

// pcdet's LiDAR box (x, y, z, dx, dy, dz, heading) for the clipping, in double (iou3d_nms_kernel.cu:50-62, 115-160)
struct LidarBoxD {
  typedef BevPtT<double> Pt;
  static __device__ __forceinline__ bool contains(const float *box, Pt p) {
    const double margin = 1e-8;          // the float kernel's 1e-2 guards float32 rounding and moves the area; not needed here
    const double cx = box[0], cy = box[1];
    const double c = cos(-(double)box[6]), s = sin(-(double)box[6]);
    const double rx = (p.x - cx) * c + (p.y - cy) * (-s);
    const double ry = (p.x - cx) * s + (p.y - cy) * c;
    return fabs(rx) < (double)box[3] / 2 + margin && fabs(ry) < (double)box[4] / 2 + margin;
  }
  static __device__ __forceinline__ void corners(const float *box, Pt *c) {
    const double cx = box[0], cy = box[1], hx = (double)box[3] / 2, hy = (double)box[4] / 2;
    const double co = cos((double)box[6]), si = sin((double)box[6]);
    const double px[4] = {-hx, hx, hx, -hx}, py[4] = {-hy, -hy, hy, hy};
    for (int k = 0; k < 4; ++k) {
      c[k].x = px[k] * co + py[k] * (-si) + cx;
      c[k].y = px[k] * si + py[k] * co + cy;
    }
    c[4] = c[0];
  }
};

// boxes_iou3d_gpu (iou3d_nms_utils.py:48-80) of one pair
__device__ double iou3d_lidar(const float *a, const float *b) {
  const double a_max = (double)a[2] + (double)a[5] / 2, a_min = (double)a[2] - (double)a[5] / 2;
  const double b_max = (double)b[2] + (double)b[5] / 2, b_min = (double)b[2] - (double)b[5] / 2;
  const double h = fmax(fmin(a_max, b_max) - fmax(a_min, b_min), 0.0);
  const double va = (double)a[3] * (double)a[4] * (double)a[5], vb = (double)b[3] * (double)b[4] * (double)b[5];
  double bev = 0.0;
  if (h > 0.0) {
    // footprints whose circumscribed circles do not meet share no area
    const double ex = (double)a[0] - (double)b[0], ey = (double)a[1] - (double)b[1];
    const double ra = 0.5 * sqrt((double)a[3] * a[3] + (double)a[4] * a[4]), rb = 0.5 * sqrt((double)b[3] * b[3] + (double)b[4] * b[4]);
    const double reach = (ra + rb) * (1.0 + 1e-9) + 1e-9;
    if (ex * ex + ey * ey <= reach * reach) bev = bev_overlap<LidarBoxD, double>(a, b);
  }
  const double o3 = bev * h;
  return o3 / fmax(va + vb - o3, 1e-6);
}

// Python's float modulo (the sign of the divisor)
__device__ __forceinline__ double py_mod(double a, double m) {
  double r = fmod(a, m);
  if (r != 0.0 && ((r < 0.0) != (m < 0.0))) r += m;
  return r;
}

struct TargetArgs {
  const float *rois, *scores;
  const long long *labels;
  const float *gt, *u_fg, *u_slot;
  df3d_roi_target_cfg c;
  float *o_rois;
  long long *o_labels;
  float *o_scores, *o_ious;
  int32_t *o_inds;
  float *o_src, *o_gt;
  int32_t *o_mask;
  float *o_cls;
  int32_t *counts;
  float *w_iou;                          // workspace [B][R] each
  int32_t *w_asg, *w_fg, *w_bg;
};

// grid (batch), 256 threads
__global__ __launch_bounds__(256) void roi_targets_kernel(TargetArgs a) {
  __shared__ float s_gt[MAX_GT * 8];
  __shared__ float s_key[MAX_ROIS];
  __shared__ int s_cnt[3][256];
  __shared__ int s_last;
  const df3d_roi_target_cfg &c = a.c;
  const int b = blockIdx.x, tid = threadIdx.x, R = c.num_rois, G = c.max_gt, M = c.roi_per_image;
  const float *gt = a.gt + (size_t)b * G * 8;
  const float *rois = a.rois + (size_t)b * R * 7;
  const long long *labels = a.labels + (size_t)b * R;
  float *w_iou = a.w_iou + (size_t)b * R;
  int32_t *w_asg = a.w_asg + (size_t)b * R, *w_fg = a.w_fg + (size_t)b * R, *w_bg = a.w_bg + (size_t)b * R;
  int32_t *o_inds = a.o_inds + (size_t)b * M;

  // ---- valid ground truth: `while k > 0 and cur_gt[k].sum() == 0: k -= 1`
  if (tid == 0) s_last = 0;
  __syncthreads();
  int last = 0;
  for (int g = tid; g < G; g += 256) {
    const float *r = gt + (size_t)g * 8;
    float sum = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      s_gt[g * 8 + e] = r[e];
      sum += r[e];
    }
    if (sum != 0.f) last = g;                                       // (NaN counts as non-zero, as in the reference)
  }
  atomicMax(&s_last, last);
  __syncthreads();
  const int valid = s_last + 1;

  // ---- per RoI: the best overlap and its ground-truth row
  for (int i = tid; i < R; i += 256) {
    const float *r = rois + (size_t)i * 7;
    const long long lab = labels[i];
    float best = -1.f;
    int arg = -1;
    for (int g = 0; g < valid; ++g) {
      if (c.sample_by_class && (long long)s_gt[g * 8 + 7] != lab) continue;
      const float iou = (float)iou3d_lidar(r, s_gt + g * 8);
      if (iou > best) {                                             // first maximum wins
        best = iou;
        arg = g;
      }
    }
    if (arg < 0) best = 0.f, arg = 0;                               // no ground truth of the RoI's class: overlap 0, row 0
    w_iou[i] = best;
    w_asg[i] = arg;
  }
  __syncthreads();

  // ---- the three lists in ascending RoI index: thread t owns RoIs [t * run, (t + 1) * run)
  const float fg_thresh = (float)fmin(c.reg_fg_thresh, c.cls_fg_thresh);
  const float reg_fg = (float)c.reg_fg_thresh, bg_lo = (float)c.cls_bg_thresh_lo;
  const int run = (R + 255) / 256;
  const int i0 = min(tid * run, R), i1 = min(i0 + run, R);
  int n[3] = {0, 0, 0};
  for (int i = i0; i < i1; ++i) {
    const float v = w_iou[i];
    n[0] += v >= fg_thresh ? 1 : 0;
    n[1] += (v < reg_fg && v >= bg_lo) ? 1 : 0;
    n[2] += v < bg_lo ? 1 : 0;
  }
  for (int k = 0; k < 3; ++k) s_cnt[k][tid] = n[k];
  __syncthreads();
  int off[3] = {0, 0, 0}, tot[3] = {0, 0, 0};
  for (int t = 0; t < 256; ++t)
    for (int k = 0; k < 3; ++k) {
      const int v = s_cnt[k][t];
      off[k] += t < tid ? v : 0;
      tot[k] += v;
    }
  const int n_fg = tot[0], n_hard = tot[1], n_easy = tot[2], n_bg = n_hard + n_easy;
  for (int i = i0; i < i1; ++i) {
    const float v = w_iou[i];
    if (v >= fg_thresh) w_fg[off[0]++] = i;
    if (v < reg_fg && v >= bg_lo) w_bg[off[1]++] = i;
    if (v < bg_lo) w_bg[n_hard + off[2]++] = i;
  }
  if (tid < 3) a.counts[(size_t)b * 3 + tid] = tot[tid];
  for (int j = tid; j < n_fg; j += 256) s_key[j] = a.u_fg[(size_t)b * R + j];
  __threadfence_block();
  __syncthreads();

  // ---- the RoI of every slot
  const float *u_slot = a.u_slot + (size_t)b * M;
  int F = 0;
  if (n_fg > 0 && n_bg > 0) {
    F = min(c.fg_per_image, n_fg);
    for (int j = tid; j < n_fg; j += 256) {                         // stable rank of key j: argsort(u_fg[b, :n_fg], stable)
      const float kj = s_key[j];
      int rank = 0;
      for (int i = 0; i < n_fg; ++i) {
        const float ki = s_key[i];
        rank += (ki < kj || (ki == kj && i < j)) ? 1 : 0;
      }
      if (rank < F) o_inds[rank] = w_fg[j];
    }
  }
  if (n_bg > 0) {
    int n_from_hard;                                                // slots F .. F + n_from_hard - 1 index the hard list
    if (n_hard > 0 && n_easy > 0) n_from_hard = min((int)((double)(M - F) * c.hard_bg_ratio), n_hard);
    else n_from_hard = n_hard > 0 ? M - F : 0;
    for (int s = F + tid; s < M; s += 256) {
      const bool hard = s < F + n_from_hard;
      const int cnt = hard ? n_hard : n_easy;
      int e = (int)floor((double)u_slot[s] * (double)cnt);
      e = min(max(e, 0), cnt - 1);
      o_inds[s] = w_bg[(hard ? 0 : n_hard) + e];
    }
  } else if (n_fg > 0) {
    for (int s = tid; s < M; s += 256) {
      int e = (int)floor((double)u_slot[s] * (double)n_fg);
      e = min(max(e, 0), n_fg - 1);
      o_inds[s] = w_fg[e];
    }
  } else {
    for (int s = tid; s < M; s += 256) o_inds[s] = 0;               // NaN overlaps only (the reference raises)
  }
  __threadfence_block();
  __syncthreads();

  // ---- gather, masks, labels, canonical transform
  const float cls_fg = (float)c.cls_fg_thresh, cls_bg = (float)c.cls_bg_thresh;
  for (int s = tid; s < M; s += 256) {
    const int i = min(max(o_inds[s], 0), R - 1);                    // (NaN keys leave a slot unwritten: stay inside the frame)
    o_inds[s] = i;
    const size_t o = (size_t)b * M + s;
    const float *r = rois + (size_t)i * 7;
    const float iou = w_iou[i];
    const float *g = s_gt + w_asg[i] * 8;
#pragma unroll
    for (int e = 0; e < 7; ++e) a.o_rois[o * 7 + e] = r[e];
    a.o_labels[o] = labels[i];
    a.o_scores[o] = a.scores[(size_t)b * R + i];
    a.o_ious[o] = iou;
    a.o_mask[o] = iou > reg_fg ? 1 : 0;
    float label;
    if (c.cls_score_type == DF3D_ROI_SCORE_CLS) {
      label = iou > cls_fg ? 1.f : 0.f;
      if (iou > cls_bg && iou < cls_fg) label = -1.f;
    } else {
      const bool fg = iou > cls_fg, bg = iou < cls_bg;
      label = fg ? 1.f : 0.f;
      if (!fg && !bg) label = (float)(((double)iou - c.cls_bg_thresh) / (c.cls_fg_thresh - c.cls_bg_thresh));
    }
    a.o_cls[o] = label;
#pragma unroll
    for (int e = 0; e < 8; ++e) a.o_src[o * 8 + e] = g[e];
    // roi_head_template.py:113-132
    const double roi_ry = py_mod((double)r[6], TWO_PI_D);
    const double x = (double)g[0] - (double)r[0], y = (double)g[1] - (double)r[1], z = (double)g[2] - (double)r[2];
    const double co = cos(-roi_ry), si = sin(-roi_ry);
    double heading = py_mod((double)g[6] - roi_ry, TWO_PI_D);
    if (heading > PI_D * 0.5 && heading < PI_D * 1.5) heading = py_mod(heading + PI_D, TWO_PI_D);
    if (heading > PI_D) heading -= TWO_PI_D;
    heading = fmin(fmax(heading, -PI_D / 2), PI_D / 2);
    float *t = a.o_gt + o * 8;
    t[0] = (float)(x * co - y * si);
    t[1] = (float)(x * si + y * co);
    t[2] = (float)z;
    t[3] = g[3], t[4] = g[4], t[5] = g[5];
    t[6] = (float)heading;
    t[7] = g[7];
  }
}

// ---- losses ------------------------------------------------------------------------------------------------------------
struct RcnnArgs {
  const float *cls, *reg, *rois, *gt, *src, *labels;
  const int32_t *mask;
  int ld_cls, ld_reg, N, corner;
  double cw[7], beta, weight[3];         // cls, reg, corner
};

// what one sampled RoI contributes: the values, and the derivatives with respect to its logit and its seven residuals
struct RowTerms {
  double l_cls, valid, l_reg, fg, l_corner;
  double d_cls, d_reg[7], d_corner[7];
};

__device__ void row_terms(const RcnnArgs &a, int i, RowTerms &t) {
  t.l_cls = t.valid = t.l_reg = t.fg = t.l_corner = t.d_cls = 0.0;
  for (int e = 0; e < 7; ++e) t.d_reg[e] = t.d_corner[e] = 0.0;
  const double label = (double)a.labels[i];
  if (label >= 0.0) {                                               // BCE with logits, stable form
    bce_with_logits((double)a.cls[(size_t)i * a.ld_cls], label, t.l_cls, t.d_cls);
    t.valid = 1.0;
  }
  if (a.mask[i] <= 0) return;
  t.fg = 1.0;
  const float *p = a.reg + (size_t)i * a.ld_reg;
  const float *r = a.rois + (size_t)i * 7, *g = a.gt + (size_t)i * 8, *s = a.src + (size_t)i * 8;
  {  // ResidualCoder.encode_torch against the RoI with centre and heading zeroed; smooth L1
    double tg[7];
    residual_encode<double>(g, 0.0, 0.0, 0.0, r[3], r[4], r[5], 0.0, tg);
    for (int e = 0; e < 7; ++e) {
      if (tg[e] != tg[e]) continue;                                 // NaN targets are ignored (loss_utils.py:122)
      double v, slope;
      smooth_l1(a.cw[e] * ((double)p[e] - tg[e]), a.beta, v, slope);
      t.l_reg += v;
      t.d_reg[e] = slope * a.cw[e];
    }
  }
  if (!a.corner) return;
  // decode against the RoI with zero centre, rotate by the RoI heading, add the centre (roi_head_template.py:169-184)
  const double dxa = r[3], dya = r[4], dza = r[5];
  double q[6];
  const double diag = residual_decode_local(p, dxa, dya, dza, q);  // (no zero centre added: a -0 offset stays -0)
  const double x = q[0], y = q[1], z = q[2], dx = q[3], dy = q[4], dz = q[5];
  const double rg = (double)p[6] + (double)r[6];
  const double c0 = cos((double)r[6]), s0 = sin((double)r[6]);
  const double X = x * c0 - y * s0 + (double)r[0], Y = x * s0 + y * c0 + (double)r[1], Z = z + (double)r[2];
  const double cr = cos(rg), sr = sin(rg);
  const double cg = cos((double)s[6]), sg = sin((double)s[6]);     // the flipped box: cos and sin change sign
  double gX = 0.0, gY = 0.0, gZ = 0.0, g_dx = 0.0, g_dy = 0.0, g_dz = 0.0, g_r = 0.0;
  const double sxs[8] = {1, 1, -1, -1, 1, 1, -1, -1}, sys[8] = {1, -1, -1, 1, 1, -1, -1, 1}, szs[8] = {-1, -1, -1, -1, 1, 1, 1, 1};
  for (int k = 0; k < 8; ++k) {
    const double pa = sxs[k] * dx / 2, pb = sys[k] * dy / 2, pc = szs[k] * dz / 2;
    const double px = pa * cr - pb * sr + X, py = pa * sr + pb * cr + Y, pz = pc + Z;
    const double ga = sxs[k] * (double)s[3] / 2, gb = sys[k] * (double)s[4] / 2, gc = szs[k] * (double)s[5] / 2;
    const double qx = ga * cg - gb * sg, qy = ga * sg + gb * cg;   // the GT corner about its centre; flipped: -qx, -qy
    const double ez = pz - (gc + (double)s[2]);
    const double e1x = px - (qx + (double)s[0]), e1y = py - (qy + (double)s[1]);
    const double e2x = px - (-qx + (double)s[0]), e2y = py - (-qy + (double)s[1]);
    const double d1 = sqrt(e1x * e1x + e1y * e1y + ez * ez), d2 = sqrt(e2x * e2x + e2y * e2y + ez * ez);
    const bool direct = d1 <= d2;
    const double d = direct ? d1 : d2, ex = direct ? e1x : e2x, ey = direct ? e1y : e2y;
    t.l_corner += d < 1.0 ? 0.5 * d * d : d - 0.5;
    if (d == 0.0) continue;                                         // the norm's subgradient at zero
    const double w = (d < 1.0 ? d : 1.0) / d;
    const double gpx = w * ex, gpy = w * ey, gpz = w * ez;
    gX += gpx, gY += gpy, gZ += gpz;
    g_dx += (gpx * cr + gpy * sr) * sxs[k] / 2;
    g_dy += (-gpx * sr + gpy * cr) * sys[k] / 2;
    g_dz += gpz * szs[k] / 2;
    g_r += gpx * (-pa * sr - pb * cr) + gpy * (pa * cr - pb * sr);
  }
  t.d_corner[0] = (gX * c0 + gY * s0) * diag;
  t.d_corner[1] = (-gX * s0 + gY * c0) * diag;
  t.d_corner[2] = gZ * dza;
  t.d_corner[3] = g_dx * dx;
  t.d_corner[4] = g_dy * dy;
  t.d_corner[5] = g_dz * dz;
  t.d_corner[6] = g_r;
}

// grid (ceil(N / 256)): partials[block][5] (cls, valid, reg, fg, corner)
__global__ __launch_bounds__(256) void rcnn_loss_kernel(RcnnArgs a, double *__restrict__ partials) {
  __shared__ double s_red[4];
  const int i = blockIdx.x * 256 + threadIdx.x;
  RowTerms t;
  t.l_cls = t.valid = t.l_reg = t.fg = t.l_corner = 0.0;
  if (i < a.N) row_terms(a, i, t);
  const double v[5] = {t.l_cls, t.valid, t.l_reg, t.fg, t.l_corner};
  partials_write<5>(v, partials, s_red);
}

// one workgroup: the partials in a fixed order -> the three scalars and the two normalisers
__global__ __launch_bounds__(256) void rcnn_loss_final_kernel(const double *__restrict__ partials, int nblocks, double w_cls,
                                                              double w_reg, double w_corner, float *__restrict__ losses,
                                                              double *__restrict__ norms) {
  __shared__ double s_red[4];
  double tot[5];
  partials_sum<5>(partials, nblocks, tot, s_red);
  if (threadIdx.x == 0) {
    const double valid = tot[1], fg = tot[3];
    losses[0] = (float)(tot[0] / fmax(valid, 1.0) * w_cls);
    losses[1] = (float)(tot[2] / fmax(fg, 1.0) * w_reg);
    losses[2] = (float)(fg > 0.0 ? tot[4] / (8.0 * fg) * w_corner : 0.0);
    norms[0] = valid;
    norms[1] = fg;
  }
}

// grid (ceil(N / 256)): every element of both gradients
__global__ __launch_bounds__(256) void rcnn_loss_grad_kernel(RcnnArgs a, const double *__restrict__ norms,
                                                             const float *__restrict__ upstream, float *__restrict__ g_cls,
                                                             int ld_gcls, float *__restrict__ g_reg, int ld_greg) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.N) return;
  RowTerms t;
  row_terms(a, i, t);
  const double valid = norms[0], fg = norms[1];
  const double k_cls = (double)upstream[0] * a.weight[0] / fmax(valid, 1.0);
  const double k_reg = (double)upstream[1] * a.weight[1] / fmax(fg, 1.0);
  const double k_corner = fg > 0.0 ? (double)upstream[2] * a.weight[2] / (8.0 * fg) : 0.0;
  g_cls[(size_t)i * ld_gcls] = (float)(t.d_cls * k_cls);
  for (int e = 0; e < 7; ++e) g_reg[(size_t)i * ld_greg + e] = (float)(t.d_reg[e] * k_reg + t.d_corner[e] * k_corner);
}

}  // namespace df3d

using namespace df3d;

static int check_target_cfg(const df3d_roi_target_cfg *c) {
  DF3D_CHECK_ARG(c, "roi_targets: null config");
  DF3D_CHECK_ARG(c->batch > 0 && c->batch <= 65535, "roi_targets: 1..65535 frames (got %d)", c->batch);
  DF3D_CHECK_ARG(c->num_rois > 0 && c->num_rois <= MAX_ROIS, "roi_targets: 1..%d RoIs per frame (got R = %d)", MAX_ROIS, c->num_rois);
  DF3D_CHECK_ARG(c->roi_per_image > 0 && c->roi_per_image <= MAX_SAMPLES, "roi_targets: 1..%d sampled RoIs per frame (got M = %d)",
                 MAX_SAMPLES, c->roi_per_image);
  DF3D_CHECK_ARG(c->max_gt > 0 && c->max_gt <= MAX_GT, "roi_targets: 1..%d ground-truth rows per frame (got G = %d)", MAX_GT, c->max_gt);
  DF3D_CHECK_ARG(c->fg_per_image >= 0 && c->fg_per_image <= c->roi_per_image, "roi_targets: fg_per_image %d outside 0..M", c->fg_per_image);
  DF3D_CHECK_ARG(c->hard_bg_ratio >= 0.0 && c->hard_bg_ratio <= 1.0, "roi_targets: hard_bg_ratio %g outside [0, 1]", c->hard_bg_ratio);
  DF3D_CHECK_ARG(c->cls_score_type == DF3D_ROI_SCORE_ROI_IOU || c->cls_score_type == DF3D_ROI_SCORE_CLS,
                 "roi_targets: unknown cls_score_type %d", c->cls_score_type);
  DF3D_CHECK_ARG(c->cls_fg_thresh > c->cls_bg_thresh, "roi_targets: cls_fg_thresh must exceed cls_bg_thresh");
  return DF3D_OK;
}

struct TargetPlan {
  size_t iou, asg, fg, bg, total;
};

static void target_plan(int batch, int R, TargetPlan &p) {
  WsLayout l;
  const size_t n = (size_t)batch * R * 4;
  p.iou = l.take(n), p.asg = l.take(n), p.fg = l.take(n), p.bg = l.take(n);
  p.total = l.total();
}

extern "C" size_t df3d_roi_targets_workspace_bytes(const df3d_roi_target_cfg *cfg) {
  if (!cfg || cfg->batch <= 0 || cfg->num_rois <= 0 || cfg->num_rois > MAX_ROIS) return 0;
  TargetPlan p;
  target_plan(cfg->batch, cfg->num_rois, p);
  return p.total;
}

extern "C" int df3d_roi_targets(const float *rois, const float *roi_scores, const int64_t *roi_labels, const float *gt_boxes,
                                const float *u_fg, const float *u_slot, const df3d_roi_target_cfg *cfg, float *out_rois,
                                int64_t *out_labels, float *out_scores, float *out_ious, int32_t *roi_inds, float *gt_of_rois_src,
                                float *gt_of_rois, int32_t *reg_valid_mask, float *rcnn_cls_labels, int32_t *counts,
                                void *workspace, size_t workspace_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  int rc = check_target_cfg(cfg);
  if (rc) return rc;
  DF3D_CHECK_ARG(rois && roi_scores && roi_labels && gt_boxes && u_fg && u_slot, "roi_targets: null input");
  DF3D_CHECK_ARG(out_rois && out_labels && out_scores && out_ious && roi_inds && gt_of_rois_src && gt_of_rois && reg_valid_mask &&
                     rcnn_cls_labels && counts && workspace,
                 "roi_targets: null output");
  TargetPlan p;
  target_plan(cfg->batch, cfg->num_rois, p);
  DF3D_CHECK_ARG(workspace_bytes >= p.total, "roi_targets: workspace %zu < %zu bytes", workspace_bytes, p.total);
  TargetArgs a;
  memset(&a, 0, sizeof(a));
  a.rois = rois, a.scores = roi_scores, a.labels = (const long long *)roi_labels, a.gt = gt_boxes, a.u_fg = u_fg, a.u_slot = u_slot;
  a.c = *cfg;
  a.o_rois = out_rois, a.o_labels = (long long *)out_labels, a.o_scores = out_scores, a.o_ious = out_ious, a.o_inds = roi_inds;
  a.o_src = gt_of_rois_src, a.o_gt = gt_of_rois, a.o_mask = reg_valid_mask, a.o_cls = rcnn_cls_labels, a.counts = counts;
  char *ws = (char *)workspace;
  a.w_iou = (float *)(ws + p.iou), a.w_asg = (int32_t *)(ws + p.asg), a.w_fg = (int32_t *)(ws + p.fg), a.w_bg = (int32_t *)(ws + p.bg);
  hipLaunchKernelGGL(roi_targets_kernel, dim3(cfg->batch), dim3(256), 0, stream, a);
  DF3D_LAUNCH_CHECK();
  return DF3D_OK;
}

static int fill_rcnn_args(RcnnArgs &a, const char *what, const float *rcnn_cls, int ld_cls, const float *rcnn_reg, int ld_reg,
                          const float *rois, const float *gt_of_rois, const float *gt_of_rois_src, const int32_t *reg_valid_mask,
                          const float *rcnn_cls_labels, const df3d_rcnn_loss_cfg *cfg) {
  DF3D_CHECK_ARG(cfg, "%s: null config", what);
  DF3D_CHECK_ARG(cfg->num_rows > 0 && cfg->num_rows <= 65535 * MAX_SAMPLES, "%s: bad row count %d", what, cfg->num_rows);
  DF3D_CHECK_ARG(cfg->beta >= 0.f, "%s: smooth-L1 beta >= 0 (got %g)", what, (double)cfg->beta);
  DF3D_CHECK_ARG(rcnn_cls && rcnn_reg && rois && gt_of_rois && gt_of_rois_src && reg_valid_mask && rcnn_cls_labels, "%s: null input", what);
  DF3D_CHECK_ARG(ld_cls >= 1 && ld_reg >= 7, "%s: a row stride is smaller than its channel count", what);
  memset(&a, 0, sizeof(a));
  a.cls = rcnn_cls, a.reg = rcnn_reg, a.rois = rois, a.gt = gt_of_rois, a.src = gt_of_rois_src, a.labels = rcnn_cls_labels;
  a.mask = reg_valid_mask;
  a.ld_cls = ld_cls, a.ld_reg = ld_reg, a.N = cfg->num_rows, a.corner = cfg->corner_loss != 0;
  for (int e = 0; e < 7; ++e) a.cw[e] = (double)cfg->code_weights[e];
  a.beta = (double)cfg->beta;
  a.weight[0] = (double)cfg->cls_weight, a.weight[1] = (double)cfg->reg_weight, a.weight[2] = (double)cfg->corner_weight;
  return DF3D_OK;
}

extern "C" size_t df3d_rcnn_loss_workspace_bytes(const df3d_rcnn_loss_cfg *cfg) {
  if (!cfg || cfg->num_rows <= 0) return 0;
  return partials_bytes(cdiv(cfg->num_rows, 256), 5);
}

extern "C" int df3d_rcnn_loss(const float *rcnn_cls, int ld_cls, const float *rcnn_reg, int ld_reg, const float *rois,
                              const float *gt_of_rois, const float *gt_of_rois_src, const int32_t *reg_valid_mask,
                              const float *rcnn_cls_labels, const df3d_rcnn_loss_cfg *cfg, float *losses, double *norms,
                              void *workspace, size_t workspace_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  RcnnArgs a;
  int rc = fill_rcnn_args(a, "rcnn_loss", rcnn_cls, ld_cls, rcnn_reg, ld_reg, rois, gt_of_rois, gt_of_rois_src, reg_valid_mask,
                          rcnn_cls_labels, cfg);
  if (rc) return rc;
  DF3D_CHECK_ARG(losses && norms && workspace, "rcnn_loss: null output");
  const int nblocks = cdiv(a.N, 256);
  const size_t need = partials_bytes(nblocks, 5);
  DF3D_CHECK_ARG(workspace_bytes >= need, "rcnn_loss: workspace %zu < %zu bytes", workspace_bytes, need);
  double *partials = (double *)workspace;
  hipLaunchKernelGGL(rcnn_loss_kernel, dim3(nblocks), dim3(256), 0, stream, a, partials);
  DF3D_LAUNCH_CHECK();
  hipLaunchKernelGGL(rcnn_loss_final_kernel, dim3(1), dim3(256), 0, stream, partials, nblocks, a.weight[0], a.weight[1], a.weight[2],
                     losses, norms);
  DF3D_LAUNCH_CHECK();
  return DF3D_OK;
}

extern "C" int df3d_rcnn_loss_grad(const float *rcnn_cls, int ld_cls, const float *rcnn_reg, int ld_reg, const float *rois,
                                   const float *gt_of_rois, const float *gt_of_rois_src, const int32_t *reg_valid_mask,
                                   const float *rcnn_cls_labels, const df3d_rcnn_loss_cfg *cfg, const double *norms,
                                   const float *grad_losses, float *grad_cls, int ld_gcls, float *grad_reg, int ld_greg,
                                   void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  RcnnArgs a;
  int rc = fill_rcnn_args(a, "rcnn_loss_grad", rcnn_cls, ld_cls, rcnn_reg, ld_reg, rois, gt_of_rois, gt_of_rois_src, reg_valid_mask,
                          rcnn_cls_labels, cfg);
  if (rc) return rc;
  DF3D_CHECK_ARG(norms && grad_losses && grad_cls && grad_reg, "rcnn_loss_grad: null gradient");
  DF3D_CHECK_ARG(ld_gcls >= 1 && ld_greg >= 7, "rcnn_loss_grad: a gradient row stride is smaller than its channel count");
  hipLaunchKernelGGL(rcnn_loss_grad_kernel, dim3(cdiv(a.N, 256)), dim3(256), 0, stream, a, norms, grad_losses, grad_cls, ld_gcls,
                     grad_reg, ld_greg);
  DF3D_LAUNCH_CHECK();
  return DF3D_OK;
}
