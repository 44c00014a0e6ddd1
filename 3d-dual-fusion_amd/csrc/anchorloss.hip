// Voxel-RCNN first-stage training: anchor target assignment and the RPN losses on the device.
//
// Reference: VR/pcdet/models/dense_heads/target_assigner/axis_aligned_target_assigner.py:36-210 loops over frames and anchor
// classes in Python: a `while cur_gt[cnt].sum() == 0` loop that reads one row back per iteration, a dense [H*W*A_set, G] IoU
// matrix, four nonzero() calls and a [B, H*W*A, 7] target tensor; anchor_head_template.py:101-223 then builds one-hot tensors
// and three dense loss maps over every anchor, although only the positives carry a regression or direction term.
//
// df3d_anchor_assign -- three launches for all frames and anchor sets, no host round trip; anchors come from the TABLES:
//   assign_prepare   per frame: valid GT count, aligned BEV boxes + areas + classes of the GT rows, counters zeroed
//   assign_pass<0>   IoU of every (anchor, GT of the anchor's class); per (frame, set, GT) the max over the set's anchors:
//                    wave max, then one INTEGER atomicMax per wave on the float's bits (IoU >= 0: the order of the bits is
//                    the order of the floats, and the result does not depend on arrival order)
//   assign_pass<1>   the same IoUs again (the same device function, no contraction: the forced-match rule is a float
//                    equality); arg-max, thresholds, forced matches -> labels, gt_ids; positives counted by wave ballot and
//                    one integer atomicAdd per wave; optionally the reference's dense targets and weights
// df3d_anchor_loss / df3d_anchor_loss_grad -- get_cls_layer_loss + get_box_reg_layer_loss fused: one thread per anchor, the
// regression target encoded on the fly from gt_boxes[b, gt_id] and the table anchor; fp64 partials per workgroup at fixed
// positions and an ordered final sum (bit-identical from run to run); the gradient kernel writes every element of the three
// maps (zeros where nothing contributes) and reads the upstream gradients from device memory.
#include <cstring>

#include "common.h"

// the reference's float expressions, evaluated operation by operation (no fused multiply-adds): both passes of the
// assignment must give the same float for the same (anchor, GT) pair
#pragma clang fp contract(off)
#include "anchor_box.h"
#include "loss_terms.h"

namespace df3d {

constexpr int GT_CHUNK = DF3D_ANCHOR_GT_CHUNK;
constexpr float PI_F = 3.14159265358979323846f;
constexpr float QUARTER_PI_F = (float)(3.14159265358979323846 / 4.0);
constexpr float TWO_PI_F = (float)(2.0 * 3.14159265358979323846);

struct AssignArgs {
  AnchorTab t;
  const float *gt;                        // [B][M][8]
  int M, set_class[DF3D_MAX_ANCHORS];     // ground-truth rows per frame; the class an anchor set serves
  float matched[DF3D_MAX_ANCHORS], unmatched[DF3D_MAX_ANCHORS];
  float *gt_bev;                          // [B][M][5]: x1, y1, x2, y2, area
  int32_t *gt_cls;                        // [B][M]: class of the row, 0 = padding or past the valid count
  int32_t *valid;                         // [B]
  unsigned *gt_max;                       // [B][S][M]: bits of the largest IoU of the GT with an anchor of the set
  int32_t *labels, *gt_ids, *num_pos;
  float *reg_targets, *reg_weights;       // optional
};

struct Bev {
  float x1, y1, x2, y2, area;
};

// boxes3d_lidar_to_aligned_bev_boxes (box_utils.py:309-320) and the area boxes_iou_normal takes of it
__device__ __forceinline__ Bev aligned_bev(float x, float y, float dx, float dy, float r) {
  const float rot = fabsf(r - floorf(r / PI_F + 0.5f) * PI_F);
  const bool keep = rot < QUARTER_PI_F;
  const float hx = (keep ? dx : dy) / 2.f, hy = (keep ? dy : dx) / 2.f;
  Bev b;
  b.x1 = x - hx, b.y1 = y - hy, b.x2 = x + hx, b.y2 = y + hy;
  b.area = (b.x2 - b.x1) * (b.y2 - b.y1);
  return b;
}

// boxes_iou_normal (box_utils.py:286-306) of one pair
__device__ __forceinline__ float bev_iou(const Bev &a, float gx1, float gy1, float gx2, float gy2, float garea) {
  const float x_min = fmaxf(a.x1, gx1), x_max = fminf(a.x2, gx2);
  const float y_min = fmaxf(a.y1, gy1), y_max = fminf(a.y2, gy2);
  const float x_len = fmaxf(x_max - x_min, 0.f), y_len = fmaxf(y_max - y_min, 0.f);
  const float inter = x_len * y_len;
  return inter / fmaxf(a.area + garea - inter, 1e-6f);
}

// grid (batch), 256 threads
__global__ __launch_bounds__(256) void assign_prepare_kernel(AssignArgs a) {
  __shared__ int s_last;
  const int b = blockIdx.x, M = a.M;
  const float *gt = a.gt + (size_t)b * M * 8;
  if (threadIdx.x == 0) s_last = 0;
  __syncthreads();
  int last = 0;
  for (int m = threadIdx.x; m < M; m += 256) {
    const float *g = gt + (size_t)m * 8;
    const float sum = (((((g[0] + g[1]) + g[2]) + g[3]) + g[4]) + g[5]) + g[6];
    if (sum != 0.f) last = m;                                     // (NaN counts as non-zero, as in the reference)
  }
  atomicMax(&s_last, last);
  __syncthreads();
  const int valid = s_last + 1;                                   // `while cnt > 0 and cur_gt[cnt].sum() == 0`: at least 1
  if (threadIdx.x == 0) {
    a.valid[b] = valid;
    a.num_pos[b] = 0;
  }
  for (int m = threadIdx.x; m < M; m += 256) {
    const float *g = gt + (size_t)m * 8;
    const Bev v = aligned_bev(g[0], g[1], g[3], g[4], g[6]);
    float *o = a.gt_bev + ((size_t)b * M + m) * 5;
    o[0] = v.x1, o[1] = v.y1, o[2] = v.x2, o[3] = v.y2, o[4] = v.area;
    const int c = (int)g[7];
    a.gt_cls[(size_t)b * M + m] = (m < valid && c >= 1) ? c : 0;
  }
  for (int i = threadIdx.x; i < a.t.S * M; i += 256) a.gt_max[(size_t)b * a.t.S * M + i] = 0u;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// grid (ceil(H*W / 256), batch): one thread per pixel, the A anchors of the pixel in turn, so that the lanes of a wave
// always hold anchors of ONE set.  PASS 0: per-GT maxima; PASS 1: labels.
template <int PASS>
__global__ __launch_bounds__(256) void assign_pass_kernel(AssignArgs a) {
  __shared__ float s_bev[GT_CHUNK][5];
  __shared__ int s_cls[GT_CHUNK];
  const AnchorTab &t = a.t;
  const int b = blockIdx.y, M = a.M, HW = t.H * t.W;
  const int pix = blockIdx.x * 256 + threadIdx.x;
  const bool live = pix < HW;
  const int valid = a.valid[b];
  const int nchunks = (valid + GT_CHUNK - 1) / GT_CHUNK;
  const size_t per_frame = (size_t)HW * t.A;
  int positives = 0;
  for (int an = 0; an < t.A; ++an) {
    const int s = t.set[an];
    const int my_class = a.set_class[s];
    float xa, ya;
    const float *an5 = anchor_at(t, live ? pix : 0, an, xa, ya);    // (a thread past the map reads pixel 0 and writes nothing)
    const Bev box = aligned_bev(xa, ya, an5[1], an5[2], an5[4]);
    float best = -1.f;
    int arg = -1;
    bool forced = false;
    for (int c = 0; c < nchunks; ++c) {
      const int c0 = c * GT_CHUNK, n = min(GT_CHUNK, valid - c0);
      if (nchunks > 1 || an == 0) {                                 // (one chunk: staged once for all anchors of the pixel)
        __syncthreads();
        for (int i = threadIdx.x; i < n * 5; i += 256) s_bev[i / 5][i % 5] = a.gt_bev[((size_t)b * M + c0) * 5 + i];
        for (int i = threadIdx.x; i < n; i += 256) s_cls[i] = a.gt_cls[(size_t)b * M + c0 + i];
        __syncthreads();
      }
      for (int g = 0; g < n; ++g) {
        if (s_cls[g] != my_class) continue;                         // uniform over the workgroup
        const float iou = live ? bev_iou(box, s_bev[g][0], s_bev[g][1], s_bev[g][2], s_bev[g][3], s_bev[g][4]) : 0.f;
        unsigned *slot = a.gt_max + ((size_t)b * t.S + s) * M + c0 + g;
        if (PASS == 0) {
          const float w = wave_max(iou);
          if (w > 0.f && (threadIdx.x & 63) == 0) atomicMax(slot, __float_as_uint(w));
        } else {
          if (iou > best) {                                         // first maximum wins (argmax(dim=1))
            best = iou;
            arg = c0 + g;
          }
          const unsigned gm = *slot;                                // a GT whose max is 0 matches nothing
          forced |= gm != 0u && __float_as_uint(iou) == gm;
        }
      }
    }
    if (PASS == 1) {
      int label = 0, id = -1;                                       // no GT of this class in the frame: labels[:] = 0
      if (arg >= 0) {
        const bool pos = best >= a.matched[s];
        label = -1;
        if (forced || pos) {
          label = a.gt_cls[(size_t)b * M + arg];
          id = arg;
        }
        if (best < a.unmatched[s] && !forced) label = 0;
      }
      const bool positive = live && label > 0;
      positives += positive ? 1 : 0;
      if (live) {
        const size_t o = (size_t)b * per_frame + (size_t)pix * t.A + an;
        a.labels[o] = label;
        a.gt_ids[o] = id;
        if (a.reg_weights) a.reg_weights[o] = positive ? 1.f : 0.f;
        if (a.reg_targets) {
          float tg[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
          if (positive) residual_encode(a.gt + ((size_t)b * M + arg) * 8, xa, ya, an5[0], an5[1], an5[2], an5[3], an5[4], tg);
#pragma unroll
          for (int e = 0; e < 7; ++e) a.reg_targets[o * 7 + e] = tg[e];
        }
      }
    }
  }
  if (PASS == 1) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) positives += __shfl_xor(positives, o, 64);
    if (positives > 0 && (threadIdx.x & 63) == 0) atomicAdd(a.num_pos + b, positives);
  }
}

// ---- losses ------------------------------------------------------------------------------------------------------------
struct LossArgs {
  AnchorTab t;
  const float *cls, *box, *dir, *gt;
  int M, ld_cls, ld_box, ld_dir;          // M: ground-truth rows per frame
  const int32_t *labels, *gt_ids, *num_pos;
  int C, NB;
  float dir_offset;
  double cw[7], beta;
  double weight[3];                       // cls, loc, dir
};

// what one anchor contributes: its rows, label, weight and (for a positive) the target and the direction bin
struct Site {
  long long row;
  int b, an, label, bin;
  bool positive;
  double w, tg[7];
};

__device__ __forceinline__ void load_site(const LossArgs &a, long long i, Site &s) {
  const AnchorTab &t = a.t;
  const long long per_frame = (long long)t.H * t.W * t.A;
  s.b = (int)(i / per_frame);
  const int idx = (int)(i - (long long)s.b * per_frame);
  int pix;
  anchor_split(t, idx, pix, s.an);
  s.row = (long long)s.b * t.H * t.W + pix;
  s.label = a.labels[i];
  const int np = a.num_pos[s.b];
  s.w = 1.0 / (double)(np > 1 ? np : 1);
  const int id = a.gt_ids[i];
  s.positive = s.label > 0 && id >= 0 && id < a.M;
  s.bin = 0;
  if (!s.positive) return;
  float xa, ya;
  const float *an5 = anchor_at(t, pix, s.an, xa, ya);
  const float *g = a.gt + ((size_t)s.b * a.M + id) * 8;
  // the target in fp64 (the loss values), and code 6 in fp32 as the reference holds it (the direction bin is a floor)
  residual_encode<double>(g, xa, ya, an5[0], an5[1], an5[2], an5[3], an5[4], s.tg);
  if (a.dir) {                                                      // get_direction_target (anchor_head_template.py:146-160)
    const float t6 = g[6] - an5[4];
    const float rot_gt = t6 + an5[4];
    const float v = rot_gt - a.dir_offset;
    const float offset_rot = v - floorf(v / TWO_PI_F + 0.f) * TWO_PI_F;
    const float per_bin = (float)(2.0 * 3.14159265358979323846 / a.NB);
    int bin = (int)floorf(offset_rot / per_bin);
    s.bin = bin < 0 ? 0 : (bin > a.NB - 1 ? a.NB - 1 : bin);
  }
}

// code-weighted difference of code e (add_sin_difference on code 6) and its derivative with respect to the prediction
__device__ __forceinline__ void code_diff(const LossArgs &a, const float *p, const Site &s, int e, double &d, double &dd) {
  if (e == 6) {
    const double p6 = (double)p[6], t6 = s.tg[6];
    d = a.cw[6] * (sin(p6) * cos(t6) - cos(p6) * sin(t6));
    dd = a.cw[6] * (cos(p6) * cos(t6) + sin(p6) * sin(t6));
  } else {
    d = a.cw[e] * ((double)p[e] - s.tg[e]);
    dd = a.cw[e];
  }
}

// grid (ceil(B*N / 256)): partials[block][3] (cls, loc, dir)
__global__ __launch_bounds__(256) void anchor_loss_kernel(LossArgs a, long long total, double *__restrict__ partials) {
  __shared__ double s_red[4];
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  double l_cls = 0.0, l_loc = 0.0, l_dir = 0.0;
  if (i < total) {
    Site s;
    load_site(a, i, s);
    if (s.label >= 0) {
      const float *c = a.cls + s.row * a.ld_cls + s.an * a.C;
      for (int k = 0; k < a.C; ++k) {
        const double tt = (a.C == 1 ? s.label > 0 : s.label == k + 1) ? 1.0 : 0.0;
        double v, dv;
        focal((double)c[k], tt, v, dv);
        l_cls += v * s.w;
      }
    }
    if (s.positive) {
      const float *p = a.box + s.row * a.ld_box + s.an * 7;
      for (int e = 0; e < 7; ++e) {
        double d, dd, v, slope;
        code_diff(a, p, s, e, d, dd);
        smooth_l1(d, a.beta, v, slope);                             // (beta >= 1e-5 here: check_loss_cfg)
        l_loc += v * s.w;
      }
      if (a.dir) {
        const float *q = a.dir + s.row * a.ld_dir + s.an * a.NB;
        double mx, sum;
        softmax_stats(q, a.NB, mx, sum);
        l_dir = (mx + log(sum) - (double)q[s.bin]) * s.w;
      }
    }
  }
  const double v[3] = {l_cls, l_loc, l_dir};
  partials_write<3>(v, partials, s_red);
}

// one workgroup: the partials in a fixed order -> the three scalars, each sum / B * weight
__global__ __launch_bounds__(256) void anchor_loss_final_kernel(const double *__restrict__ partials, int nblocks, int batch,
                                                                double w_cls, double w_loc, double w_dir,
                                                                float *__restrict__ losses) {
  __shared__ double s_red[4];
  double tot[3];
  partials_sum<3>(partials, nblocks, tot, s_red);
  const double w[3] = {w_cls, w_loc, w_dir};
  if (threadIdx.x == 0)
    for (int j = 0; j < 3; ++j) losses[j] = (float)(tot[j] / (double)batch * w[j]);
}

// grid (ceil(B*N / 256)): every element of the three gradient maps
__global__ __launch_bounds__(256) void anchor_loss_grad_kernel(LossArgs a, long long total, const float *__restrict__ upstream,
                                                               float *__restrict__ g_cls, int ld_gcls, float *__restrict__ g_box,
                                                               int ld_gbox, float *__restrict__ g_dir, int ld_gdir) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  Site s;
  load_site(a, i, s);
  const double inv_b = 1.0 / (double)a.t.batch;
  const double k_cls = (double)upstream[0] * a.weight[0] * inv_b * s.w;
  const double k_loc = (double)upstream[1] * a.weight[1] * inv_b * s.w;
  const double k_dir = (double)upstream[2] * a.weight[2] * inv_b * s.w;
  const float *c = a.cls + s.row * a.ld_cls + s.an * a.C;
  float *gc = g_cls + s.row * ld_gcls + s.an * a.C;
  for (int k = 0; k < a.C; ++k) {
    double v = 0.0, dv = 0.0;
    if (s.label >= 0) {
      const double tt = (a.C == 1 ? s.label > 0 : s.label == k + 1) ? 1.0 : 0.0;
      focal((double)c[k], tt, v, dv);
    }
    gc[k] = (float)(dv * k_cls);
  }
  const float *p = a.box + s.row * a.ld_box + s.an * 7;
  float *gb = g_box + s.row * ld_gbox + s.an * 7;
  for (int e = 0; e < 7; ++e) {
    double g = 0.0;
    if (s.positive) {
      double d, dd, v, slope;
      code_diff(a, p, s, e, d, dd);
      smooth_l1(d, a.beta, v, slope);
      g = slope * dd * k_loc;
    }
    gb[e] = (float)g;
  }
  if (a.dir) {
    const float *q = a.dir + s.row * a.ld_dir + s.an * a.NB;
    float *gd = g_dir + s.row * ld_gdir + s.an * a.NB;
    if (s.positive) {
      double mx, sum;
      softmax_stats(q, a.NB, mx, sum);
      for (int k = 0; k < a.NB; ++k) gd[k] = (float)((exp((double)q[k] - mx) / sum - (k == s.bin ? 1.0 : 0.0)) * k_dir);
    } else {
      for (int k = 0; k < a.NB; ++k) gd[k] = 0.f;
    }
  }
}

}  // namespace df3d

using namespace df3d;

// the limits the assignment and the losses share: the table's, then the ground-truth rows; `what` names the entry point
static int check_tables(const df3d_anchor_cfg *c, int max_gt, const char *what) {
  int rc = anchor_check(c, what);
  if (rc) return rc;
  DF3D_CHECK_ARG(max_gt > 0 && max_gt <= DF3D_ANCHOR_MAX_GT, "%s: 1..%d ground-truth rows per frame (got M = %d)", what,
                 DF3D_ANCHOR_MAX_GT, max_gt);
  return DF3D_OK;
}

struct AssignPlan {
  size_t gt_bev, gt_cls, valid, gt_max, total;
};

static void assign_plan(int batch, int sets, int M, AssignPlan &p) {
  WsLayout l;
  const size_t rows = (size_t)batch * M;
  p.gt_bev = l.take(rows * 5 * 4);
  p.gt_cls = l.take(rows * 4);
  p.valid = l.take((size_t)batch * 4);
  p.gt_max = l.take(rows * sets * 4);
  p.total = l.total();
}

static int check_assign_cfg(const df3d_anchor_assign_cfg *cfg) {
  DF3D_CHECK_ARG(cfg, "anchor_assign: null config");
  int rc = check_tables(&cfg->anchors, cfg->max_gt, "anchor_assign");
  if (rc) return rc;
  for (int s = 0; s < cfg->anchors.num_sets; ++s)
    DF3D_CHECK_ARG(cfg->set_class[s] >= 1, "anchor_assign: anchor set %d serves class %d (class ids are 1-based)", s,
                   cfg->set_class[s]);
  return DF3D_OK;
}

extern "C" size_t df3d_anchor_assign_workspace_bytes(const df3d_anchor_assign_cfg *cfg) {
  if (!cfg || cfg->anchors.batch <= 0 || cfg->anchors.num_sets <= 0 || cfg->anchors.num_sets > DF3D_MAX_ANCHORS || cfg->max_gt <= 0 ||
      cfg->max_gt > DF3D_ANCHOR_MAX_GT)
    return 0;
  AssignPlan p;
  assign_plan(cfg->anchors.batch, cfg->anchors.num_sets, cfg->max_gt, p);
  return p.total;
}

extern "C" int df3d_anchor_assign(const float *x_shifts, const float *y_shifts, const float *gt_boxes,
                                  const df3d_anchor_assign_cfg *cfg, int32_t *labels, int32_t *gt_ids, int32_t *num_pos,
                                  float *box_reg_targets, float *reg_weights, void *workspace, size_t workspace_bytes,
                                  void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  int rc = check_assign_cfg(cfg);
  if (rc) return rc;
  DF3D_CHECK_ARG(x_shifts && y_shifts && gt_boxes, "anchor_assign: null input");
  DF3D_CHECK_ARG(labels && gt_ids && num_pos && workspace, "anchor_assign: null output");
  const df3d_anchor_cfg *c = &cfg->anchors;
  AssignPlan p;
  assign_plan(c->batch, c->num_sets, cfg->max_gt, p);
  DF3D_CHECK_ARG(workspace_bytes >= p.total, "anchor_assign: workspace %zu < %zu bytes", workspace_bytes, p.total);

  AssignArgs a;
  memset(&a, 0, sizeof(a));
  anchor_fill(a.t, c, x_shifts, y_shifts);
  a.M = cfg->max_gt, a.gt = gt_boxes;
  for (int s = 0; s < c->num_sets; ++s) {
    a.set_class[s] = cfg->set_class[s];
    a.matched[s] = cfg->matched_threshold[s];
    a.unmatched[s] = cfg->unmatched_threshold[s];
  }
  char *ws = (char *)workspace;
  a.gt_bev = (float *)(ws + p.gt_bev), a.gt_cls = (int32_t *)(ws + p.gt_cls), a.valid = (int32_t *)(ws + p.valid);
  a.gt_max = (unsigned *)(ws + p.gt_max);
  a.labels = labels, a.gt_ids = gt_ids, a.num_pos = num_pos, a.reg_targets = box_reg_targets, a.reg_weights = reg_weights;
  const dim3 grid(cdiv((long long)c->H * c->W, 256), c->batch);
  hipLaunchKernelGGL(assign_prepare_kernel, dim3(c->batch), dim3(256), 0, stream, a);
  DF3D_LAUNCH_CHECK();
  hipLaunchKernelGGL(assign_pass_kernel<0>, grid, dim3(256), 0, stream, a);
  DF3D_LAUNCH_CHECK();
  hipLaunchKernelGGL(assign_pass_kernel<1>, grid, dim3(256), 0, stream, a);
  DF3D_LAUNCH_CHECK();
  return DF3D_OK;
}

static int check_loss_cfg(const df3d_anchor_loss_cfg *cfg, const char *what) {
  DF3D_CHECK_ARG(cfg, "%s: null config", what);
  int rc = check_tables(&cfg->anchors, cfg->max_gt, what);
  if (rc) return rc;
  DF3D_CHECK_ARG(cfg->anchors.num_classes > 0 && cfg->anchors.num_dir_bins >= 0, "%s: bad class / direction-bin count", what);
  DF3D_CHECK_ARG(cfg->beta >= 1e-5f, "%s: smooth-L1 beta >= 1e-5 (got %g)", what, (double)cfg->beta);
  return DF3D_OK;
}

static int fill_loss_args(LossArgs &a, const char *what, const float *cls, int ld_cls, const float *box, int ld_box,
                          const float *dir, int ld_dir, const float *x_shifts, const float *y_shifts, const int32_t *labels,
                          const int32_t *gt_ids, const int32_t *num_pos, const float *gt_boxes, const df3d_anchor_loss_cfg *cfg) {
  int rc = check_loss_cfg(cfg, what);
  if (rc) return rc;
  const df3d_anchor_cfg *c = &cfg->anchors;
  DF3D_CHECK_ARG(cls && box && x_shifts && y_shifts && labels && gt_ids && num_pos && gt_boxes, "%s: null input", what);
  DF3D_CHECK_ARG(ld_cls >= c->num_anchors * c->num_classes && ld_box >= c->num_anchors * 7,
                 "%s: a row stride is smaller than its channel count", what);
  DF3D_CHECK_ARG(!dir || (c->num_dir_bins > 0 && ld_dir >= c->num_anchors * c->num_dir_bins),
                 "%s: direction map needs num_dir_bins > 0 and ld_dir >= anchors * bins", what);
  memset(&a, 0, sizeof(a));
  anchor_fill(a.t, c, x_shifts, y_shifts);
  a.M = cfg->max_gt, a.cls = cls, a.box = box, a.dir = dir, a.gt = gt_boxes;
  a.ld_cls = ld_cls, a.ld_box = ld_box, a.ld_dir = ld_dir;
  a.labels = labels, a.gt_ids = gt_ids, a.num_pos = num_pos;
  a.C = c->num_classes, a.NB = c->num_dir_bins, a.dir_offset = c->dir_offset;
  for (int e = 0; e < 7; ++e) a.cw[e] = (double)cfg->code_weights[e];
  a.beta = (double)cfg->beta;
  a.weight[0] = (double)cfg->cls_weight, a.weight[1] = (double)cfg->loc_weight, a.weight[2] = (double)cfg->dir_weight;
  return DF3D_OK;
}

static long long loss_total(const df3d_anchor_cfg *c) { return (long long)c->batch * c->H * c->W * c->num_anchors; }

extern "C" size_t df3d_anchor_loss_workspace_bytes(const df3d_anchor_loss_cfg *cfg) {
  if (!cfg || cfg->anchors.batch <= 0 || cfg->anchors.H <= 0 || cfg->anchors.W <= 0 || cfg->anchors.num_anchors <= 0) return 0;
  return partials_bytes(cdiv(loss_total(&cfg->anchors), 256), 3);
}

extern "C" int df3d_anchor_loss(const float *cls, int ld_cls, const float *box, int ld_box, const float *dir, int ld_dir,
                                const float *x_shifts, const float *y_shifts, const int32_t *labels, const int32_t *gt_ids,
                                const int32_t *num_pos, const float *gt_boxes, const df3d_anchor_loss_cfg *cfg, float *losses,
                                void *workspace, size_t workspace_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  LossArgs a;
  int rc = fill_loss_args(a, "anchor_loss", cls, ld_cls, box, ld_box, dir, ld_dir, x_shifts, y_shifts, labels, gt_ids, num_pos,
                          gt_boxes, cfg);
  if (rc) return rc;
  DF3D_CHECK_ARG(losses && workspace, "anchor_loss: null output");
  const long long total = loss_total(&cfg->anchors);
  const int nblocks = cdiv(total, 256);
  const size_t need = partials_bytes(nblocks, 3);
  DF3D_CHECK_ARG(workspace_bytes >= need, "anchor_loss: workspace %zu < %zu bytes", workspace_bytes, need);
  double *partials = (double *)workspace;
  hipLaunchKernelGGL(anchor_loss_kernel, dim3(nblocks), dim3(256), 0, stream, a, total, partials);
  DF3D_LAUNCH_CHECK();
  hipLaunchKernelGGL(anchor_loss_final_kernel, dim3(1), dim3(256), 0, stream, partials, nblocks, cfg->anchors.batch, a.weight[0],
                     a.weight[1], a.weight[2], losses);
  DF3D_LAUNCH_CHECK();
  return DF3D_OK;
}

extern "C" int df3d_anchor_loss_grad(const float *cls, int ld_cls, const float *box, int ld_box, const float *dir, int ld_dir,
                                     const float *x_shifts, const float *y_shifts, const int32_t *labels, const int32_t *gt_ids,
                                     const int32_t *num_pos, const float *gt_boxes, const df3d_anchor_loss_cfg *cfg,
                                     const float *grad_losses, float *grad_cls, int ld_gcls, float *grad_box, int ld_gbox,
                                     float *grad_dir, int ld_gdir, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  LossArgs a;
  int rc = fill_loss_args(a, "anchor_loss_grad", cls, ld_cls, box, ld_box, dir, ld_dir, x_shifts, y_shifts, labels, gt_ids,
                          num_pos, gt_boxes, cfg);
  if (rc) return rc;
  const df3d_anchor_cfg *c = &cfg->anchors;
  DF3D_CHECK_ARG(grad_losses && grad_cls && grad_box && (grad_dir || !dir), "anchor_loss_grad: null gradient");
  DF3D_CHECK_ARG(ld_gcls >= c->num_anchors * c->num_classes && ld_gbox >= c->num_anchors * 7 &&
                     (!dir || ld_gdir >= c->num_anchors * c->num_dir_bins),
                 "anchor_loss_grad: a gradient row stride is smaller than its channel count");
  const long long total = loss_total(c);
  hipLaunchKernelGGL(anchor_loss_grad_kernel, dim3(cdiv(total, 256)), dim3(256), 0, stream, a, total, grad_losses, grad_cls,
                     ld_gcls, grad_box, ld_gbox, grad_dir, ld_gdir);
  DF3D_LAUNCH_CHECK();
  return DF3D_OK;
}
