// Detection tail, part 3: the Voxel-RCNN tail from head maps to boxes on the device.
//
// Reference: VR/pcdet/models/dense_heads/anchor_head_template.py:225-272 decodes EVERY anchor of every frame
// (ResidualCoder.decode_torch + the direction classifier: ~25 elementwise launches over [B, H*W*A, 7]) although only
// NMS_PRE_MAXSIZE of them survive the top-k; roi_head_template.py:45-102 (proposal_layer) and
// detector3d_template.py:178-284 (post_processing) then loop over the frames in Python with several host round trips
// each (len(selected), boolean masks, nonzero).
//
// df3d_anchor_proposals -- five steps for all frames, no host round trip:
//   anchor_keys      one 64-bit key per anchor: [frame 8 | 0 0 | ~ordered(raw logit) 32 | anchor index 22]; ascending key =
//                    descending logit, ties by ascending anchor index.  (The select of topk.hip orders 54 key bits; the
//                    heads' [0x3F800000 - score bits | index 24] packing holds scores in (0, 1] only, logits need all 32.)
//   top-k select     (topk.hip) the k = min(pre_max, H*W*A) smallest keys of every frame
//   anchor_gather    the k selected anchors are decoded from the maps and the anchor TABLES (x / y shift tables per anchor
//                    set, centre z / size / rotation per anchor): no [H*W*A, 7] anchor tensor, no dense decode
//   nms mask + reduce   (nms.hip) rotated NMS of all frames
//   roi_compact      kept boxes / raw-logit scores / labels in kept order; the other slots as the reference leaves them
//                    (zeros, label 0 + 1 = 1)
// df3d_roi_decode_select -- RoIHeadTemplate.generate_predicted_boxes (roi_head_template.py:233-261) and the
// class-agnostic branch of post_processing for all frames: roi_decode (boxes, scores, keys), top-k select, roi_gather, NMS,
// final_compact.
#include <cstring>

#include "common.h"

// the reference's float expressions, evaluated operation by operation (no fused multiply-adds)
#pragma clang fp contract(off)
#include "anchor_box.h"

namespace df3d {

struct AnchorArgs {
  AnchorTab t;
  const float *cls, *box, *dir;
  int ld_cls, ld_box, ld_dir;
  int C, NB, k;
  float dir_offset, dir_limit_offset, period;
};

// float -> unsigned whose order is the float order (-0 counts as +0, like the comparison torch.topk makes)
__device__ __forceinline__ unsigned ordered_bits(float v) {
  v = v + 0.f;                                   // -0 + 0 = +0
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// max over the C logits of anchor a (first maximum wins like torch.max), label = its index
__device__ __forceinline__ void logit_label(const float *p, int C, float &score, int &label) {
  score = p[0];
  label = 0;
  for (int c = 1; c < C; ++c) {
    const float v = p[c];
    if (v > score) {
      score = v;
      label = c;
    }
  }
}

__global__ __launch_bounds__(256) void anchor_keys_kernel(AnchorArgs a, unsigned long long *__restrict__ keys) {
  const long long per_frame = (long long)a.t.H * a.t.W * a.t.A;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= per_frame * a.t.batch) return;
  const int b = (int)(i / per_frame);
  const int idx = (int)(i - (long long)b * per_frame);
  int pix, an;
  anchor_split(a.t, idx, pix, an);
  float score;
  int label;
  logit_label(a.cls + ((long long)b * a.t.H * a.t.W + pix) * a.ld_cls + an * a.C, a.C, score, label);
  const unsigned inv = ~ordered_bits(score);
  keys[i] = ((unsigned long long)b << 56) | ((unsigned long long)inv << ANCHOR_INDEX_BITS) | (unsigned)idx;
}

// grid (ceil(k / 256), batch)
__global__ __launch_bounds__(256) void anchor_gather_kernel(AnchorArgs a, const unsigned long long *__restrict__ keys,
                                                            float *__restrict__ cand_boxes, float *__restrict__ cand_scores,
                                                            int32_t *__restrict__ cand_labels) {
  const int b = blockIdx.y, r = blockIdx.x * 256 + threadIdx.x;
  if (r >= a.k) return;
  const size_t o = (size_t)b * a.k + r;
  const int idx = (int)(keys[o] & ((1ull << ANCHOR_INDEX_BITS) - 1));
  int pix, an;
  anchor_split(a.t, idx, pix, an);
  const long long row = (long long)b * a.t.H * a.t.W + pix;
  float score;
  int label;
  logit_label(a.cls + row * a.ld_cls + an * a.C, a.C, score, label);
  float xa, ya;
  const float *an5 = anchor_at(a.t, pix, an, xa, ya);
  float g[7];
  residual_decode(a.box + row * a.ld_box + an * 7, xa, ya, an5[0], an5[1], an5[2], an5[3], an5[4], g);
  if (a.dir) {                                        // anchor_head_template.py:254-265
    const float *d = a.dir + row * a.ld_dir + an * a.NB;
    float best = d[0];
    int lab = 0;
    for (int e = 1; e < a.NB; ++e)
      if (d[e] > best) {
        best = d[e];
        lab = e;
      }
    const float v = g[6] - a.dir_offset;
    const float rot = v - floorf(v / a.period + a.dir_limit_offset) * a.period;
    g[6] = rot + a.dir_offset + a.period * (float)lab;
  }
#pragma unroll
  for (int e = 0; e < 7; ++e) cand_boxes[o * 7 + e] = g[e];
  cand_scores[o] = score;
  cand_labels[o] = label;
}

// grid (batch): kept candidates into the first num[b] slots, the rest as the reference's new_zeros leaves them
__global__ __launch_bounds__(128) void roi_compact_kernel(const float *__restrict__ cand_boxes,
                                                          const float *__restrict__ cand_scores,
                                                          const int32_t *__restrict__ cand_labels,
                                                          const int32_t *__restrict__ keep, const int32_t *__restrict__ num_keep,
                                                          int cap, int post_max, float *__restrict__ out_boxes,
                                                          float *__restrict__ out_scores, long long *__restrict__ out_labels) {
  const int b = blockIdx.x;
  const int n = min(num_keep[b], post_max);
  for (int r = threadIdx.x; r < post_max; r += blockDim.x) {
    const size_t o = (size_t)b * post_max + r;
    if (r < n) {
      const size_t c = (size_t)b * cap + keep[(size_t)b * cap + r];
      for (int e = 0; e < 7; ++e) out_boxes[o * 7 + e] = cand_boxes[c * 7 + e];
      out_scores[o] = cand_scores[c];
      out_labels[o] = cand_labels[c] + 1;
    } else {
      for (int e = 0; e < 7; ++e) out_boxes[o * 7 + e] = 0.f;
      out_scores[o] = 0.f;
      out_labels[o] = 1;
    }
  }
}

struct ProposalPlan {
  size_t keys_in, keys_out, select, select_bytes, cand_boxes, cand_scores, cand_labels, keep, mask, mask_bytes, total;
  int k;
};

static void proposal_plan(int batch, long long per_frame, int pre_max, ProposalPlan &p) {
  WsLayout l;
  p.k = (int)(per_frame < pre_max ? per_frame : pre_max);
  const size_t S = (size_t)batch, k = (size_t)p.k;
  p.keys_in = l.take(S * per_frame * 8);
  p.keys_out = l.take(S * k * 8);
  p.select_bytes = topk_keys_workspace(batch, per_frame, p.k);
  p.select = l.take(p.select_bytes);
  p.cand_boxes = l.take(S * k * 7 * 4);
  p.cand_scores = l.take(S * k * 4);
  p.cand_labels = l.take(S * k * 4);
  p.keep = l.take(S * k * 4);
  p.mask_bytes = df3d_nms_bev_workspace_bytes(batch, p.k);
  p.mask = l.take(p.mask_bytes);
  p.total = l.total();
}

// ---- RoI decode and final selection ------------------------------------------------------------------------------------
struct RoiArgs {
  const float *rois, *cls, *reg;
  const long long *roi_labels;
  int ld_cls, ld_reg, batch, N, C, k, raw_score;
  float score_thr;
};

// one thread per RoI: batch_box_preds, and the selection key of its score.  The counts of the top-k select are the
// per-frame numbers of RoIs that pass the threshold.
__global__ __launch_bounds__(256) void roi_decode_kernel(RoiArgs a, float *__restrict__ box_preds,
                                                         unsigned long long *__restrict__ keys) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)a.batch * a.N) return;
  const int b = (int)(i / a.N), n = (int)(i - (long long)b * a.N);
  const float *roi = a.rois + i * 7;
  float g[7];
  residual_decode(a.reg + i * a.ld_reg, 0.f, 0.f, 0.f, roi[3], roi[4], roi[5], roi[6], g);   // local_rois[:, :, 0:3] = 0
  const float cosa = cosf(roi[6]), sina = sinf(roi[6]);                                      // rotate_points_along_z
  const float xr = g[0] * cosa + g[1] * -sina;
  const float yr = g[0] * sina + g[1] * cosa;
  g[0] = xr + roi[0];
  g[1] = yr + roi[1];
  g[2] = g[2] + roi[2];
#pragma unroll
  for (int e = 0; e < 7; ++e) box_preds[i * 7 + e] = g[e];
  const float *c = a.cls + i * a.ld_cls;
  float score = sigmoidf(c[0]);
  for (int e = 1; e < a.C; ++e) score = fmaxf(score, sigmoidf(c[e]));
  unsigned long long key = ~0ull;
  if (score >= a.score_thr)      // sigmoid scores lie in [0, 1]: descending score = ascending 0x3F800000 - bits
    key = ((unsigned long long)b << 56) | ((unsigned long long)(0x3F800000u - __float_as_uint(score)) << 24) | (unsigned)n;
  keys[i] = key;
}

// grid (ceil(k / 256), batch)
__global__ __launch_bounds__(256) void roi_gather_kernel(RoiArgs a, const unsigned long long *__restrict__ keys,
                                                         const int32_t *__restrict__ counts, const float *__restrict__ box_preds,
                                                         float *__restrict__ cand_boxes, int32_t *__restrict__ cand_index) {
  const int b = blockIdx.y, r = blockIdx.x * 256 + threadIdx.x;
  if (r >= counts[b]) return;
  const size_t o = (size_t)b * a.k + r;
  const int n = (int)(keys[o] & 0xFFFFFFull);
  const float *src = box_preds + ((size_t)b * a.N + n) * 7;
#pragma unroll
  for (int e = 0; e < 7; ++e) cand_boxes[o * 7 + e] = src[e];
  cand_index[o] = n;
}

// grid (batch)
__global__ __launch_bounds__(128) void final_compact_kernel(RoiArgs a, const float *__restrict__ box_preds,
                                                            const int32_t *__restrict__ cand_index,
                                                            const int32_t *__restrict__ keep, const int32_t *__restrict__ num_keep,
                                                            int post_max, float *__restrict__ out_boxes,
                                                            float *__restrict__ out_scores, long long *__restrict__ out_labels) {
  const int b = blockIdx.x;
  const int kept = min(num_keep[b], post_max);
  for (int r = threadIdx.x; r < post_max; r += blockDim.x) {
    const size_t o = (size_t)b * post_max + r;
    if (r < kept) {
      const int n = cand_index[(size_t)b * a.k + keep[(size_t)b * a.k + r]];
      const size_t i = (size_t)b * a.N + n;
      for (int e = 0; e < 7; ++e) out_boxes[o * 7 + e] = box_preds[i * 7 + e];
      float raw;
      int label;
      logit_label(a.cls + i * a.ld_cls, a.C, raw, label);          // sigmoid is monotonic: the arg-max of the logits
      float score = sigmoidf(a.cls[i * a.ld_cls]);
      for (int e = 1; e < a.C; ++e) score = fmaxf(score, sigmoidf(a.cls[i * a.ld_cls + e]));
      out_scores[o] = a.raw_score ? raw : score;
      out_labels[o] = a.roi_labels ? a.roi_labels[i] : (long long)(label + 1);
    } else {
      for (int e = 0; e < 7; ++e) out_boxes[o * 7 + e] = 0.f;
      out_scores[o] = 0.f;
      out_labels[o] = 0;
    }
  }
}

}  // namespace df3d

using namespace df3d;

extern "C" size_t df3d_anchor_proposals_workspace_bytes(const df3d_anchor_cfg *cfg) {
  if (!cfg || cfg->batch <= 0 || cfg->H <= 0 || cfg->W <= 0 || cfg->num_anchors <= 0 || cfg->pre_max <= 0 || cfg->pre_max > 4096)
    return 0;
  ProposalPlan p;
  proposal_plan(cfg->batch, (long long)cfg->H * cfg->W * cfg->num_anchors, cfg->pre_max, p);
  return p.total;
}

extern "C" int df3d_anchor_proposals(const float *cls, int ld_cls, const float *box, int ld_box, const float *dir, int ld_dir,
                                     const float *x_shifts, const float *y_shifts, const df3d_anchor_cfg *cfg, float *rois,
                                     float *roi_scores, long long *roi_labels, int32_t *num, void *workspace,
                                     size_t workspace_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  DF3D_CHECK_ARG(cfg, "anchor_proposals: null config");
  int rc = anchor_check(cfg, "anchor_proposals");
  if (rc) return rc;
  DF3D_CHECK_ARG(cfg->num_classes > 0 && cfg->num_dir_bins >= 0, "anchor_proposals: bad class / direction-bin count");
  DF3D_CHECK_ARG(cfg->pre_max > 0 && cfg->pre_max <= 4096, "anchor_proposals: 0 < NMS_PRE_MAXSIZE <= 4096 (got %d)",
                 cfg->pre_max);
  DF3D_CHECK_ARG(cfg->post_max > 0, "anchor_proposals: NMS_POST_MAXSIZE > 0");
  DF3D_CHECK_ARG(cls && box && x_shifts && y_shifts, "anchor_proposals: null input");
  DF3D_CHECK_ARG(rois && roi_scores && roi_labels && num && workspace, "anchor_proposals: null output");
  DF3D_CHECK_ARG(ld_cls >= cfg->num_anchors * cfg->num_classes && ld_box >= cfg->num_anchors * 7,
                 "anchor_proposals: a row stride is smaller than its channel count");
  DF3D_CHECK_ARG(!dir || (cfg->num_dir_bins > 0 && ld_dir >= cfg->num_anchors * cfg->num_dir_bins),
                 "anchor_proposals: direction map needs num_dir_bins > 0 and ld_dir >= anchors * bins");
  const long long per_frame = (long long)cfg->H * cfg->W * cfg->num_anchors;
  ProposalPlan p;
  proposal_plan(cfg->batch, per_frame, cfg->pre_max, p);
  DF3D_CHECK_ARG(workspace_bytes >= p.total, "anchor_proposals: workspace %zu < %zu bytes", workspace_bytes, p.total);

  AnchorArgs a;
  memset(&a, 0, sizeof(a));
  anchor_fill(a.t, cfg, x_shifts, y_shifts);
  a.cls = cls, a.box = box, a.dir = dir;
  a.ld_cls = ld_cls, a.ld_box = ld_box, a.ld_dir = ld_dir;
  a.C = cfg->num_classes, a.NB = cfg->num_dir_bins, a.k = p.k;
  a.dir_offset = cfg->dir_offset, a.dir_limit_offset = cfg->dir_limit_offset;
  a.period = cfg->num_dir_bins > 0 ? (float)(2.0 * 3.141592653589793 / cfg->num_dir_bins) : 0.f;

  char *ws = (char *)workspace;
  unsigned long long *kin = (unsigned long long *)(ws + p.keys_in), *kout = (unsigned long long *)(ws + p.keys_out);
  float *cb = (float *)(ws + p.cand_boxes), *cs = (float *)(ws + p.cand_scores);
  int32_t *cl = (int32_t *)(ws + p.cand_labels), *keep = (int32_t *)(ws + p.keep);
  hipLaunchKernelGGL(anchor_keys_kernel, dim3(cdiv(per_frame * cfg->batch, 256)), dim3(256), 0, stream, a, kin);
  DF3D_LAUNCH_CHECK();
  rc = topk_keys(kin, cfg->batch, per_frame, p.k, kout, nullptr, ws + p.select, p.select_bytes, stream);
  if (rc) return rc;
  hipLaunchKernelGGL(anchor_gather_kernel, dim3(cdiv(p.k, 256), cfg->batch), dim3(256), 0, stream, a, kout, cb, cs, cl);
  DF3D_LAUNCH_CHECK();
  rc = df3d_nms_bev(cb, nullptr, cfg->batch, p.k, cfg->nms_threshold, DF3D_NMS_ROTATED, cfg->post_max, keep, num, ws + p.mask,
                    p.mask_bytes, stream_);
  if (rc) return rc;
  hipLaunchKernelGGL(roi_compact_kernel, dim3(cfg->batch), dim3(128), 0, stream, cb, cs, cl, keep, num, p.k, cfg->post_max, rois,
                     roi_scores, roi_labels);
  DF3D_LAUNCH_CHECK();
  return DF3D_OK;
}

static int check_roi_cfg(const df3d_roi_decode_cfg *cfg) {
  DF3D_CHECK_ARG(cfg, "roi_decode_select: null config");
  DF3D_CHECK_ARG(cfg->batch > 0 && cfg->batch <= 255, "roi_decode_select: 1..255 frames");
  DF3D_CHECK_ARG(cfg->num_rois > 0 && cfg->num_rois <= 4096, "roi_decode_select: 0 < RoIs per frame <= 4096 (got %d)",
                 cfg->num_rois);
  DF3D_CHECK_ARG(cfg->num_classes > 0, "roi_decode_select: bad class count");
  DF3D_CHECK_ARG(cfg->pre_max > 0 && cfg->pre_max <= 4096, "roi_decode_select: 0 < NMS_PRE_MAXSIZE <= 4096 (got %d)",
                 cfg->pre_max);
  DF3D_CHECK_ARG(cfg->post_max > 0, "roi_decode_select: NMS_POST_MAXSIZE > 0");
  return DF3D_OK;
}

extern "C" size_t df3d_roi_decode_select_workspace_bytes(const df3d_roi_decode_cfg *cfg) {
  if (!cfg || cfg->batch <= 0 || cfg->num_rois <= 0 || cfg->num_rois > 4096 || cfg->pre_max <= 0 || cfg->pre_max > 4096) return 0;
  ProposalPlan p;
  proposal_plan(cfg->batch, cfg->num_rois, cfg->pre_max, p);
  return align_up(p.total, 256) + (size_t)cfg->batch * 4;
}

extern "C" int df3d_roi_decode_select(const float *rois, const float *rcnn_cls, int ld_cls, const float *rcnn_reg, int ld_reg,
                                      const long long *roi_labels, const df3d_roi_decode_cfg *cfg, float *box_preds,
                                      float *pred_boxes, float *pred_scores, long long *pred_labels, int32_t *counts,
                                      void *workspace, size_t workspace_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  int rc = check_roi_cfg(cfg);
  if (rc) return rc;
  DF3D_CHECK_ARG(rois && rcnn_cls && rcnn_reg, "roi_decode_select: null input");
  DF3D_CHECK_ARG(box_preds && pred_boxes && pred_scores && pred_labels && counts && workspace, "roi_decode_select: null output");
  DF3D_CHECK_ARG(ld_cls >= cfg->num_classes && ld_reg >= 7, "roi_decode_select: a row stride is smaller than its channel count");
  ProposalPlan p;
  proposal_plan(cfg->batch, cfg->num_rois, cfg->pre_max, p);
  const size_t cnt_off = align_up(p.total, 256);
  DF3D_CHECK_ARG(workspace_bytes >= cnt_off + (size_t)cfg->batch * 4, "roi_decode_select: workspace %zu < %zu bytes",
                 workspace_bytes, cnt_off + (size_t)cfg->batch * 4);
  RoiArgs a;
  memset(&a, 0, sizeof(a));
  a.rois = rois, a.cls = rcnn_cls, a.reg = rcnn_reg, a.roi_labels = roi_labels;
  a.ld_cls = ld_cls, a.ld_reg = ld_reg, a.batch = cfg->batch, a.N = cfg->num_rois, a.C = cfg->num_classes, a.k = p.k;
  a.raw_score = cfg->output_raw_score;
  a.score_thr = cfg->score_threshold;

  char *ws = (char *)workspace;
  unsigned long long *kin = (unsigned long long *)(ws + p.keys_in), *kout = (unsigned long long *)(ws + p.keys_out);
  float *cb = (float *)(ws + p.cand_boxes);
  int32_t *ci = (int32_t *)(ws + p.cand_labels), *keep = (int32_t *)(ws + p.keep), *cnt = (int32_t *)(ws + cnt_off);
  hipLaunchKernelGGL(roi_decode_kernel, dim3(cdiv((long long)cfg->batch * cfg->num_rois, 256)), dim3(256), 0, stream, a, box_preds,
                     kin);
  DF3D_LAUNCH_CHECK();
  rc = topk_keys(kin, cfg->batch, cfg->num_rois, p.k, kout, cnt, ws + p.select, p.select_bytes, stream);
  if (rc) return rc;
  hipLaunchKernelGGL(roi_gather_kernel, dim3(cdiv(p.k, 256), cfg->batch), dim3(256), 0, stream, a, kout, cnt, box_preds, cb, ci);
  DF3D_LAUNCH_CHECK();
  rc = df3d_nms_bev(cb, cnt, cfg->batch, p.k, cfg->nms_threshold, DF3D_NMS_ROTATED, cfg->post_max, keep, counts, ws + p.mask,
                    p.mask_bytes, stream_);
  if (rc) return rc;
  hipLaunchKernelGGL(final_compact_kernel, dim3(cfg->batch), dim3(128), 0, stream, a, box_preds, ci, keep, counts, cfg->post_max,
                     pred_boxes, pred_scores, pred_labels);
  DF3D_LAUNCH_CHECK();
  return DF3D_OK;
}
