// PV-RCNN keypoint segmentation head: points in boxes, the point targets and the point loss on the device.
//
// Reference: VR/pcdet/models/dense_heads/point_head_template.py:49-129 (assign_stack_targets) loops over frames on the host:
// per frame a boolean-mask compaction whose size is read back, points_in_boxes_gpu twice (the boxes and the boxes enlarged by
// GT_EXTRA_WIDTH; VR/pcdet/ops/roiaware_pool3d/src/roiaware_pool3d_kernel.cu:16-36, 313-336) and a scatter back;
// get_cls_layer_loss (:131-155) builds a one-hot tensor and a weights tensor and reads two scalars back.
//
// df3d_points_in_boxes      one thread per point, the boxes of the frame staged in LDS 128 at a time with cos / sin of the
//                           heading computed once per box; the first box that holds the point
// df3d_point_head_targets   one launch for all frames: one thread per row of `points`; a workgroup walks the frames its rows
//                           name (one frame when the rows are stacked frame after frame) and stages that frame's ground truth
//                           in the same chunks; ONE rotation per (point, box) serves the plain and the enlarged test
// df3d_point_cls_loss       one thread per point: the focal terms of its classes (loss_terms.h), fp64 partials of the sum and
//                           of the positive count per workgroup at fixed positions, the un-normalised derivative of every
//                           logit stored; a one-workgroup ordered finish writes loss and pos_num (bit-identical run to run)
// df3d_point_cls_loss_grad  the stored derivatives times upstream * weight / max(pos_num, 1), both scalars read on the device
#include <climits>

#include "common.h"

// the reference's float expressions, evaluated operation by operation (no fused multiply-adds)
#pragma clang fp contract(off)
#include "loss_terms.h"

namespace df3d {

constexpr int PH_CHUNK = DF3D_POINT_HEAD_GT_CHUNK;

// rows of `stride` floats (x, y, z, dx, dy, dz, heading, ..) -> s_box[k] = (cx, cy, cz, dx, dy, dz, cos(-rz), sin(-rz)): the
// rotation of lidar_to_local_coords in float32, once per box instead of once per pair.  n <= PH_CHUNK <= 256 threads.
__device__ __forceinline__ void stage_boxes(const float *__restrict__ rows, int stride, int n, float (*s_box)[8]) {
  const int k = threadIdx.x;
  if (k < n) {
    const float *g = rows + (size_t)k * stride;
    float *o = s_box[k];
    o[0] = g[0], o[1] = g[1], o[2] = g[2], o[3] = g[3], o[4] = g[4], o[5] = g[5];
    const float a = -g[6];
    o[6] = cosf(a), o[7] = sinf(a);
  }
}

// check_pt_in_box3d (roiaware_pool3d_kernel.cu:23-36) of one staged box: bit 0 = inside the box, bit 1 (EXT only) = inside the
// box whose sizes are dx + ex, dy + ey, dz + ez, added in float32 as enlarge_box3d does on float32 tensors.  The z test is
// `fabsf(z - cz) > dz / 2.0` -> outside (strict: a point on the face is inside; NaN is not outside); the xy tests compare in
// double against `d / 2.0 + MARGIN` with MARGIN the float 1e-5.
template <bool EXT>
__device__ __forceinline__ int box_test(float x, float y, float z, const float *b, float ex, float ey, float ez) {
  const double margin = (double)1e-5f;
  const float az = fabsf(z - b[2]);
  const bool z_in = !((double)az > (double)b[5] / 2.0);
  float edx = 0.f, edy = 0.f, edz = 0.f;
  bool z_ext = false;
  if (EXT) {
    edx = b[3] + ex, edy = b[4] + ey, edz = b[5] + ez;
    z_ext = !((double)az > (double)edz / 2.0);
  }
  if (!z_in && !z_ext) return 0;
  const float sx = x - b[0], sy = y - b[1];
  const float lx = sx * b[6] + sy * (-b[7]);
  const float ly = sx * b[7] + sy * b[6];
  const double ax = (double)fabsf(lx), ay = (double)fabsf(ly);
  int r = 0;
  if (z_in && ax < (double)b[3] / 2.0 + margin && ay < (double)b[4] / 2.0 + margin) r |= 1;
  if (EXT && z_ext && ax < (double)edx / 2.0 + margin && ay < (double)edy / 2.0 + margin) r |= 2;
  return r;
}

// grid (ceil(npts / 256), B)
__global__ __launch_bounds__(256) void points_in_boxes_kernel(const float *__restrict__ boxes, const float *__restrict__ pts, int N,
                                                              int npts, int32_t *__restrict__ out) {
  __shared__ float s_box[PH_CHUNK][8];
  const int b = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool live = i < npts;
  float x = 0.f, y = 0.f, z = 0.f;
  if (live) {
    const float *p = pts + ((size_t)b * npts + i) * 3;
    x = p[0], y = p[1], z = p[2];
  }
  int idx = -1;
  for (int c0 = 0; c0 < N; c0 += PH_CHUNK) {
    const int n = min(PH_CHUNK, N - c0);
    stage_boxes(boxes + ((size_t)b * N + c0) * 7, 7, n, s_box);
    __syncthreads();
    if (live && idx < 0)
      for (int k = 0; k < n; ++k)
        if (box_test<false>(x, y, z, s_box[k], 0.f, 0.f, 0.f) & 1) {
          idx = c0 + k;
          break;
        }
    if (__syncthreads_and(!live || idx >= 0)) break;                // (also the barrier in front of the next chunk)
  }
  if (live) out[(size_t)b * npts + i] = idx;
}

struct TargetArgs {
  const float *points;                    // [P][4]: frame, x, y, z
  const float *gt;                        // [B][G][8]
  long long P;
  int B, G, num_class;
  float ex, ey, ez;
  int64_t *labels;                        // [P]
  int32_t *box_idx;                       // [P] or null
};

// grid (ceil(P / 256))
__global__ __launch_bounds__(256) void point_head_targets_kernel(TargetArgs a) {
  __shared__ float s_box[PH_CHUNK][8];
  __shared__ int s_lo, s_hi;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool live = i < a.P;
  int frame = -1;                                                   // a row of no frame 0..B-1 keeps label 0 (`bs_idx == k`)
  float x = 0.f, y = 0.f, z = 0.f;
  if (live) {
    const float *p = a.points + i * 4;
    const float bf = p[0];
    if (bf >= 0.f && bf < (float)a.B) {
      const int t = (int)bf;
      if ((float)t == bf) frame = t;
    }
    x = p[1], y = p[2], z = p[3];
  }
  if (threadIdx.x == 0) s_lo = INT_MAX, s_hi = -1;
  __syncthreads();
  if (frame >= 0) {
    atomicMin(&s_lo, frame);
    atomicMax(&s_hi, frame);
  }
  __syncthreads();
  const int lo = s_lo, hi = s_hi;
  bool fg = false, ext = false;
  int idx = -1;
  for (int f = lo; f <= hi; ++f) {
    const bool mine = frame == f;
    if (!__syncthreads_or(mine)) continue;                          // uniform: no row of this workgroup names frame f
    // a row is done at the first box that holds it: the reference writes the class AFTER the ignore flag, so a foreground
    // row keeps its class whatever the enlarged boxes say (they differ only under a negative extra width)
    bool done = !mine;
    for (int c0 = 0; c0 < a.G; c0 += PH_CHUNK) {
      const int n = min(PH_CHUNK, a.G - c0);
      stage_boxes(a.gt + ((size_t)f * a.G + c0) * 8, 8, n, s_box);
      __syncthreads();
      if (!done)
        for (int k = 0; k < n; ++k) {
          const int r = box_test<true>(x, y, z, s_box[k], a.ex, a.ey, a.ez);
          if (r & 2) ext = true;
          if (r & 1) {
            fg = done = true, idx = c0 + k;
            break;
          }
        }
      if (__syncthreads_and(done)) break;                           // (also the barrier in front of the next chunk)
    }
  }
  if (!live) return;
  long long label = 0;                                              // point_cls_labels_single[ignore_flag] = -1, then [fg_flag] = class
  if (fg)
    label = a.num_class == 1 ? 1 : (long long)a.gt[((size_t)frame * a.G + idx) * 8 + 7];
  else if (ext)
    label = -1;
  a.labels[i] = label;
  if (a.box_idx) a.box_idx[i] = idx;
}

// grid (ceil(P / 256)): partials[block][2] (focal sum, positives), dlogit[P][C]
__global__ __launch_bounds__(256) void point_cls_loss_kernel(const float *__restrict__ preds, int ld, const int64_t *__restrict__ labels,
                                                             long long P, int C, double *__restrict__ partials,
                                                             double *__restrict__ dlogit) {
  __shared__ double s_red[4];
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  double sum = 0.0, pos = 0.0;
  if (i < P) {
    const long long label = labels[i];
    pos = label > 0 ? 1.0 : 0.0;
    const float *c = preds + i * ld;
    for (int k = 0; k < C; ++k) {
      double v = 0.0, dv = 0.0;
      if (label >= 0) {
        focal((double)c[k], label == k + 1 ? 1.0 : 0.0, v, dv);
        sum += v;
      }
      dlogit[i * C + k] = dv;
    }
  }
  const double v[2] = {sum, pos};
  partials_write<2>(v, partials, s_red);
}

// one workgroup: loss = weight * sum / max(positives, 1), pos_num = positives
__global__ __launch_bounds__(256) void point_cls_loss_final_kernel(const double *__restrict__ partials, int nblocks, double weight,
                                                                   float *__restrict__ loss, float *__restrict__ pos_num) {
  __shared__ double s_red[4];
  double tot[2];
  partials_sum<2>(partials, nblocks, tot, s_red);
  if (threadIdx.x == 0) {
    loss[0] = (float)(weight * tot[0] / fmax(tot[1], 1.0));
    pos_num[0] = (float)tot[1];
  }
}

// grid (ceil(P * C / 256))
__global__ __launch_bounds__(256) void point_cls_loss_grad_kernel(const double *__restrict__ dlogit, const float *__restrict__ pos_num,
                                                                  const float *__restrict__ upstream, long long total, int C,
                                                                  double weight, float *__restrict__ grad, int ld_grad) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const double scale = (double)upstream[0] * weight / fmax((double)pos_num[0], 1.0);
  const long long i = e / C;
  const int k = (int)(e - i * C);
  grad[i * ld_grad + k] = (float)(dlogit[e] * scale);
}

}  // namespace df3d

using namespace df3d;

// what one launch can index: rows, and 256-thread workgroups in grid.x
static const long long PH_MAX_POINTS = 1LL << 24;

extern "C" int df3d_points_in_boxes(const float *boxes, const float *pts, int batch, int num_boxes, int num_pts,
                                    int32_t *box_idx_of_points, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  DF3D_CHECK_ARG(batch >= 0 && batch <= 65535 && num_boxes >= 0 && num_pts >= 0, "points_in_boxes: 0..65535 frames, counts >= 0 "
                 "(got B = %d, N = %d, npts = %d)", batch, num_boxes, num_pts);
  if (batch == 0 || num_pts == 0) return DF3D_OK;
  DF3D_CHECK_ARG(pts && box_idx_of_points && (boxes || num_boxes == 0), "points_in_boxes: null pointer");
  hipLaunchKernelGGL(points_in_boxes_kernel, dim3(cdiv(num_pts, 256), batch), dim3(256), 0, stream, boxes, pts, num_boxes, num_pts,
                     box_idx_of_points);
  DF3D_LAUNCH_CHECK();
  return DF3D_OK;
}

extern "C" int df3d_point_head_targets(const float *points, long long num_points, const float *gt_boxes, int batch, int max_gt,
                                       const float *extra_width, int num_class, int64_t *labels, int32_t *box_idx, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  DF3D_CHECK_ARG(num_points >= 0 && num_points <= PH_MAX_POINTS, "point_head_targets: 0..%lld points (got %lld)", PH_MAX_POINTS,
                 num_points);
  DF3D_CHECK_ARG(batch >= 0 && num_class >= 1, "point_head_targets: batch >= 0 and num_class >= 1 (got %d, %d)", batch, num_class);
  DF3D_CHECK_ARG(max_gt >= 0 && max_gt <= DF3D_POINT_HEAD_MAX_GT, "point_head_targets: 0..%d ground-truth rows per frame (got G = %d)",
                 DF3D_POINT_HEAD_MAX_GT, max_gt);
  DF3D_CHECK_ARG(extra_width, "point_head_targets: null extra_width");
  if (num_points == 0) return DF3D_OK;
  DF3D_CHECK_ARG(points && labels && (gt_boxes || max_gt == 0 || batch == 0), "point_head_targets: null pointer");
  TargetArgs a;
  a.points = points, a.gt = gt_boxes, a.P = num_points, a.B = batch, a.G = max_gt, a.num_class = num_class;
  a.ex = extra_width[0], a.ey = extra_width[1], a.ez = extra_width[2];
  a.labels = labels, a.box_idx = box_idx;
  hipLaunchKernelGGL(point_head_targets_kernel, dim3(cdiv(num_points, 256)), dim3(256), 0, stream, a);
  DF3D_LAUNCH_CHECK();
  return DF3D_OK;
}

extern "C" size_t df3d_point_cls_loss_workspace_bytes(long long num_points) {
  if (num_points < 0 || num_points > PH_MAX_POINTS) return 0;
  return partials_bytes(cdiv(num_points > 0 ? num_points : 1, 256), 2);
}

extern "C" int df3d_point_cls_loss(const float *preds, int ld, const int64_t *labels, long long num_points, int num_class,
                                   float weight, float *loss, float *pos_num, double *dlogit, void *workspace,
                                   size_t workspace_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  DF3D_CHECK_ARG(num_points >= 0 && num_points <= PH_MAX_POINTS, "point_cls_loss: 0..%lld points (got %lld)", PH_MAX_POINTS,
                 num_points);
  DF3D_CHECK_ARG(num_class >= 1 && num_class <= 64 && ld >= num_class, "point_cls_loss: 1..64 classes and ld >= num_class (got %d, ld %d)",
                 num_class, ld);
  DF3D_CHECK_ARG(loss && pos_num && workspace, "point_cls_loss: null output");
  DF3D_CHECK_ARG(num_points == 0 || (preds && labels && dlogit), "point_cls_loss: null input");
  const int nblocks = cdiv(num_points > 0 ? num_points : 1, 256);
  const size_t need = partials_bytes(nblocks, 2);
  DF3D_CHECK_ARG(workspace_bytes >= need, "point_cls_loss: workspace %zu < %zu bytes", workspace_bytes, need);
  double *partials = (double *)workspace;
  hipLaunchKernelGGL(point_cls_loss_kernel, dim3(nblocks), dim3(256), 0, stream, preds, ld, labels, num_points, num_class, partials,
                     dlogit);
  DF3D_LAUNCH_CHECK();
  hipLaunchKernelGGL(point_cls_loss_final_kernel, dim3(1), dim3(256), 0, stream, partials, nblocks, (double)weight, loss, pos_num);
  DF3D_LAUNCH_CHECK();
  return DF3D_OK;
}

extern "C" int df3d_point_cls_loss_grad(const double *dlogit, const float *pos_num, const float *upstream, long long num_points,
                                        int num_class, float weight, float *grad, int ld_grad, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  DF3D_CHECK_ARG(num_points >= 0 && num_points <= PH_MAX_POINTS, "point_cls_loss_grad: 0..%lld points (got %lld)", PH_MAX_POINTS,
                 num_points);
  DF3D_CHECK_ARG(num_class >= 1 && num_class <= 64 && ld_grad >= num_class,
                 "point_cls_loss_grad: 1..64 classes and ld_grad >= num_class (got %d, ld %d)", num_class, ld_grad);
  if (num_points == 0) return DF3D_OK;
  DF3D_CHECK_ARG(dlogit && pos_num && upstream && grad, "point_cls_loss_grad: null pointer");
  const long long total = num_points * num_class;
  hipLaunchKernelGGL(point_cls_loss_grad_kernel, dim3(cdiv(total, 256)), dim3(256), 0, stream, dlogit, pos_num, upstream, total,
                     num_class, (double)weight, grad, ld_grad);
  DF3D_LAUNCH_CHECK();
  return DF3D_OK;
}
