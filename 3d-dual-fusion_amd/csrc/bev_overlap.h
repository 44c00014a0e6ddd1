// Overlap area of two rotated BEV boxes by polygon clipping, shared by nms.hip and tfloss.hip.
//
// Both reference kernels (CP/det3d/ops/iou3d_nms/src/iou3d_nms_kernel.cu:36-245 and TF/mmdet3d/ops/iou3d/src/
// iou3d_kernel.cu:56-258) run the same clipping: crossings of the 4 x 4 edges, the corners of one box inside the other,
// the reference's bubble sort by atan2f about the centroid, a triangle fan.  They differ in the box layout and in the
// containment margin; a unit supplies both as a policy
//     struct Box { static void corners(const float *box, BevPt *c);      // c[0..3] and c[4] = c[0]
//                  static bool contains(const float *box, BevPt p); };
// The arithmetic is float, operation for operation the reference's: the includer sets `#pragma clang fp contract(off)`
// in front of the include (a file-scope pragma here would run on into the rest of the includer).
//
// roiloss.hip runs the same clipping in double (bev_overlap<Box, double>, a policy on BevPtT<double>): the scalar type is
// a template parameter that defaults to float, and the float instantiation is the code above, operation for operation.
#pragma once
#include "common.h"

namespace df3d {

template <class T>
struct BevPtT {
  T x, y;
};
using BevPt = BevPtT<float>;

__device__ __forceinline__ float bev_min(float a, float b) { return fminf(a, b); }
__device__ __forceinline__ float bev_max(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ float bev_abs(float a) { return fabsf(a); }
__device__ __forceinline__ float bev_atan2(float y, float x) { return atan2f(y, x); }
__device__ __forceinline__ double bev_min(double a, double b) { return fmin(a, b); }
__device__ __forceinline__ double bev_max(double a, double b) { return fmax(a, b); }
__device__ __forceinline__ double bev_abs(double a) { return fabs(a); }
__device__ __forceinline__ double bev_atan2(double y, double x) { return atan2(y, x); }

template <class T>
__device__ __forceinline__ T bev_cross3(BevPtT<T> p1, BevPtT<T> p2, BevPtT<T> p0) {
  return (p1.x - p0.x) * (p2.y - p0.y) - (p2.x - p0.x) * (p1.y - p0.y);
}

template <class T>
__device__ __forceinline__ bool bev_rect_cross(BevPtT<T> p1, BevPtT<T> p2, BevPtT<T> q1, BevPtT<T> q2) {
  return bev_min(p1.x, p2.x) <= bev_max(q1.x, q2.x) && bev_min(q1.x, q2.x) <= bev_max(p1.x, p2.x) &&
         bev_min(p1.y, p2.y) <= bev_max(q1.y, q2.y) && bev_min(q1.y, q2.y) <= bev_max(p1.y, p2.y);
}

template <class T>
__device__ __forceinline__ bool bev_intersection(BevPtT<T> p1, BevPtT<T> p0, BevPtT<T> q1, BevPtT<T> q0, BevPtT<T> &ans) {
  if (!bev_rect_cross(p0, p1, q0, q1)) return false;
  const T s1 = bev_cross3(q0, p1, p0), s2 = bev_cross3(p1, q1, p0);
  const T s3 = bev_cross3(p0, q1, q0), s4 = bev_cross3(q1, p1, q0);
  if (!(s1 * s2 > 0 && s3 * s4 > 0)) return false;
  const T s5 = bev_cross3(q1, p1, p0);
  if (bev_abs(s5 - s1) > (T)1e-8f) {
    ans.x = (s5 * q0.x - s1 * q1.x) / (s5 - s1);
    ans.y = (s5 * q0.y - s1 * q1.y) / (s5 - s1);
  } else {
    const T a0 = p0.y - p1.y, b0 = p1.x - p0.x, c0 = p0.x * p1.y - p1.x * p0.y;
    const T a1 = q0.y - q1.y, b1 = q1.x - q0.x, c1 = q0.x * q1.y - q1.x * q0.y;
    const T D = a0 * b1 - a1 * b0;
    ans.x = (b0 * c1 - b1 * c0) / D;
    ans.y = (a1 * c0 - a0 * c1) / D;
  }
  return true;
}

template <class Box, class T = float>
__device__ T bev_overlap(const float *a, const float *b) {
  typedef BevPtT<T> BevPt;
  BevPt ca[5], cb[5], pts[16], ctr = {(T)0.f, (T)0.f};
  int cnt = 0;
  Box::corners(a, ca);
  Box::corners(b, cb);
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      BevPt x;
      if (bev_intersection(ca[i + 1], ca[i], cb[j + 1], cb[j], x)) {
        pts[cnt] = x;
        ctr.x += x.x;
        ctr.y += x.y;
        cnt++;
      }
    }
  for (int k = 0; k < 4; ++k) {
    if (Box::contains(a, cb[k])) {
      ctr.x += cb[k].x;
      ctr.y += cb[k].y;
      pts[cnt++] = cb[k];
    }
    if (Box::contains(b, ca[k])) {
      ctr.x += ca[k].x;
      ctr.y += ca[k].y;
      pts[cnt++] = ca[k];
    }
  }
  if (cnt < 3) return (T)0.f;                 // the reference's fan over fewer than three vertices is empty as well
  ctr.x /= cnt;
  ctr.y /= cnt;
  T ang[16];
  for (int i = 0; i < cnt; ++i) ang[i] = bev_atan2(pts[i].y - ctr.y, pts[i].x - ctr.x);
  for (int j = 0; j < cnt - 1; ++j)        // the reference's bubble sort (same swaps: the keys do not change)
    for (int i = 0; i < cnt - j - 1; ++i)
      if (ang[i] > ang[i + 1]) {
        const BevPt t = pts[i];
        pts[i] = pts[i + 1];
        pts[i + 1] = t;
        const T u = ang[i];
        ang[i] = ang[i + 1];
        ang[i + 1] = u;
      }
  T area = (T)0.f;
  for (int k = 0; k < cnt - 1; ++k) {
    const T ax = pts[k].x - pts[0].x, ay = pts[k].y - pts[0].y;
    const T bx = pts[k + 1].x - pts[0].x, by = pts[k + 1].y - pts[0].y;
    area += ax * by - ay * bx;
  }
  return bev_abs(area) / (T)2.0f;
}

}  // namespace df3d
