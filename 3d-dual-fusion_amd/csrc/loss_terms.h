// Loss terms and the ordered reduction of the fused loss kernels: anchorloss.hip, roiloss.hip, pointhead.hip, and
// the reduction in tfloss.hip.  A term is the fp64 value and derivative of one element (the compiler drops what a caller does not
// use); the includer sets `#pragma clang fp contract(off)` in front of the include, as for bev_overlap.h.
// Reduction: every workgroup of 256 threads writes its J fp64 sums at partials[block * J + j]; ONE workgroup then adds them,
// thread t taking blocks t, t + 256, ... in turn, and block_sum256 adds the 256 accumulators of each j: a fixed order.
#pragma once
#include "common.h"

namespace df3d {

// bytes of the partials of `nblocks` workgroups: what the ..._workspace_bytes entries return and the run entries ask for
static inline size_t partials_bytes(int nblocks, int J) { return align_up((size_t)nblocks * J * sizeof(double), 256); }

__device__ __forceinline__ double sign_of(double d) { return d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0); }

// smooth L1 of difference d (WeightedSmoothL1Loss.smooth_l1_loss, loss_utils.py): plain L1 below beta = 1e-5
__device__ __forceinline__ void smooth_l1(double d, double beta, double &value, double &slope) {
  const double n = fabs(d);
  value = beta < 1e-5 ? n : (n < beta ? 0.5 * n * n / beta : n - 0.5 * beta);
  slope = beta >= 1e-5 && n < beta ? d / beta : sign_of(d);
}

// binary cross entropy of logit x against target, stable form; slope = sigmoid(x) - target
__device__ __forceinline__ void bce_with_logits(double x, double target, double &value, double &slope) {
  value = fmax(x, 0.0) - x * target + log1p(exp(-fabs(x)));
  slope = 1.0 / (1.0 + exp(-x)) - target;
}

// sigmoid focal loss (alpha 0.25, gamma 2) of one logit against target tt in {0, 1}: value and derivative
__device__ __forceinline__ void focal(double x, double tt, double &value, double &dx) {
  const double p = 1.0 / (1.0 + exp(-x));
  const double alpha_w = tt * 0.25 + (1.0 - tt) * 0.75;
  const double pt = tt * (1.0 - p) + (1.0 - tt) * p;
  double bce, dbce;
  bce_with_logits(x, tt, bce, dbce);
  value = alpha_w * pt * pt * bce;
  const double dpt = (1.0 - 2.0 * tt) * p * (1.0 - p);
  dx = alpha_w * (2.0 * pt * dpt * bce + pt * pt * dbce);
}

// max and sum of exp(q - max) of n logits: log-softmax of k is q[k] - (mx + log(sum)), softmax exp(q[k] - mx) / sum
__device__ __forceinline__ void softmax_stats(const float *q, int n, double &mx, double &sum) {
  mx = (double)q[0], sum = 0.0;
  for (int k = 1; k < n; ++k) mx = fmax(mx, (double)q[k]);
  for (int k = 0; k < n; ++k) sum += exp((double)q[k] - mx);
}

// the workgroup's sums of v[0..J) -> partials[blockIdx.x][J]; s_red: 4 doubles of LDS
template <int J>
__device__ __forceinline__ void partials_write(const double (&v)[J], double *__restrict__ partials, double *s_red) {
  for (int j = 0; j < J; ++j) {
    const double sum = block_sum256(v[j], s_red);
    if (threadIdx.x == 0) partials[(size_t)blockIdx.x * J + j] = sum;
  }
}

// by ONE workgroup: tot[j] = the sum over the blocks of partials[block][j], in every thread
template <int J>
__device__ __forceinline__ void partials_sum(const double *__restrict__ partials, int nblocks, double (&tot)[J], double *s_red) {
  double acc[J] = {};
  for (int k = threadIdx.x; k < nblocks; k += 256)
    for (int j = 0; j < J; ++j) acc[j] += partials[(size_t)k * J + j];
  for (int j = 0; j < J; ++j) tot[j] = block_sum256(acc[j], s_red);
}

}  // namespace df3d
