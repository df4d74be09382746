// What follows the summation in every training-mode BatchNorm of this library, written once: the
// 64-lane fold of (sum, sum) partials, the statistics -> coefficients step, and the backward's
// per-channel terms.  Each caller keeps its own summation (bn.hip's shifted partials, the
// synchronised norm's all-reduced moments, mlp.hip's LDS tree and X4 covariance, pwconv.hip's Chan
// merge); once a channel's n, mean and var are known, all of them finish HERE, so every route
// rounds the same way: fused_mlp.py mixes the routes inside one chain and the float64 pins compare
// them with each other.  The library builds with -ffp-contract=off: an expression rounds the same
// inlined from here as written out in place, as long as its order of operations is kept.
//
// The two per-channel records:
//   coef[c*4 + {0,1,2,3}] = scale, bias, mean, invstd          (forward: y = x * scale + bias)
//   bnb[c*8 + {0..7}]     = scale, bias, a, mean, d1, e0, -, - (the norm backward fused into the
//                           weight gradient, pwconv_wgrad.hip: a = gamma invstd,
//                           d1 = a invstd k2, e0 = -a k1 with k1, k2 of bn_bwd_terms)
#pragma once
#include "common.h"

namespace nesie {

template <typename T> struct FoldPair { T x, y; };   // one slot, loaded whole (T = float or double)

// s0, s1 = sums over i < nslice of partial[(c * nslice + i) * 2 + {0, 1}], in double, by ONE wave
// (threadIdx.x < 64): lane t adds slots t, t + 64, ... in that order -- four loads in flight while
// there are that many -- then wave_sum's butterfly.  Every lane of the wave gets the sums.
template <typename T>
__device__ __forceinline__ void fold_pairs(const T *__restrict__ partial, int c, int nslice,
                                           double &s0, double &s1) {
  const FoldPair<T> *pc = (const FoldPair<T> *)partial + (size_t)c * nslice;
  s0 = 0.0; s1 = 0.0;
  int i = threadIdx.x;
  for (; i + 192 < nslice; i += 256) {
    FoldPair<T> q[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) q[u] = pc[i + 64 * u];
#pragma unroll
    for (int u = 0; u < 4; ++u) { s0 += (double)q[u].x; s1 += (double)q[u].y; }
  }
  for (; i < nslice; i += 64) {
    const FoldPair<T> q = pc[i];
    s0 += (double)q.x;
    s1 += (double)q.y;
  }
  s0 = wave_sum(s0);
  s1 = wave_sum(s1);
}

// Where the statistics -> coefficients step reads its parameters and leaves its results.  Every
// pointer but coef may be NULL: gamma / beta default to 1 / 0, running_mean and running_var come
// as a pair.  The fields after coef are what the callers differ in.
struct BnTail {
  const float *gamma, *beta;
  float *running_mean, *running_var;
  float momentum, eps;
  float *coef;                                    // [C][4], layout above
  float *save_mean = nullptr, *save_invstd = nullptr;   // the same mean / invstd as plain vectors
  // bias of the convolution in front of the norm.  The layer kernel never adds it (the mean
  // subtraction removes it from every normalised value): it shifts the running mean, nothing else
  const float *chan_bias = nullptr;
  // running_var takes var itself, as the reference's NaiveSyncBatchNorm does
  // (mmdet3d/ops/norm.py:68-71), not var * n / (n - 1)
  bool biased_running_var = false;
};

// Channel c from its count, mean and biased variance (clamped at 0 here): -> (scale, bias, mean,
// invstd), for every caller.  Only a `writer` touches memory: the running statistics, coef and
// save_*.  (bn_apply_kernel: every block of a channel needs scale / bias, one of them writes.)
__device__ __forceinline__ float4 bn_coef_finish(const BnTail &t, int c, double n, double mean,
                                                 double var, bool writer = true) {
  if (var < 0.0) var = 0.0;
  const double invstd = 1.0 / sqrt(var + (double)t.eps);
  const double g = t.gamma ? (double)t.gamma[c] : 1.0, bt = t.beta ? (double)t.beta[c] : 0.0;
  const float4 q = make_float4((float)(g * invstd), (float)(bt - mean * g * invstd), (float)mean,
                               (float)invstd);
  if (!writer) return q;
  if (t.running_mean) {
    const double shown = t.chan_bias ? mean + (double)t.chan_bias[c] : mean;
    t.running_mean[c] = (float)((1.0 - t.momentum) * t.running_mean[c] + t.momentum * shown);
    const double unbiased = !t.biased_running_var && n > 1.0 ? var * n / (n - 1.0) : var;
    t.running_var[c] = (float)((1.0 - t.momentum) * t.running_var[c] + t.momentum * unbiased);
  }
  if (t.save_mean) t.save_mean[c] = q.z;
  if (t.save_invstd) t.save_invstd[c] = q.w;
  t.coef[c * 4 + 0] = q.x;
  t.coef[c * 4 + 1] = q.y;
  t.coef[c * 4 + 2] = q.z;
  t.coef[c * 4 + 3] = q.w;
  return q;
}

// The backward's per-channel terms from s0 = sum(g), s1 = sum(g xhat) over the channel's n
// positions: dx = a (g - k1 - xhat k2).  A `writer` also leaves dbeta = s0, dgamma = s1 (either
// may be NULL).
struct BnBwdTerms { float a, k1, k2; };   // gamma invstd, sum(g) / n, sum(g xhat) / n
__device__ __forceinline__ BnBwdTerms bn_bwd_terms(double s0, double s1, double n, const float *gamma,
                                                   float invstd, int c, float *dgamma, float *dbeta,
                                                   bool writer = true) {
  if (writer) {
    if (dbeta) dbeta[c] = (float)s0;
    if (dgamma) dgamma[c] = (float)s1;
  }
  return {(float)((gamma ? (double)gamma[c] : 1.0) * (double)invstd), (float)(s0 / n), (float)(s1 / n)};
}

}  // namespace nesie
