// l2o_conv_bn.h -- the fixed-order per-channel reductions of batch normalisation that the conv-net optimizees share
// (l2o_mnist_conv.h, l2o_cifar_conv.h, l2o_lenet.h, l2o_nas.h): per-sample (mean, M2) and backward sums, their merge over
// the minibatch, and the factored conv-bias gradient.  Workgroups of kCvThreads threads; device functions only, no kernel.
// BN variance: per-sample (mean, M2) merged as M2 = sum M2_s + n sum (mean_s - mean)^2 (never E[z^2] - E[z]^2).
#pragma once
#include "l2o_params.h"

namespace l2o {

constexpr int kCvThreads = 256;
constexpr float kCvEps = 1e-3f;

// Per-channel sums of v[pos * C + c] over npos positions: lane l of channel c takes pos = l, l + L, ... (L = 256 / C) in
// order, then the L lane sums in lane order.  Returns the sum to threads tid < C (others: 0).
template <int C>
__device__ float cv_chan_sum(const float* v, int npos, float* red) {
  constexpr int L = kCvThreads / C;
  const int tid = threadIdx.x, c = tid % C, l = tid / C;
  float s = 0.0f;
  for (int p = l; p < npos; p += L) s += v[p * C + c];
  red[tid] = s;
  __syncthreads();
  float t = 0.0f;
  if (tid < C)
    for (int k = 0; k < L; ++k) t += red[k * C + c];
  __syncthreads();
  return t;
}

// (mean, M2) of one sample's channels, two passes over the LDS-resident values; written to part[c][2].
template <int C>
__device__ void cv_sample_stats(const float* v, int npos, float* red, float* mean_sh, float* part) {
  const int tid = threadIdx.x;
  const float s = cv_chan_sum<C>(v, npos, red);
  if (tid < C) mean_sh[tid] = s / (float)npos;
  __syncthreads();
  constexpr int L = kCvThreads / C;
  const int c = tid % C, l = tid / C;
  const float m = mean_sh[c];
  float q = 0.0f;
  for (int p = l; p < npos; p += L) {
    const float d = v[p * C + c] - m;
    q = __builtin_fmaf(d, d, q);
  }
  red[tid] = q;
  __syncthreads();
  if (tid < C) {
    float t = 0.0f;
    for (int k = 0; k < L; ++k) t += red[k * C + c];
    part[2 * tid] = mean_sh[tid];
    part[2 * tid + 1] = t;
  }
  __syncthreads();
}

// BN statistics of the minibatch from the per-sample (mean, M2) partials part[s][C][2] (n positions per sample), the same
// fixed order in every workgroup: mean -> mean_sh[C], 1 / sqrt(var + eps) -> rstd_sh[C].
template <int C>
__device__ void cv_merge_stats(const float* part, int B, float n, float* red, float* mean_sh, float* rstd_sh) {
  constexpr int L = kCvThreads / C;
  const int tid = threadIdx.x, c = tid % C, l = tid / C;
  float s = 0.0f;
  for (int b = l; b < B; b += L) s += part[(b * C + c) * 2];
  red[tid] = s;
  __syncthreads();
  if (tid < C) {
    float t = 0.0f;
    for (int k = 0; k < L; ++k) t += red[k * C + c];
    mean_sh[tid] = t / (float)B;
  }
  __syncthreads();
  const float m = mean_sh[c];
  float q = 0.0f;
  for (int b = l; b < B; b += L) {
    const float d = part[(b * C + c) * 2] - m;
    q += __builtin_fmaf(n * d, d, part[(b * C + c) * 2 + 1]);
  }
  red[tid] = q;
  __syncthreads();
  if (tid < C) {
    float t = 0.0f;
    for (int k = 0; k < L; ++k) t += red[k * C + c];
    rstd_sh[tid] = 1.0f / sqrtf(t / (n * (float)B) + kCvEps);
  }
  __syncthreads();
}

// Means over the minibatch of the per-sample sums part[s][C][2] (n positions per sample): -> a_sh[C], b_sh[C].
template <int C>
__device__ void cv_merge_means(const float* part, int B, float n, float* red, float* a_sh, float* b_sh) {
  constexpr int L = kCvThreads / C;
  const int tid = threadIdx.x, c = tid % C, l = tid / C;
  for (int j = 0; j < 2; ++j) {
    float s = 0.0f;
    for (int b = l; b < B; b += L) s += part[(b * C + c) * 2 + j];
    red[tid] = s;
    __syncthreads();
    if (tid < C) {
      float t = 0.0f;
      for (int k = 0; k < L; ++k) t += red[k * C + c];
      (j == 0 ? a_sh : b_sh)[tid] = t / (n * (float)B);
    }
    __syncthreads();
  }
}

// Per-sample (sum dy, sum dy * xhat) of one layer: dy[pos * C + c] in LDS, z from `z` (same layout), BN stats in LDS.
template <int C>
__device__ void cv_sample_bwd_sums(const float* dy, const float* z, int npos, const float* mean_sh, const float* rstd_sh,
                                   float* red, float* part) {
  constexpr int L = kCvThreads / C;
  const int tid = threadIdx.x, c = tid % C, l = tid / C;
  const float m = mean_sh[c], r = rstd_sh[c];
  float s0 = 0.0f, s1 = 0.0f;
  for (int p = l; p < npos; p += L) {
    const float d = dy[p * C + c];
    s0 += d;
    s1 = __builtin_fmaf(d, (z[p * C + c] - m) * r, s1);
  }
  red[tid] = s0;
  __syncthreads();
  if (tid < C) {
    float t = 0.0f;
    for (int k = 0; k < L; ++k) t += red[k * C + c];
    part[2 * tid] = t;
  }
  __syncthreads();
  red[tid] = s1;
  __syncthreads();
  if (tid < C) {
    float t = 0.0f;
    for (int k = 0; k < L; ++k) t += red[k * C + c];
    part[2 * tid + 1] = t;
  }
  __syncthreads();
}

// A conv bias followed by batch norm: sum_i dz_i = gamma rstd (sum dy - N mean(dy) - mean(dy xhat) sum xhat) with
// sum xhat = n rstd sum_s (mean_s - mean) -- zero in exact arithmetic (batch norm removes any per-channel shift).  Summing
// the N = n B values dz_i themselves leaves O(sqrt(N) eps |dz|) of noise; this factored form leaves O(eps |sum dy|).
__device__ float cv_bn_bias_grad(const float* st, const float* bw, const float* mean, const float* rstd, const float* gamma,
                                 int C, int c, int B, float n) {
  float sdy = 0.0f, sdx = 0.0f, sx = 0.0f;
  for (int s = 0; s < B; ++s) {
    sdy += bw[(s * C + c) * 2];
    sdx += bw[(s * C + c) * 2 + 1];
    sx += st[(s * C + c) * 2] - mean[c];
  }
  const float N = n * (float)B, r = rstd[c];
  return gamma[c] * r * ((sdy - N * (sdy / N)) - (sdx / N) * (n * r * sx));
}

}  // namespace l2o
