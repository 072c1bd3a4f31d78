// l2o_lenet.h -- forward + gradient of problems.LeNet (DM/problems.py:461-537; DM/util.py:176-184 "lenet"):
// conv 5x5x3x6 VALID (32x32 -> 28x28) -> [BN] -> sigmoid -> max-pool 2x2 (14x14) -> conv 5x5x6x16 VALID (10x10) -> [BN] ->
// sigmoid -> max-pool 2x2 (5x5x16) -> flatten NHWC (400) -> linear 400x120 -> [BN over the minibatch] -> sigmoid -> linear
// 120x84 -> [BN] -> sigmoid -> linear 84x10 -> mean sparse softmax cross-entropy.  BN = snt.BatchNorm in training mode:
// batch statistics, biased variance, eps 1e-3, an offset beta and NO scale.  NHWC activations, HWIO / [in, out] weights.
// The step-granular evaluation l2o_lenet_fg; the conv half calls the cv_* reductions of l2o_conv_bn.h
// (256 threads); included by l2o_nets.hip; written for gfx950 only.
//
// sigmoid is strictly increasing, so the pools take the maximum of the normalised pre-activation (first maximum of the
// window in row-major order) and one sigmoid is applied per pooled output.
//
// Twelve launches per evaluation, fp32 VALU -- except the batch mean of a linear layer and the sum of its centred values,
// which are accumulated in double (ln_lane_sum_d; ln_fc_body says why) -- every reduction in a fixed order (no atomics:
// bit-reproducible):
//   k_ln_conv1    one workgroup per sample: conv1 (+ bias); the sample's per-channel (mean, M2) of z1
//   k_ln_conv2    one workgroup per sample: BN1 statistics merged from the per-sample partials (every workgroup the same
//                 way; workgroup 0 keeps them), normalise, pool with argmax, sigmoid, conv2; the sample's (mean, M2) of z2
//   k_ln_pool2    one workgroup per sample: BN2 statistics merged, normalise, pool with argmax, sigmoid -> f [400]
//   k_ln_fc       (twice) a workgroup owns kLnU output units of a linear layer for ALL samples: the [B x K] . [K x U]
//                 product, the units' batch statistics (two passes over the LDS-resident column, the mean kept as
//                 hi + lo floats), normalise, sigmoid
//   k_ln_out      16 samples per workgroup: linear 84x10, cross-entropy, dL/dlogits
//   k_ln_fcb      (twice, layer 2 then 1) a workgroup owns kLnU units for all samples: dL/dy from the layer above
//                 (dz_up . W_up^T) times the sigmoid's derivative, BN backward with the units' own sums (sum dy,
//                 sum dy xhat) -> dz, the beta / bias gradients, and dW[:, units] = in^T . dz as a [K x B] . [B x U]
//                 product, one thread per input row, the samples in order
//   k_ln_mid      one workgroup per sample: dL/df = dz_fc1 . W0^T, pool-2 / sigmoid backward -> dL/dy2 and the sample's
//                 (sum dy2, sum dy2 xhat2)
//   k_ln_mid2     one workgroup per sample: BN2 backward -> dz2, the sample's share of dW2 / db2, conv2 input gradient,
//                 pool-1 / sigmoid backward -> dL/dy1 and the sample's (sum dy1, sum dy1 xhat1)
//   k_ln_first    one workgroup per sample: BN1 backward -> dz1, the sample's share of dW1 / db1
//   k_ln_grad     the minibatch sums in sample order, one thread per coordinate: dW1 / dW2 and the conv biases from the
//                 per-sample shares (under batch norm the biases in the factored form cv_bn_bias_grad, gamma = 1), the
//                 conv betas, the last linear layer; thread 0 the mean loss
// Forward only (g == NULL): the first six and the loss sum.
#pragma once
#include "l2o_conv_bn.h"

namespace l2o {

constexpr int kLnThreads = kCvThreads;    // the cv_* helpers assume 256 threads
constexpr int kLnMaxBatch = 1024;
constexpr int kLnImg = 32 * 32 * 3;       // 3072, HWC
constexpr int kLnC1 = 6, kLnC2 = 16, kLnOut = 10;
constexpr int kLnH1 = 28, kLnQ1 = 14, kLnH2 = 10, kLnQ2 = 5;
constexpr int kLnP1 = kLnH1 * kLnH1, kLnP2 = kLnH2 * kLnH2;            // 784, 100
constexpr int kLnZ1 = kLnP1 * kLnC1;      // 4704: z1, and dL/dy1
constexpr int kLnA1 = kLnQ1 * kLnQ1 * kLnC1;                          // 1176: pooled layer-1 output / its argmax
constexpr int kLnZ2 = kLnP2 * kLnC2;      // 1600: z2, dL/dy2, dz2
constexpr int kLnF = kLnQ2 * kLnQ2 * kLnC2;                           // 400: flattened pool-2 output
constexpr int kLnN1 = 120, kLnN2 = 84;
constexpr int kLnNW1 = 5 * 5 * 3 * kLnC1, kLnNW2 = 5 * 5 * kLnC1 * kLnC2;   // 450, 2400
constexpr int kLnPW1 = kLnNW1 + kLnC1, kLnPW2 = kLnNW2 + kLnC2;      // a sample's dW + db share
constexpr int kLnU = 4;                   // output units of a linear layer per workgroup
constexpr int kLnLanes = kLnThreads / kLnU;                           // 64 sample lanes
constexpr int kLnOutSamples = kLnThreads / 16;                        // 16
// stat: conv mean1[8] rstd1[8] mean2[16] rstd2[16] ones[16]; then (mean, rstd, the mean's low part, -) of linear_0
// [120][4], linear_1 [84][4]
constexpr int kLnStM1 = 0, kLnStR1 = 8, kLnStM2 = 16, kLnStR2 = 32, kLnStOne = 48, kLnStF1 = 64, kLnStF2 = kLnStF1 + 4 * kLnN1;
constexpr int kLnStat = kLnStF2 + 4 * kLnN2;                          // 880

struct LenetArgs {
  int batch, bn, want_grad;
  const float* images;                    // [n_data, 3072]
  const int* labels;
  const int* idx;                         // [batch]
  const float *w1, *b1, *be1, *w2, *b2, *be2, *wl0, *bl0, *bel0, *wl1, *bl1, *bel1, *wl2, *bl2;
  float *gw1, *gb1, *gbe1, *gw2, *gb2, *gbe2, *gwl0, *gbl0, *gbel0, *gwl1, *gbl1, *gbel1, *gwl2, *gbl2;
  // scratch
  float* z1;      // [batch][784][6]
  float* d1;      // [batch][784][6]    dL/dy1 (BN) or dL/dz1
  float* p1;      // [batch][196][6]    pooled layer-1 output (after the sigmoid)
  int* am1;       // [batch][196][6]    argmax (0..3) of each pool-1 window
  float* z2;      // [batch][100][16]
  float* d2;      // [batch][100][16]   dL/dy2 (BN) or dL/dz2
  float* f;       // [batch][400]       pooled layer-2 output (after the sigmoid), NHWC-flattened
  int* am2;       // [batch][400]
  float* h1;      // [batch][120]       linear_0 output
  float* a1;      // [batch][120]       after BN / sigmoid
  float* dh1;     // [batch][120]       dL/dh1
  float* h2;      // [batch][84]
  float* a2;      // [batch][84]
  float* dh2;     // [batch][84]
  float* dlog;    // [batch][16]        dL/dlogits
  float* loss_s;  // [batch]
  float* st1;     // [batch][6][2]      (mean, M2) of z1 per sample
  float* bw1;     // [batch][6][2]      (sum dy1, sum dy1 xhat1)
  float* st2;     // [batch][16][2]
  float* bw2;     // [batch][16][2]
  float* pw1;     // [batch][456]
  float* pw2;     // [batch][2416]
  float* stat;    // [kLnStat]
  float* loss;    // [1]
};

__device__ __forceinline__ float ln_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

__global__ __launch_bounds__(kLnThreads) void k_ln_conv1(LenetArgs a) {
  __shared__ float img[kLnImg];
  __shared__ __attribute__((aligned(16))) float w[kLnNW1 + 2];
  __shared__ float z[kLnZ1];
  __shared__ float red[kLnThreads];
  __shared__ float msh[8];
  const int s = blockIdx.x, tid = threadIdx.x;
  const float4* src = reinterpret_cast<const float4*>(a.images + (size_t)a.idx[s] * kLnImg);
  for (int k = tid; k < kLnImg / 4; k += kLnThreads) reinterpret_cast<float4*>(img)[k] = src[k];
  for (int k = tid; k < kLnNW1; k += kLnThreads) w[k] = a.w1[k];
  if (s == 0 && tid < 16) a.stat[kLnStOne + tid] = 1.0f;
  __syncthreads();
  float* zo = a.z1 + (size_t)s * kLnZ1;
  // one thread per output position, all 6 channels: a tap's three input values meet 18 weights
  for (int pos = tid; pos < kLnP1; pos += kLnThreads) {
    const int oy = pos / kLnH1, ox = pos - oy * kLnH1;
    const float* ip = img + (oy * 32 + ox) * 3;
    float acc[kLnC1];
#pragma unroll
    for (int c = 0; c < kLnC1; ++c) acc[c] = 0.0f;
    for (int ky = 0; ky < 5; ++ky)
#pragma unroll
      for (int kx = 0; kx < 5; ++kx)
#pragma unroll
        for (int ci = 0; ci < 3; ++ci) {
          const float v = ip[(ky * 32 + kx) * 3 + ci];
          const float* wr = w + ((ky * 5 + kx) * 3 + ci) * kLnC1;
#pragma unroll
          for (int c = 0; c < kLnC1; ++c) acc[c] = __builtin_fmaf(v, wr[c], acc[c]);
        }
#pragma unroll
    for (int c = 0; c < kLnC1; ++c) {
      const float v = acc[c] + a.b1[c];
      z[pos * kLnC1 + c] = v;
      zo[pos * kLnC1 + c] = v;
    }
  }
  __syncthreads();
  if (a.bn) cv_sample_stats<kLnC1>(z, kLnP1, red, msh, a.st1 + (size_t)s * kLnC1 * 2);
}

__global__ __launch_bounds__(kLnThreads) void k_ln_conv2(LenetArgs a) {
  __shared__ __attribute__((aligned(16))) float p1[kLnA1];
  __shared__ __attribute__((aligned(16))) float w[kLnNW2];
  __shared__ float z[kLnZ2];
  __shared__ float red[kLnThreads];
  __shared__ float mean1[8], rstd1[8], msh[kLnC2];
  const int s = blockIdx.x, tid = threadIdx.x;
  if (a.bn) {
    cv_merge_stats<kLnC1>(a.st1, a.batch, (float)kLnP1, red, mean1, rstd1);
    if (s == 0 && tid < kLnC1) { a.stat[kLnStM1 + tid] = mean1[tid]; a.stat[kLnStR1 + tid] = rstd1[tid]; }
  }
  for (int k = tid; k < kLnNW2; k += kLnThreads) w[k] = a.w2[k];
  // BN1 -> 2x2 max-pool (the first maximum of the window in row-major order) -> sigmoid
  const float* zi = a.z1 + (size_t)s * kLnZ1;
  int* am = a.am1 + (size_t)s * kLnA1;
  float* po = a.p1 + (size_t)s * kLnA1;
  for (int o = tid; o < kLnA1; o += kLnThreads) {
    const int pos = o / kLnC1, c = o - pos * kLnC1, py = pos / kLnQ1, px = pos - py * kLnQ1;
    float best = 0.0f;
    int arg = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float v = zi[((2 * py + (q >> 1)) * kLnH1 + 2 * px + (q & 1)) * kLnC1 + c];
      if (a.bn) v = (v - mean1[c]) * rstd1[c] + a.be1[c];
      if (q == 0 || v > best) { best = v; arg = q; }
    }
    const float y = ln_sigmoid(best);
    p1[o] = y;
    po[o] = y;
    am[o] = arg;
  }
  __syncthreads();
  // conv2: thread = (output position, half of the 16 output channels)
  if (tid < 2 * kLnP2) {
    const int pos = tid >> 1, h = tid & 1, oy = pos / kLnH2, ox = pos - oy * kLnH2;
    const float* pb = p1 + (oy * kLnQ1 + ox) * kLnC1;
    const float* wb = w + 8 * h;
    float acc[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[c] = 0.0f;
    for (int ky = 0; ky < 5; ++ky)
#pragma unroll
      for (int kx = 0; kx < 5; ++kx)
#pragma unroll
        for (int ci = 0; ci < kLnC1; ++ci) {
          const float v = pb[(ky * kLnQ1 + kx) * kLnC1 + ci];
          const float* wr = wb + ((ky * 5 + kx) * kLnC1 + ci) * kLnC2;
#pragma unroll
          for (int c = 0; c < 8; ++c) acc[c] = __builtin_fmaf(v, wr[c], acc[c]);
        }
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const float v = acc[c] + a.b2[8 * h + c];
      z[pos * kLnC2 + 8 * h + c] = v;
      a.z2[(size_t)s * kLnZ2 + pos * kLnC2 + 8 * h + c] = v;
    }
  }
  __syncthreads();
  if (a.bn) cv_sample_stats<kLnC2>(z, kLnP2, red, msh, a.st2 + (size_t)s * kLnC2 * 2);
}

__global__ __launch_bounds__(kLnThreads) void k_ln_pool2(LenetArgs a) {
  __shared__ float red[kLnThreads];
  __shared__ float mean2[kLnC2], rstd2[kLnC2];
  const int s = blockIdx.x, tid = threadIdx.x;
  if (a.bn) {
    cv_merge_stats<kLnC2>(a.st2, a.batch, (float)kLnP2, red, mean2, rstd2);
    if (s == 0 && tid < kLnC2) { a.stat[kLnStM2 + tid] = mean2[tid]; a.stat[kLnStR2 + tid] = rstd2[tid]; }
  }
  const float* zi = a.z2 + (size_t)s * kLnZ2;
  for (int o = tid; o < kLnF; o += kLnThreads) {
    const int c = o & 15, pos = o >> 4, py = pos / kLnQ2, px = pos - py * kLnQ2;
    float best = 0.0f;
    int arg = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float v = zi[((2 * py + (q >> 1)) * kLnH2 + 2 * px + (q & 1)) * kLnC2 + c];
      if (a.bn) v = (v - mean2[c]) * rstd2[c] + a.be2[c];
      if (q == 0 || v > best) { best = v; arg = q; }
    }
    a.f[(size_t)s * kLnF + o] = ln_sigmoid(best);
    a.am2[(size_t)s * kLnF + o] = arg;
  }
}

// Sum of v over this unit's sample lanes: the 64 lane values in lane order.  Returns the sum to every thread of unit u.
__device__ float ln_lane_sum(float v, float* red) {
  const int tid = threadIdx.x, u = tid & (kLnU - 1);
  red[tid] = v;
  __syncthreads();
  float t = 0.0f;
  for (int k = 0; k < kLnLanes; ++k) t += red[k * kLnU + u];
  __syncthreads();
  return t;
}

// The same sum in double (the batch mean of a linear layer and the sum of the centred values, see ln_fc_body).
__device__ double ln_lane_sum_d(double v, double* red) {
  const int tid = threadIdx.x, u = tid & (kLnU - 1);
  red[tid] = v;
  __syncthreads();
  double t = 0.0;
  for (int k = 0; k < kLnLanes; ++k) t += red[k * kLnU + u];
  __syncthreads();
  return t;
}

// A linear layer + [BN over the minibatch] + sigmoid for kLnU output units and every sample.  Thread = (unit u, sample
// lane l): samples l, l + 64, ... four at a time, the K terms of a dot product in order.
// The batch mean is kept as two floats (hi + lo, from a double sum over the samples) and every centred value is
// (z - hi) - lo: with one float, the mean's own rounding (up to half an ulp, times the B samples) is what the centred
// values fail to sum to zero by, and that residue is the whole of the gradient of the bias in front of the batch norm
// (measured: 2.6e-6 of the layer's largest dW entry with a float mean, against the 1e-6 the project holds).
template <int K, int N>
__device__ void ln_fc_body(const LenetArgs& a, const float* in, const float* W, const float* b, const float* beta, float* h,
                           float* act, float* st) {
  static_assert(K % 4 == 0 && N % kLnU == 0, "k_ln_fc tiling");
  __shared__ float wt[K * kLnU];
  __shared__ float zt[kLnMaxBatch * kLnU];
  __shared__ double red[kLnThreads];
  const int tid = threadIdx.x, u = tid & (kLnU - 1), l = tid >> 2, u0 = blockIdx.x * kLnU, B = a.batch;
  for (int k = tid; k < K * kLnU; k += kLnThreads) wt[k] = W[(k >> 2) * N + u0 + (k & 3)];
  __syncthreads();
  const float bias = b[u0 + u];
  for (int sb = 0; sb < B; sb += 4 * kLnLanes) {
    const float4* row[4];
    float acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      row[j] = reinterpret_cast<const float4*>(in + (size_t)min(sb + l + kLnLanes * j, B - 1) * K);
      acc[j] = 0.0f;
    }
#pragma unroll 2
    for (int k4 = 0; k4 < K / 4; ++k4) {
      const float w0 = wt[(4 * k4) * kLnU + u], w1 = wt[(4 * k4 + 1) * kLnU + u], w2 = wt[(4 * k4 + 2) * kLnU + u],
                  w3 = wt[(4 * k4 + 3) * kLnU + u];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float4 x = row[j][k4];
        acc[j] = __builtin_fmaf(x.x, w0, acc[j]);
        acc[j] = __builtin_fmaf(x.y, w1, acc[j]);
        acc[j] = __builtin_fmaf(x.z, w2, acc[j]);
        acc[j] = __builtin_fmaf(x.w, w3, acc[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int s = sb + l + kLnLanes * j;
      if (s < B) {
        const float v = acc[j] + bias;
        zt[s * kLnU + u] = v;
        h[(size_t)s * N + u0 + u] = v;
      }
    }
  }
  __syncthreads();
  float mean = 0.0f, mlo = 0.0f, rstd = 1.0f, be = 0.0f;
  if (a.bn) {
    double t = 0.0;
    for (int s = l; s < B; s += kLnLanes) t += (double)zt[s * kLnU + u];
    const double md = ln_lane_sum_d(t, red) / (double)B;
    mean = (float)md;
    mlo = (float)(md - (double)mean);
    double q = 0.0;
    for (int s = l; s < B; s += kLnLanes) {
      const float d = (zt[s * kLnU + u] - mean) - mlo;
      q += (double)(d * d);
    }
    rstd = 1.0f / sqrtf((float)(ln_lane_sum_d(q, red) / (double)B) + kCvEps);
    be = beta[u0 + u];
    if (l == 0) { st[4 * (u0 + u)] = mean; st[4 * (u0 + u) + 1] = rstd; st[4 * (u0 + u) + 2] = mlo; }
  }
  for (int s = l; s < B; s += kLnLanes)
    act[(size_t)s * N + u0 + u] = ln_sigmoid(((zt[s * kLnU + u] - mean) - mlo) * rstd + be);
}

template <int LAYER>
__global__ __launch_bounds__(kLnThreads) void k_ln_fc(LenetArgs a) {
  if (LAYER == 0) ln_fc_body<kLnF, kLnN1>(a, a.f, a.wl0, a.bl0, a.bel0, a.h1, a.a1, a.stat + kLnStF1);
  else ln_fc_body<kLnN1, kLnN2>(a, a.a1, a.wl1, a.bl1, a.bel1, a.h2, a.a2, a.stat + kLnStF2);
}

__global__ __launch_bounds__(kLnThreads) void k_ln_out(LenetArgs a) {
  __shared__ float w[kLnN2 * kLnOut];
  __shared__ float lg[kLnOutSamples][16];
  const int tid = threadIdx.x, o = tid & 15, ls = tid >> 4, s = blockIdx.x * kLnOutSamples + ls;
  const bool live = s < a.batch;
  for (int k = tid; k < kLnN2 * kLnOut; k += kLnThreads) w[k] = a.wl2[k];
  __syncthreads();
  if (live && o < kLnOut) {
    const float* x = a.a2 + (size_t)s * kLnN2;
    float t = 0.0f;
#pragma unroll 4
    for (int k = 0; k < kLnN2; ++k) t = __builtin_fmaf(x[k], w[k * kLnOut + o], t);
    lg[ls][o] = t + a.bl2[o];
  }
  __syncthreads();
  if (live && o == 0) {
    const int lab = a.labels[a.idx[s]];
    float rmax = lg[ls][0];
    for (int k = 1; k < kLnOut; ++k) rmax = fmaxf(rmax, lg[ls][k]);
    float se = 0.0f;
    for (int k = 0; k < kLnOut; ++k) se += expf(lg[ls][k] - rmax);
    const float lse = rmax + logf(se), invB = 1.0f / (float)a.batch;
    a.loss_s[s] = lse - lg[ls][lab];
    if (a.want_grad)
      for (int k = 0; k < 16; ++k)
        a.dlog[(size_t)s * 16 + k] = k < kLnOut ? (expf(lg[ls][k] - lse) - (k == lab ? 1.0f : 0.0f)) * invB : 0.0f;
  }
}

// Backward of a linear layer + [BN] + sigmoid for kLnU of its N output units and every sample.  dzup [B][SUP] is dL/d(the
// NUP pre-activations of the layer above), Wup [N][NUP] that layer's weights; in [B][K] this layer's input.
template <int K, int N, int NUP, int SUP>
__device__ void ln_fcb_body(const LenetArgs& a, const float* in, const float* h, const float* act, const float* st,
                            const float* dzup, const float* Wup, float* dh, float* gW, float* gb, float* gbeta) {
  __shared__ float wu[kLnU * NUP];
  __shared__ __attribute__((aligned(16))) float dzs[kLnMaxBatch * kLnU];
  __shared__ float red[kLnThreads];
  __shared__ double redd[kLnThreads];
  const int tid = threadIdx.x, u = tid & (kLnU - 1), l = tid >> 2, u0 = blockIdx.x * kLnU, B = a.batch;
  for (int k = tid; k < kLnU * NUP; k += kLnThreads) wu[k] = Wup[(size_t)u0 * NUP + k];
  __syncthreads();
  float mean = 0.0f, mlo = 0.0f, rstd = 1.0f;
  if (a.bn) { mean = st[4 * (u0 + u)]; rstd = st[4 * (u0 + u) + 1]; mlo = st[4 * (u0 + u) + 2]; }
  // dL/dy = (dz_up . W_up[unit, :]) sigmoid'(y); this lane's part of (sum dy, sum dy xhat) and, in double, of the sum of
  // the centred values (z - mean): what the xhat used below fail to sum to zero by
  float s0 = 0.0f, s1 = 0.0f;
  double s2 = 0.0;
  for (int s = l; s < B; s += kLnLanes) {
    const float* dr = dzup + (size_t)s * SUP;
    float t = 0.0f;
#pragma unroll 4
    for (int n = 0; n < NUP; ++n) t = __builtin_fmaf(dr[n], wu[u * NUP + n], t);
    const float y = act[(size_t)s * N + u0 + u], dy = t * (y * (1.0f - y));
    dzs[s * kLnU + u] = dy;
    if (a.bn) {
      const float d = (h[(size_t)s * N + u0 + u] - mean) - mlo;
      s0 += dy;
      s1 = __builtin_fmaf(dy, d * rstd, s1);
      s2 += (double)d;
    }
  }
  __syncthreads();
  if (a.bn) {
    const float fB = (float)B;
    const float sdy = ln_lane_sum(s0, red), sdx = ln_lane_sum(s1, red), sx = (float)ln_lane_sum_d(s2, redd);
    const float ma = sdy / fB, mb = sdx / fB;
    for (int s = l; s < B; s += kLnLanes) {
      const float xh = ((h[(size_t)s * N + u0 + u] - mean) - mlo) * rstd;
      dzs[s * kLnU + u] = rstd * (dzs[s * kLnU + u] - ma - xh * mb);
    }
    if (l == 0) {
      gbeta[u0 + u] = sdy;
      // the bias feeds the batch norm: 0 in exact arithmetic; the factored form of cv_bn_bias_grad with n = 1, gamma = 1
      gb[u0 + u] = rstd * ((sdy - fB * (sdy / fB)) - (sdx / fB) * (rstd * sx));
    }
  } else {
    float t = 0.0f;
    for (int s = l; s < B; s += kLnLanes) t += dzs[s * kLnU + u];
    t = ln_lane_sum(t, red);
    if (l == 0) gb[u0 + u] = t;
  }
  __syncthreads();
  for (int s = l; s < B; s += kLnLanes) dh[(size_t)s * N + u0 + u] = dzs[s * kLnU + u];
  // dW[k, units] = sum_s in[s, k] dz[s, units]: one thread per input row k, the samples in order, 16 loads in flight
  for (int k = tid; k < K; k += kLnThreads) {
    float acc[kLnU];
#pragma unroll
    for (int j = 0; j < kLnU; ++j) acc[j] = 0.0f;
    const float* ip = in + k;
#pragma unroll 16
    for (int s = 0; s < B; ++s) {
      const float x = ip[(size_t)s * K];
      const float4 d = reinterpret_cast<const float4*>(dzs)[s];
      acc[0] = __builtin_fmaf(x, d.x, acc[0]);
      acc[1] = __builtin_fmaf(x, d.y, acc[1]);
      acc[2] = __builtin_fmaf(x, d.z, acc[2]);
      acc[3] = __builtin_fmaf(x, d.w, acc[3]);
    }
#pragma unroll
    for (int j = 0; j < kLnU; ++j) gW[(size_t)k * N + u0 + j] = acc[j];
  }
}

template <int LAYER>
__global__ __launch_bounds__(kLnThreads) void k_ln_fcb(LenetArgs a) {
  if (LAYER == 1)
    ln_fcb_body<kLnN1, kLnN2, kLnOut, 16>(a, a.a1, a.h2, a.a2, a.stat + kLnStF2, a.dlog, a.wl2, a.dh2, a.gwl1, a.gbl1, a.gbel1);
  else
    ln_fcb_body<kLnF, kLnN1, kLnN2, kLnN2>(a, a.f, a.h1, a.a1, a.stat + kLnStF1, a.dh2, a.wl1, a.dh1, a.gwl0, a.gbl0, a.gbel0);
}

__global__ __launch_bounds__(kLnThreads) void k_ln_mid(LenetArgs a) {
  __shared__ float dh[kLnN1];
  __shared__ float d2s[kLnZ2];
  __shared__ float wtile[32 * (kLnN1 + 1)];
  __shared__ float runs[8][32];
  __shared__ float red[kLnThreads];
  __shared__ float mean2[kLnC2], rstd2[kLnC2];
  const int s = blockIdx.x, tid = threadIdx.x;
  if (tid < kLnN1) dh[tid] = a.dh1[(size_t)s * kLnN1 + tid];
  if (tid < kLnC2) { mean2[tid] = a.bn ? a.stat[kLnStM2 + tid] : 0.0f; rstd2[tid] = a.bn ? a.stat[kLnStR2 + tid] : 1.0f; }
  for (int o = tid; o < kLnZ2; o += kLnThreads) d2s[o] = 0.0f;
  __syncthreads();
  // dL/df[j] = sum_n dh1[n] W0[j, n] -> sigmoid' -> the argmax of the pool-2 window.  32 rows of W0 at a time through LDS
  // (rows padded to 121 floats); thread = (row, one of 8 runs of 15 terms), the 8 run sums added in run order
  for (int t0 = 0; t0 < kLnF; t0 += 32) {
    const int rows = min(32, kLnF - t0);
    for (int k = tid; k < rows * kLnN1; k += kLnThreads) {
      const int r = k / kLnN1;
      wtile[r * (kLnN1 + 1) + (k - r * kLnN1)] = a.wl0[(size_t)t0 * kLnN1 + k];
    }
    __syncthreads();
    {
      const int ol = tid & 31, run = tid >> 5;
      float t = 0.0f;
      if (ol < rows) {
        const float* wr = wtile + ol * (kLnN1 + 1) + run * 15;
#pragma unroll
        for (int n = 0; n < 15; ++n) t = __builtin_fmaf(dh[run * 15 + n], wr[n], t);
      }
      runs[run][ol] = t;
    }
    __syncthreads();
    if (tid < rows) {
      float t = runs[0][tid];
      for (int k = 1; k < 8; ++k) t += runs[k][tid];
      const int o = t0 + tid, c = o & 15, pos = o >> 4, py = pos / kLnQ2, px = pos - py * kLnQ2;
      const int q = a.am2[(size_t)s * kLnF + o];
      const float y = a.f[(size_t)s * kLnF + o];
      d2s[((2 * py + (q >> 1)) * kLnH2 + 2 * px + (q & 1)) * kLnC2 + c] = t * (y * (1.0f - y));
    }
  }
  __syncthreads();
  float* d2 = a.d2 + (size_t)s * kLnZ2;
  for (int o = tid; o < kLnZ2; o += kLnThreads) d2[o] = d2s[o];
  if (a.bn)
    cv_sample_bwd_sums<kLnC2>(d2s, a.z2 + (size_t)s * kLnZ2, kLnP2, mean2, rstd2, red, a.bw2 + (size_t)s * kLnC2 * 2);
}

__global__ __launch_bounds__(kLnThreads) void k_ln_mid2(LenetArgs a) {
  // LDS: W2 [ky][kx][ci][co] and the sample's pooled layer-1 output while dW2's share and the conv2 input gradient are
  // formed, then the sample's [784][6] dL/dy1 in the same space
  constexpr int kPool = kLnZ1;
  static_assert(kLnNW2 + kLnA1 <= kPool, "k_ln_mid2 LDS carve-up");
  __shared__ __attribute__((aligned(16))) float pool[kPool];
  __shared__ __attribute__((aligned(16))) float dzs[kLnZ2];
  __shared__ float red[kLnThreads];
  __shared__ float ma[kLnC2], mb[kLnC2], mean1[8], rstd1[8];
  const int s = blockIdx.x, tid = threadIdx.x;
  float* ws = pool;
  float* p1 = pool + kLnNW2;
  if (a.bn) {
    cv_merge_means<kLnC2>(a.bw2, a.batch, (float)kLnP2, red, ma, mb);
    if (tid < kLnC1) { mean1[tid] = a.stat[kLnStM1 + tid]; rstd1[tid] = a.stat[kLnStR1 + tid]; }
  }
  for (int o = tid; o < kLnZ2; o += kLnThreads) {
    const int c = o & 15;
    float v = a.d2[(size_t)s * kLnZ2 + o];
    if (a.bn) {
      const float r = a.stat[kLnStR2 + c], xh = (a.z2[(size_t)s * kLnZ2 + o] - a.stat[kLnStM2 + c]) * r;
      v = r * (v - ma[c] - xh * mb[c]);
    }
    dzs[o] = v;
  }
  for (int o = tid; o < kLnNW2; o += kLnThreads) ws[o] = a.w2[o];
  for (int o = tid; o < kLnA1; o += kLnThreads) p1[o] = a.p1[(size_t)s * kLnA1 + o];
  __syncthreads();
  // this sample's dW2[ky, kx, ci, co] = sum_pos p1[pos + (ky, kx), ci] dz2[pos, co]: thread = (ky, kx, ci, 4 co);
  // db2[co] = sum_pos dz2[pos, co]
  float* pw = a.pw2 + (size_t)s * kLnPW2;
  for (int it = tid; it < kLnNW2 / 4 + kLnC2; it += kLnThreads) {
    if (it < kLnNW2 / 4) {
      const int cq = it & 3, r = it >> 2, ci = r % kLnC1, kk = r / kLnC1, ky = kk / 5, kx = kk - ky * 5;
      const float* pb = p1 + (ky * kLnQ1 + kx) * kLnC1 + ci;
      float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      for (int oy = 0; oy < kLnH2; ++oy)
#pragma unroll
        for (int ox = 0; ox < kLnH2; ++ox) {
          const float x = pb[(oy * kLnQ1 + ox) * kLnC1];
          const float4 d = reinterpret_cast<const float4*>(dzs)[(oy * kLnH2 + ox) * 4 + cq];
          acc.x = __builtin_fmaf(x, d.x, acc.x);
          acc.y = __builtin_fmaf(x, d.y, acc.y);
          acc.z = __builtin_fmaf(x, d.z, acc.z);
          acc.w = __builtin_fmaf(x, d.w, acc.w);
        }
      reinterpret_cast<float4*>(pw)[it] = acc;
    } else {
      const int c = it - kLnNW2 / 4;
      float t = 0.0f;
      for (int p = 0; p < kLnP2; ++p) t += dzs[p * kLnC2 + c];
      pw[kLnNW2 + c] = t;
    }
  }
  // conv2 input gradient dp1[iy, ix, ci] = sum_{ky, kx, co} dz2[iy - ky, ix - kx, co] W2[ky, kx, ci, co]
  constexpr int kIt = (kLnA1 + kLnThreads - 1) / kLnThreads;        // 5
  float acc[kIt];
#pragma unroll
  for (int i = 0; i < kIt; ++i) {
    const int o = tid + kLnThreads * i;
    float t = 0.0f;
    if (o < kLnA1) {
      const int pos = o / kLnC1, ci = o - pos * kLnC1, iy = pos / kLnQ1, ix = pos - iy * kLnQ1;
      for (int ky = max(0, iy - (kLnH2 - 1)); ky <= min(4, iy); ++ky)
        for (int kx = max(0, ix - (kLnH2 - 1)); kx <= min(4, ix); ++kx) {
          const float4* dr = reinterpret_cast<const float4*>(dzs + ((iy - ky) * kLnH2 + ix - kx) * kLnC2);
          const float4* wr = reinterpret_cast<const float4*>(ws + ((ky * 5 + kx) * kLnC1 + ci) * kLnC2);
#pragma unroll
          for (int c4 = 0; c4 < 4; ++c4) {
            const float4 d = dr[c4], w = wr[c4];
            t = __builtin_fmaf(d.x, w.x, t);
            t = __builtin_fmaf(d.y, w.y, t);
            t = __builtin_fmaf(d.z, w.z, t);
            t = __builtin_fmaf(d.w, w.w, t);
          }
        }
      const float y = p1[o];
      t *= y * (1.0f - y);
    }
    acc[i] = t;
  }
  __syncthreads();
  // pool-1 backward (to the argmax of each window) -> dL/dy1 (BN) or dL/dz1, formed in LDS
  float* d1s = pool;
  for (int o = tid; o < kLnZ1; o += kLnThreads) d1s[o] = 0.0f;
  __syncthreads();
  const int* am = a.am1 + (size_t)s * kLnA1;
#pragma unroll
  for (int i = 0; i < kIt; ++i) {
    const int o = tid + kLnThreads * i;
    if (o < kLnA1) {
      const int pos = o / kLnC1, c = o - pos * kLnC1, py = pos / kLnQ1, px = pos - py * kLnQ1, q = am[o];
      d1s[((2 * py + (q >> 1)) * kLnH1 + 2 * px + (q & 1)) * kLnC1 + c] = acc[i];
    }
  }
  __syncthreads();
  float* d1 = a.d1 + (size_t)s * kLnZ1;
  for (int o = tid; o < kLnZ1; o += kLnThreads) d1[o] = d1s[o];
  if (a.bn)
    cv_sample_bwd_sums<kLnC1>(d1s, a.z1 + (size_t)s * kLnZ1, kLnP1, mean1, rstd1, red, a.bw1 + (size_t)s * kLnC1 * 2);
}

constexpr int kLnRowChunks = 4, kLnRowsPer = kLnH1 / kLnRowChunks;      // dW1: 4 chunks of 7 output rows

__global__ __launch_bounds__(kLnThreads) void k_ln_first(LenetArgs a) {
  __shared__ float img[kLnImg];
  __shared__ float dz[kLnZ1];
  __shared__ float red[kLnThreads];
  __shared__ float part[kLnRowChunks][kLnPW1];
  __shared__ float ma[8], mb[8];
  const int s = blockIdx.x, tid = threadIdx.x;
  if (a.bn) cv_merge_means<kLnC1>(a.bw1, a.batch, (float)kLnP1, red, ma, mb);
  const float4* src = reinterpret_cast<const float4*>(a.images + (size_t)a.idx[s] * kLnImg);
  for (int k = tid; k < kLnImg / 4; k += kLnThreads) reinterpret_cast<float4*>(img)[k] = src[k];
  const float* d1 = a.d1 + (size_t)s * kLnZ1;
  const float* zi = a.z1 + (size_t)s * kLnZ1;
  for (int o = tid; o < kLnZ1; o += kLnThreads) {
    if (a.bn) {
      const int c = o % kLnC1;
      const float r = a.stat[kLnStR1 + c], xh = (zi[o] - a.stat[kLnStM1 + c]) * r;
      dz[o] = r * (d1[o] - ma[c] - xh * mb[c]);
    } else {
      dz[o] = d1[o];
    }
  }
  __syncthreads();
  // this sample's dW1[ky, kx, ci, c] = sum_pos img[pos + (ky, kx), ci] dz[pos, c]: thread = (ky, kx, ci, chunk of 7 output
  // rows), all 6 channels; item 75 of a chunk: db1[c] = sum_pos dz[pos, c]; the 4 chunk sums then added in chunk order
  for (int it = tid; it < kLnRowChunks * 76; it += kLnThreads) {
    const int ch = it / 76, r = it - ch * 76;
    float acc[kLnC1];
#pragma unroll
    for (int c = 0; c < kLnC1; ++c) acc[c] = 0.0f;
    const bool isw = r < 75;
    const int ci = r % 3, kk = isw ? r / 3 : 0, ky = kk / 5, kx = kk - ky * 5;
    const float* ip = img + (ky * 32 + kx) * 3 + ci;
    for (int oy = ch * kLnRowsPer; oy < (ch + 1) * kLnRowsPer; ++oy)
#pragma unroll 4
      for (int ox = 0; ox < kLnH1; ++ox) {
        const float x = isw ? ip[(oy * 32 + ox) * 3] : 1.0f;
        const float* dr = dz + (oy * kLnH1 + ox) * kLnC1;
#pragma unroll
        for (int c = 0; c < kLnC1; ++c) acc[c] = __builtin_fmaf(x, dr[c], acc[c]);
      }
#pragma unroll
    for (int c = 0; c < kLnC1; ++c) part[ch][r * kLnC1 + c] = acc[c];
  }
  __syncthreads();
  float* pw = a.pw1 + (size_t)s * kLnPW1;
  for (int k = tid; k < kLnPW1; k += kLnThreads) {
    float t = part[0][k];
    for (int ch = 1; ch < kLnRowChunks; ++ch) t += part[ch][k];
    pw[k] = t;
  }
}

// the minibatch sums, one thread per coordinate, in sample order (the sample loops unrolled so that 16 loads are in
// flight; the additions keep their order)
constexpr long kLnGradThreads = kLnPW1 + kLnPW2 + kLnN2 * kLnOut + kLnOut + kLnC1 + kLnC2;

__global__ __launch_bounds__(kLnThreads) void k_ln_grad(LenetArgs a) {
  long i = (long)blockIdx.x * kLnThreads + threadIdx.x;
  const int B = a.batch;
  if (i == 0) {
    float t = 0.0f;
#pragma unroll 16
    for (int s = 0; s < B; ++s) t += a.loss_s[s];
    a.loss[0] = t / (float)B;
  }
  if (!a.want_grad) return;
  if (i < kLnPW1) {                                  // dW1, db1
    if (i >= kLnNW1 && a.bn) {
      a.gb1[i - kLnNW1] = cv_bn_bias_grad(a.st1, a.bw1, a.stat + kLnStM1, a.stat + kLnStR1, a.stat + kLnStOne, kLnC1,
                                          (int)(i - kLnNW1), B, (float)kLnP1);
      return;
    }
    float t = 0.0f;
#pragma unroll 16
    for (int s = 0; s < B; ++s) t += a.pw1[(size_t)s * kLnPW1 + i];
    if (i < kLnNW1) a.gw1[i] = t; else a.gb1[i - kLnNW1] = t;
    return;
  }
  i -= kLnPW1;
  if (i < kLnPW2) {                                  // dW2, db2
    if (i >= kLnNW2 && a.bn) {
      a.gb2[i - kLnNW2] = cv_bn_bias_grad(a.st2, a.bw2, a.stat + kLnStM2, a.stat + kLnStR2, a.stat + kLnStOne, kLnC2,
                                          (int)(i - kLnNW2), B, (float)kLnP2);
      return;
    }
    float t = 0.0f;
#pragma unroll 16
    for (int s = 0; s < B; ++s) t += a.pw2[(size_t)s * kLnPW2 + i];
    if (i < kLnNW2) a.gw2[i] = t; else a.gb2[i - kLnNW2] = t;
    return;
  }
  i -= kLnPW2;
  if (i < kLnN2 * kLnOut) {                          // the last linear layer's weights
    const int k = (int)(i / kLnOut), o = (int)(i - (long)k * kLnOut);
    float t = 0.0f;
#pragma unroll 16
    for (int s = 0; s < B; ++s) t = __builtin_fmaf(a.a2[(size_t)s * kLnN2 + k], a.dlog[(size_t)s * 16 + o], t);
    a.gwl2[i] = t;
    return;
  }
  i -= kLnN2 * kLnOut;
  if (i < kLnOut) {                                  // its bias
    float t = 0.0f;
#pragma unroll 16
    for (int s = 0; s < B; ++s) t += a.dlog[(size_t)s * 16 + i];
    a.gbl2[i] = t;
    return;
  }
  i -= kLnOut;
  if (!a.bn) return;
  if (i < kLnC1) {                                   // beta of the conv batch norms = sum dy
    float t = 0.0f;
#pragma unroll 16
    for (int s = 0; s < B; ++s) t += a.bw1[((size_t)s * kLnC1 + i) * 2];
    a.gbe1[i] = t;
    return;
  }
  i -= kLnC1;
  if (i < kLnC2) {
    float t = 0.0f;
#pragma unroll 16
    for (int s = 0; s < B; ++s) t += a.bw2[((size_t)s * kLnC2 + i) * 2];
    a.gbe2[i] = t;
  }
}

}  // namespace l2o
