// l2o_cifar_conv.h -- forward + gradient of problems.cifar10 (DM/problems.py:369-458; DM/util.py:170-175 "cifar_conv"):
// conv 3x3x3x16 stride 2 VALID (32x32 -> 15x15) -> [BN] -> ReLU -> max-pool 2x2 (15x15 -> 7x7: row / column 14 dropped)
// -> conv 5x5x16x32 stride 2 VALID (7x7 -> 2x2) -> [BN] -> ReLU -> max-pool 2x2 (-> 1x1x32) -> fc 32x10 -> ReLU -> mean
// sparse softmax cross-entropy.  BN = tf.layers.batch_normalization(training=True): batch statistics over (N, H, W),
// biased variance, eps 1e-3.  NHWC activations, HWIO weights.  The step-granular evaluation l2o_cifar_conv_fg; it calls
// the cv_* reductions of l2o_conv_bn.h (256 threads, templated on the channel count); included by l2o_nets.hip;
// written for gfx950 only.
//
// Six launches per evaluation, fp32 VALU, every reduction in a fixed order (no atomics: bit-reproducible):
//   k_cc_conv1    one workgroup per sample: conv1 (+ bias); the sample's per-channel (mean, M2) of z1
//   k_cc_conv2    one workgroup per sample: BN1 statistics merged from the per-sample partials (every workgroup the same
//                 way; workgroup 0 keeps them), normalise, ReLU, pool with argmax, conv2 (two ci halves per output, summed
//                 in half order); the sample's (mean, M2) of z2
//   k_cc_head     kCcHeadSamples samples per workgroup, one thread per (sample, channel): BN2 statistics, ReLU, pool, fc,
//                 ReLU, cross-entropy; backward to dL/dy2 and the sample's per-channel sum(dy2), sum(dy2 * xhat2)
//   k_cc_mid      one workgroup per sample: BN2 backward -> dz2, conv2 input gradient (W2 staged in LDS), pool1 / ReLU1
//                 backward -> dL/dy1 and the sample's sum(dy1), sum(dy1 * xhat1)
//   k_cc_first    one workgroup per sample: BN1 backward -> dz1, the sample's share of dW1 / db1
//   k_cc_grad     the minibatch sums in sample order: dW2 formed directly from the pooled layer-1 outputs and dz2 (a
//                 sample's share is its 4-position sum, never stored), 8 sample chunks per coordinate summed in chunk order;
//                 then one thread per coordinate: db2, dW1 / db1 from the per-sample shares,
//                 gamma / beta, the fc weights, the conv biases under batch norm in the factored form cv_bn_bias_grad;
//                 thread 0 the mean loss
// Forward only (g == NULL): the first three (up to the loss) and the loss sum.
#pragma once
#include "l2o_conv_bn.h"

namespace l2o {

constexpr int kCcThreads = kCvThreads;    // the cv_* helpers assume 256 threads
constexpr int kCcMaxBatch = 1024;
constexpr int kCcImg = 32 * 32 * 3;       // 3072, HWC
constexpr int kCcC1 = 16, kCcC2 = 32, kCcOut = 10;
constexpr int kCcH1 = 15, kCcQ1 = 7, kCcH2 = 2;
constexpr int kCcP1 = kCcH1 * kCcH1, kCcP2 = kCcH2 * kCcH2;            // 225, 4
constexpr int kCcZ1 = kCcP1 * kCcC1;      // 3600: z1, and dL/dy1
constexpr int kCcA1 = kCcQ1 * kCcQ1 * kCcC1;                          // 784: pooled layer-1 output / its argmax
constexpr int kCcZ2 = kCcP2 * kCcC2;      // 128: z2, dL/dy2, dz2
constexpr int kCcNW1 = 3 * 3 * 3 * kCcC1, kCcNW2 = 5 * 5 * kCcC1 * kCcC2, kCcNF = kCcC2;   // 432, 12800, 32
constexpr int kCcPW1 = kCcNW1 + kCcC1;    // dW1 + db1 share of one sample
constexpr int kCcHeadSamples = kCcThreads / kCcC2;                    // 8

struct CifarConvArgs {
  int batch, bn, want_grad;
  const float* images;                    // [n_data, 3072]
  const int* labels;
  const int* idx;                         // [batch]
  const float *w1, *b1, *g1, *be1, *w2, *b2, *g2, *be2, *wf, *bf;
  float *gw1, *gb1, *gg1, *gbe1, *gw2, *gb2, *gg2, *gbe2, *gwf, *gbf;
  // scratch
  float* z1;      // [batch][225][16]
  float* d1;      // [batch][225][16]   dL/dy1 (BN) or dL/dz1
  float* p1;      // [batch][49][16]    pooled layer-1 output
  int* am1;       // [batch][49][16]    argmax (0..3) of each pool-1 window
  float* z2;      // [batch][4][32]
  float* d2;      // [batch][4][32]     dL/dy2 (BN) or dL/dz2
  float* dz2;     // [batch][4][32]
  float* f;       // [batch][32]        pool-2 output
  float* dlog;    // [batch][16]        dL/dlogits
  float* loss_s;  // [batch]
  float* st1;     // [batch][16][2]     (mean, M2) of z1 per sample
  float* bw1;     // [batch][16][2]     (sum dy1, sum dy1 xhat1)
  float* st2;     // [batch][32][2]
  float* bw2;     // [batch][32][2]
  float* pw1;     // [batch][448]
  float* stat;    // mean1[16], rstd1[16], mean2[32], rstd2[32]
  float* loss;    // [1]
};

__global__ __launch_bounds__(kCcThreads) void k_cc_conv1(CifarConvArgs a) {
  __shared__ float img[kCcImg];
  __shared__ float w[kCcNW1];
  __shared__ float z[kCcZ1];
  __shared__ float red[kCcThreads];
  __shared__ float msh[kCcC1];
  const int s = blockIdx.x, tid = threadIdx.x;
  const float4* src = reinterpret_cast<const float4*>(a.images + (size_t)a.idx[s] * kCcImg);
  for (int k = tid; k < kCcImg / 4; k += kCcThreads) reinterpret_cast<float4*>(img)[k] = src[k];
  for (int k = tid; k < kCcNW1; k += kCcThreads) w[k] = a.w1[k];
  __syncthreads();
  float* zo = a.z1 + (size_t)s * kCcZ1;
  for (int o = tid; o < kCcZ1; o += kCcThreads) {
    const int c = o & 15, pos = o >> 4, oy = pos / kCcH1, ox = pos - oy * kCcH1;
    const float* ip = img + (2 * oy * 32 + 2 * ox) * 3;
    float acc = 0.0f;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx)
#pragma unroll
        for (int ci = 0; ci < 3; ++ci)
          acc = __builtin_fmaf(ip[(ky * 32 + kx) * 3 + ci], w[((ky * 3 + kx) * 3 + ci) * kCcC1 + c], acc);
    const float v = acc + a.b1[c];
    z[o] = v;
    zo[o] = v;
  }
  __syncthreads();
  if (a.bn) cv_sample_stats<kCcC1>(z, kCcP1, red, msh, a.st1 + (size_t)s * kCcC1 * 2);
}

__global__ __launch_bounds__(kCcThreads) void k_cc_conv2(CifarConvArgs a) {
  __shared__ float p1[kCcA1];
  __shared__ float z[kCcZ2];
  __shared__ float red[kCcThreads];
  __shared__ float mean1[kCcC1], rstd1[kCcC1], msh[kCcC2];
  const int s = blockIdx.x, tid = threadIdx.x;
  if (a.bn) {
    cv_merge_stats<kCcC1>(a.st1, a.batch, (float)kCcP1, red, mean1, rstd1);
    if (s == 0 && tid < kCcC1) { a.stat[tid] = mean1[tid]; a.stat[16 + tid] = rstd1[tid]; }
  }
  // BN1 -> ReLU -> 2x2 max-pool over rows / columns 0..13 (the first maximum of the window in row-major order, like the
  // reference's MaxPoolGrad)
  const float* zi = a.z1 + (size_t)s * kCcZ1;
  int* am = a.am1 + (size_t)s * kCcA1;
  float* po = a.p1 + (size_t)s * kCcA1;
  for (int o = tid; o < kCcA1; o += kCcThreads) {
    const int c = o & 15, pos = o >> 4, py = pos / kCcQ1, px = pos - py * kCcQ1;
    float best = 0.0f;
    int arg = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      float v = zi[((2 * py + (w >> 1)) * kCcH1 + 2 * px + (w & 1)) * kCcC1 + c];
      if (a.bn) v = __builtin_fmaf(a.g1[c], (v - mean1[c]) * rstd1[c], a.be1[c]);
      v = fmaxf(v, 0.0f);
      if (w == 0 || v > best) { best = v; arg = w; }
    }
    p1[o] = best;
    po[o] = best;
    am[o] = arg;
  }
  __syncthreads();
  // conv2, stride 2: thread = (output channel co, position q, input-channel half h); the halves summed in order
  {
    const int co = tid & 31, q = (tid >> 5) & 3, h = tid >> 7, oy = q >> 1, ox = q & 1;
    const float* pb = p1 + ((2 * oy) * kCcQ1 + 2 * ox) * kCcC1 + 8 * h;
    const float* wb = a.w2 + 8 * h * kCcC2 + co;
    float acc = 0.0f;
    for (int ky = 0; ky < 5; ++ky)
#pragma unroll
      for (int kx = 0; kx < 5; ++kx)
#pragma unroll
        for (int ci = 0; ci < 8; ++ci)
          acc = __builtin_fmaf(pb[(ky * kCcQ1 + kx) * kCcC1 + ci], wb[((ky * 5 + kx) * kCcC1 + ci) * kCcC2], acc);
    red[tid] = acc;
  }
  __syncthreads();
  if (tid < kCcZ2) {
    const float v = (red[tid] + red[tid + kCcZ2]) + a.b2[tid & 31];
    z[tid] = v;
    a.z2[(size_t)s * kCcZ2 + tid] = v;
  }
  __syncthreads();
  if (a.bn) cv_sample_stats<kCcC2>(z, kCcP2, red, msh, a.st2 + (size_t)s * kCcC2 * 2);
}

__global__ __launch_bounds__(kCcThreads) void k_cc_head(CifarConvArgs a) {
  __shared__ float red[kCcThreads];
  __shared__ float mean2[kCcC2], rstd2[kCcC2];
  __shared__ float fv[kCcHeadSamples][kCcNF];
  __shared__ float dz[kCcHeadSamples][16];
  const int tid = threadIdx.x, c = tid & 31, ls = tid >> 5, s = blockIdx.x * kCcHeadSamples + ls;
  const bool live = s < a.batch;
  if (a.bn) {
    cv_merge_stats<kCcC2>(a.st2, a.batch, (float)kCcP2, red, mean2, rstd2);
    if (blockIdx.x == 0 && tid < kCcC2) { a.stat[32 + tid] = mean2[tid]; a.stat[64 + tid] = rstd2[tid]; }
  }
  // BN2 -> ReLU -> 2x2 max-pool of the whole 2x2 map: one feature per channel
  float zv[kCcP2], yv[kCcP2];
  float best = 0.0f;
  int arg = 0;
  if (live) {
#pragma unroll
    for (int q = 0; q < kCcP2; ++q) {
      zv[q] = a.z2[(size_t)s * kCcZ2 + q * kCcC2 + c];
      yv[q] = a.bn ? __builtin_fmaf(a.g2[c], (zv[q] - mean2[c]) * rstd2[c], a.be2[c]) : zv[q];
      const float v = fmaxf(yv[q], 0.0f);
      if (q == 0 || v > best) { best = v; arg = q; }
    }
  }
  fv[ls][c] = best;
  __syncthreads();
  // fc (32 terms in order) -> ReLU -> cross-entropy: one thread per sample
  const float invB = 1.0f / (float)a.batch;
  if (c == 0 && live) {
    const int lab = a.labels[a.idx[s]];
    float logit[kCcOut], r[kCcOut], rmax = 0.0f;
    for (int o = 0; o < kCcOut; ++o) {
      float t = 0.0f;
      for (int k = 0; k < kCcNF; ++k) t = __builtin_fmaf(fv[ls][k], a.wf[k * kCcOut + o], t);
      logit[o] = t + a.bf[o];
      // the reference's quirk: the logits pass through a ReLU before the cross-entropy (DM/problems.py:451)
      r[o] = fmaxf(logit[o], 0.0f);
      rmax = fmaxf(rmax, r[o]);
    }
    float se = 0.0f;
    for (int o = 0; o < kCcOut; ++o) se += expf(r[o] - rmax);
    const float lse = rmax + logf(se);
    a.loss_s[s] = lse - r[lab];
    for (int o = 0; o < kCcOut; ++o) {
      const float d = (expf(r[o] - lse) - (o == lab ? 1.0f : 0.0f)) * invB;
      dz[ls][o] = logit[o] > 0.0f ? d : 0.0f;
    }
    if (a.want_grad)
      for (int o = 0; o < 16; ++o) a.dlog[(size_t)s * 16 + o] = o < kCcOut ? dz[ls][o] : 0.0f;
  }
  __syncthreads();
  if (!a.want_grad || !live) return;
  // dL/df -> the argmax of the window -> ReLU2 -> dL/dy2; the sample's (sum dy2, sum dy2 xhat2) over the 4 positions
  a.f[(size_t)s * kCcNF + c] = best;
  float d = 0.0f;
#pragma unroll
  for (int o = 0; o < kCcOut; ++o) d = __builtin_fmaf(a.wf[c * kCcOut + o], dz[ls][o], d);
  float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
  for (int q = 0; q < kCcP2; ++q) {
    const float dy = (q == arg && yv[q] > 0.0f) ? d : 0.0f;
    a.d2[(size_t)s * kCcZ2 + q * kCcC2 + c] = dy;
    if (a.bn) {
      s0 += dy;
      s1 = __builtin_fmaf(dy, (zv[q] - mean2[c]) * rstd2[c], s1);
    }
  }
  if (a.bn) {
    a.bw2[((size_t)s * kCcC2 + c) * 2] = s0;
    a.bw2[((size_t)s * kCcC2 + c) * 2 + 1] = s1;
  }
}

__global__ __launch_bounds__(kCcThreads) void k_cc_mid(CifarConvArgs a) {
  // LDS: W2 as [ky][kx][ci][co] with rows padded to 33 (bank spread over ci) while the conv2 input gradient is formed,
  // then the sample's [225][16] dL/dy1 in the same space
  constexpr int kWs = 25 * kCcC1 * 33;
  static_assert(kCcZ1 <= kWs, "k_cc_mid LDS carve-up");
  __shared__ float pool[kWs];
  __shared__ float dzs[kCcZ2];
  __shared__ float red[kCcThreads];
  __shared__ float ma[kCcC2], mb[kCcC2], mean1[kCcC1], rstd1[kCcC1];
  const int s = blockIdx.x, tid = threadIdx.x;
  if (a.bn) {
    cv_merge_means<kCcC2>(a.bw2, a.batch, (float)kCcP2, red, ma, mb);
    if (tid < kCcC1) { mean1[tid] = a.stat[tid]; rstd1[tid] = a.stat[16 + tid]; }
  }
  if (tid < kCcZ2) {
    const int c = tid & 31;
    const float dy = a.d2[(size_t)s * kCcZ2 + tid];
    float v = dy;                                                      // (k_cc_head applied ReLU2 already)
    if (a.bn) {
      const float r = a.stat[64 + c], xh = (a.z2[(size_t)s * kCcZ2 + tid] - a.stat[32 + c]) * r;
      v = a.g2[c] * r * (dy - ma[c] - xh * mb[c]);
    }
    dzs[tid] = v;
    a.dz2[(size_t)s * kCcZ2 + tid] = v;
  }
  for (int o = tid; o < kCcNW2; o += kCcThreads) pool[(o >> 5) * 33 + (o & 31)] = a.w2[o];
  __syncthreads();
  // conv2 input gradient dp1[iy, ix, ci] = sum_{oy, ox, co} dz2[oy, ox, co] W2[iy - 2 oy, ix - 2 ox, ci, co]
  constexpr int kIt = (kCcA1 + kCcThreads - 1) / kCcThreads;        // 4
  float acc[kIt];
#pragma unroll
  for (int i = 0; i < kIt; ++i) {
    const int o = tid + kCcThreads * i;
    float t = 0.0f;
    if (o < kCcA1) {
      const int ci = o & 15, pos = o >> 4, iy = pos / kCcQ1, ix = pos - iy * kCcQ1;
      for (int oy = 0; oy < kCcH2; ++oy) {
        const int ky = iy - 2 * oy;
        if (ky < 0 || ky >= 5) continue;
        for (int ox = 0; ox < kCcH2; ++ox) {
          const int kx = ix - 2 * ox;
          if (kx < 0 || kx >= 5) continue;
          const float* dr = dzs + (oy * kCcH2 + ox) * kCcC2;
          const float* wr = pool + ((ky * 5 + kx) * kCcC1 + ci) * 33;
#pragma unroll 8
          for (int co = 0; co < kCcC2; ++co) t = __builtin_fmaf(dr[co], wr[co], t);
        }
      }
    }
    acc[i] = t;
  }
  __syncthreads();
  // pool-1 backward (to the argmax of each window) -> ReLU1 -> dL/dy1 (BN) or dL/dz1, formed in LDS; row / column 14 of
  // the map get 0
  float* d1s = pool;
  for (int o = tid; o < kCcZ1; o += kCcThreads) d1s[o] = 0.0f;
  __syncthreads();
  const float* zi = a.z1 + (size_t)s * kCcZ1;
  const int* am = a.am1 + (size_t)s * kCcA1;
#pragma unroll
  for (int i = 0; i < kIt; ++i) {
    const int o = tid + kCcThreads * i;
    if (o < kCcA1) {
      const int c = o & 15, pos = o >> 4, py = pos / kCcQ1, px = pos - py * kCcQ1, w = am[o];
      const int at = ((2 * py + (w >> 1)) * kCcH1 + 2 * px + (w & 1)) * kCcC1 + c;
      float yv = zi[at];
      if (a.bn) yv = __builtin_fmaf(a.g1[c], (yv - mean1[c]) * rstd1[c], a.be1[c]);
      d1s[at] = yv > 0.0f ? acc[i] : 0.0f;
    }
  }
  __syncthreads();
  float* d1 = a.d1 + (size_t)s * kCcZ1;
  for (int o = tid; o < kCcZ1; o += kCcThreads) d1[o] = d1s[o];
  if (a.bn) cv_sample_bwd_sums<kCcC1>(d1s, zi, kCcP1, mean1, rstd1, red, a.bw1 + (size_t)s * kCcC1 * 2);
}

__global__ __launch_bounds__(kCcThreads) void k_cc_first(CifarConvArgs a) {
  __shared__ float img[kCcImg];
  __shared__ float dz[kCcZ1];
  __shared__ float red[kCcThreads];
  __shared__ float ma[kCcC1], mb[kCcC1];
  const int s = blockIdx.x, tid = threadIdx.x;
  if (a.bn) cv_merge_means<kCcC1>(a.bw1, a.batch, (float)kCcP1, red, ma, mb);
  const float4* src = reinterpret_cast<const float4*>(a.images + (size_t)a.idx[s] * kCcImg);
  for (int k = tid; k < kCcImg / 4; k += kCcThreads) reinterpret_cast<float4*>(img)[k] = src[k];
  const float* d1 = a.d1 + (size_t)s * kCcZ1;
  const float* zi = a.z1 + (size_t)s * kCcZ1;
  for (int o = tid; o < kCcZ1; o += kCcThreads) {
    const int c = o & 15;
    if (a.bn) {
      const float r = a.stat[16 + c], xh = (zi[o] - a.stat[c]) * r;
      dz[o] = a.g1[c] * r * (d1[o] - ma[c] - xh * mb[c]);
    } else {
      dz[o] = d1[o];
    }
  }
  __syncthreads();
  // this sample's dW1[ky, kx, ci, c] = sum_pos img[2 pos + (ky, kx), ci] dz[pos, c]; db1[c] = sum_pos dz[pos, c]
  float* pw = a.pw1 + (size_t)s * kCcPW1;
  for (int k = tid; k < kCcPW1; k += kCcThreads) {
    float acc = 0.0f;
    if (k < kCcNW1) {
      const int c = k & 15, r = k >> 4, ci = r % 3, kk = r / 3, ky = kk / 3, kx = kk - ky * 3;
      const float* ip = img + (ky * 32 + kx) * 3 + ci;
      for (int oy = 0; oy < kCcH1; ++oy)
#pragma unroll 5
        for (int ox = 0; ox < kCcH1; ++ox)
          acc = __builtin_fmaf(ip[(2 * oy * 32 + 2 * ox) * 3], dz[(oy * kCcH1 + ox) * kCcC1 + c], acc);
    } else {
      const int c = k - kCcNW1;
      for (int p = 0; p < kCcP1; ++p) acc += dz[p * kCcC1 + c];
    }
    pw[k] = acc;
  }
}

// dW2 split over the minibatch: a workgroup owns 32 coordinates (one kernel row (ky, kx, ci), every co); 8 threads per
// coordinate each sum the shares of one contiguous chunk of samples in sample order, then the chunk sums are added in chunk
// order -- still one fixed order, 8x shorter dependent chains than one thread per coordinate
constexpr int kCcW2Chunks = kCcThreads / kCcC2;                       // 8
constexpr int kCcW2Blocks = kCcNW2 / kCcC2;                           // 400

// the minibatch sums, in sample order: dW2 in the first kCcW2Blocks workgroups (when the gradient is wanted), then one
// thread per remaining coordinate (its sample loops unrolled so that the loads of 16 samples are in flight at once; the
// additions keep their order)
__global__ __launch_bounds__(kCcThreads) void k_cc_grad(CifarConvArgs a) {
  __shared__ float part[kCcThreads];
  const int B = a.batch, nw2 = a.want_grad ? kCcW2Blocks : 0;
  if ((int)blockIdx.x < nw2) {                       // dW2: a sample's share is its sum over the 2x2 output positions
    const int co = threadIdx.x & 31, ch = threadIdx.x >> 5, r = blockIdx.x, ci = r & 15, kk = r >> 4, ky = kk / 5,
              kx = kk - ky * 5;
    const int len = (B + kCcW2Chunks - 1) / kCcW2Chunks, s0 = ch * len, s1 = min(B, s0 + len);
    const float* pb = a.p1 + (ky * kCcQ1 + kx) * kCcC1 + ci;
    const float* db = a.dz2 + co;
    float t = 0.0f;
#pragma unroll 4
    for (int s = s0; s < s1; ++s) {
      const float* ps = pb + (size_t)s * kCcA1;
      const float* ds = db + (size_t)s * kCcZ2;
      float sh = 0.0f;
#pragma unroll
      for (int q = 0; q < kCcP2; ++q)
        sh = __builtin_fmaf(ps[(2 * (q >> 1) * kCcQ1 + 2 * (q & 1)) * kCcC1], ds[q * kCcC2], sh);
      t += sh;
    }
    part[threadIdx.x] = t;
    __syncthreads();
    if (ch == 0) {
      float u = part[co];
      for (int k = 1; k < kCcW2Chunks; ++k) u += part[k * kCcC2 + co];
      a.gw2[r * kCcC2 + co] = u;
    }
    return;
  }
  long i = (long)(blockIdx.x - nw2) * kCcThreads + threadIdx.x;
  if (i == 0) {
    float t = 0.0f;
#pragma unroll 16
    for (int s = 0; s < B; ++s) t += a.loss_s[s];
    a.loss[0] = t / (float)B;
  }
  if (!a.want_grad) return;
  if (i < kCcC2) {                                   // db2
    const int c = (int)i;
    if (a.bn) {
      a.gb2[c] = cv_bn_bias_grad(a.st2, a.bw2, a.stat + 32, a.stat + 64, a.g2, kCcC2, c, B, (float)kCcP2);
      return;
    }
    float t = 0.0f;
#pragma unroll 16
    for (int s = 0; s < B; ++s) {
      float sh = 0.0f;
#pragma unroll
      for (int q = 0; q < kCcP2; ++q) sh += a.dz2[(size_t)s * kCcZ2 + q * kCcC2 + c];
      t += sh;
    }
    a.gb2[c] = t;
    return;
  }
  i -= kCcC2;
  if (i < kCcPW1) {                                  // dW1, db1
    if (i >= kCcNW1 && a.bn) {
      a.gb1[i - kCcNW1] = cv_bn_bias_grad(a.st1, a.bw1, a.stat, a.stat + 16, a.g1, kCcC1, (int)(i - kCcNW1), B, (float)kCcP1);
      return;
    }
    float t = 0.0f;
#pragma unroll 16
    for (int s = 0; s < B; ++s) t += a.pw1[(size_t)s * kCcPW1 + i];
    if (i < kCcNW1) a.gw1[i] = t; else a.gb1[i - kCcNW1] = t;
    return;
  }
  i -= kCcPW1;
  if (i < kCcNF * kCcOut) {                          // fc weights
    const int k = (int)(i / kCcOut), o = (int)(i - (long)k * kCcOut);
    float t = 0.0f;
#pragma unroll 16
    for (int s = 0; s < B; ++s) t = __builtin_fmaf(a.f[(size_t)s * kCcNF + k], a.dlog[(size_t)s * 16 + o], t);
    a.gwf[i] = t;
    return;
  }
  i -= kCcNF * kCcOut;
  if (i < kCcOut) {                                  // fc bias
    float t = 0.0f;
#pragma unroll 16
    for (int s = 0; s < B; ++s) t += a.dlog[(size_t)s * 16 + i];
    a.gbf[i] = t;
    return;
  }
  i -= kCcOut;
  if (!a.bn) return;
  if (i < 2 * kCcC1) {                               // gamma1 = sum dy1 xhat1, beta1 = sum dy1
    const int c = (int)(i >> 1), j = (int)(i & 1);
    float t = 0.0f;
#pragma unroll 16
    for (int s = 0; s < B; ++s) t += a.bw1[((size_t)s * kCcC1 + c) * 2 + (1 - j)];
    (j == 0 ? a.gg1 : a.gbe1)[c] = t;
    return;
  }
  i -= 2 * kCcC1;
  if (i < 2 * kCcC2) {
    const int c = (int)(i >> 1), j = (int)(i & 1);
    float t = 0.0f;
#pragma unroll 16
    for (int s = 0; s < B; ++s) t += a.bw2[((size_t)s * kCcC2 + c) * 2 + (1 - j)];
    (j == 0 ? a.gg2 : a.gbe2)[c] = t;
  }
}

constexpr long kCcGradThreads = kCcC2 + kCcPW1 + kCcNF * kCcOut + kCcOut + 2 * (kCcC1 + kCcC2);   // after the dW2 workgroups

}  // namespace l2o
