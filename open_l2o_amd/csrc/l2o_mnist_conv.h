// l2o_mnist_conv.h -- forward + gradient of problems.mnist_conv (DM/problems.py:291-352; DM/util.py:164-169 "mnist_conv"):
// conv 3x3x1x16 VALID -> [BN] -> ReLU -> max-pool 2x2 -> conv 5x5x16x32 VALID -> [BN] -> ReLU -> max-pool 2x2 (9x9 -> 4x4:
// row / column 8 dropped) -> fc 512x10 -> ReLU -> mean sparse softmax cross-entropy.  BN = tf.layers.batch_normalization(
// training=True): batch statistics over (N, H, W), biased variance, eps 1e-3.  NHWC activations, HWIO weights.
// The step-granular evaluation l2o_mnist_conv_fg; included by l2o_nets.hip; written for gfx950 only.
//
// Six launches per evaluation, fp32 VALU, every reduction in a fixed order (no atomics: bit-reproducible):
//   k_cv_conv1    one workgroup per sample: conv1 (+ bias); the sample's per-channel (mean, M2) of z1
//   k_cv_conv2    one workgroup per sample: BN1 statistics merged from the per-sample partials (every workgroup the same
//                 way; workgroup 0 keeps them), normalise, ReLU, pool with argmax, conv2; the sample's (mean, M2) of z2
//   k_cv_head     one workgroup per sample: BN2 statistics, ReLU, pool, fc, ReLU, cross-entropy; backward to dL/dy2 and
//                 the sample's per-channel sum(dy2), sum(dy2 * xhat2)
//   k_cv_mid      one workgroup per sample: BN2 backward -> dz2, the sample's share of dW2 / db2, conv2 input gradient,
//                 pool1 / ReLU1 backward -> dL/dy1 and the sample's sum(dy1), sum(dy1 * xhat1)
//   k_cv_first    one workgroup per sample: BN1 backward -> dz1, the sample's share of dW1 / db1
//   k_cv_grad     one thread per coordinate: the per-sample shares summed in sample order (split-K over the minibatch),
//                 gamma / beta, the fc weights, the conv biases (under batch norm in a factored form, cv_bn_bias_grad);
//                 thread 0 the mean loss
// Forward only (g == NULL): the first three (up to the loss) and the loss sum.
// BN variance: per-sample (mean, M2) merged as M2 = sum M2_s + n sum (mean_s - mean)^2 (never E[z^2] - E[z]^2): the
// reductions of l2o_conv_bn.h (kCvThreads, kCvEps and the cv_* functions).
#pragma once
#include "l2o_conv_bn.h"

namespace l2o {

constexpr int kCvMaxBatch = 1024;
constexpr int kCvC1 = 16, kCvC2 = 32, kCvOut = 10;
constexpr int kCvP1 = 26 * 26, kCvQ1 = 13 * 13, kCvP2 = 9 * 9, kCvQ2 = 4 * 4;
constexpr int kCvNW1 = 3 * 3 * kCvC1, kCvNW2 = 5 * 5 * kCvC1 * kCvC2, kCvNF = kCvQ2 * kCvC2;   // 144, 12800, 512

// per-sample scratch, in floats (offsets of one sample's slice inside each region)
constexpr int kCvZ1 = kCvP1 * kCvC1;      // 10816: z1, and dL/dy1
constexpr int kCvA1 = kCvQ1 * kCvC1;      // 2704:  pooled layer-1 output / its argmax
constexpr int kCvZ2 = kCvP2 * kCvC2;      // 2592:  z2, and dL/dy2 -> dz2
constexpr int kCvPW2 = kCvNW2 + kCvC2;    // dW2 + db2 share of one sample
constexpr int kCvPW1 = kCvNW1 + kCvC1;    // dW1 + db1 share of one sample

struct MnistConvArgs {
  int batch, bn, want_grad;
  const float* images;                    // [n_data, 784]
  const int* labels;
  const int* idx;                         // [batch]
  const float *w1, *b1, *g1, *be1, *w2, *b2, *g2, *be2, *wf, *bf;
  float *gw1, *gb1, *gg1, *gbe1, *gw2, *gb2, *gg2, *gbe2, *gwf, *gbf;
  // scratch
  float* z1;      // [batch][676][16]
  float* p1;      // [batch][169][16]
  int* am1;       // [batch][169][16]   argmax (0..3) of each pool-1 window
  float* z2;      // [batch][81][32]
  float* d2;      // [batch][81][32]    dL/dy2 (BN) -> nothing else reads it; without BN dL/dz2
  float* f;       // [batch][512]       flattened pool-2 output
  float* dlog;    // [batch][16]        dL/dlogits
  float* loss_s;  // [batch]
  float* d1;      // [batch][676][16]   dL/dy1 (BN) or dL/dz1
  float* st1;     // [batch][16][2]     (mean, M2) of z1 per sample
  float* st2;     // [batch][32][2]
  float* bw2;     // [batch][32][2]     (sum dy2, sum dy2 xhat2)
  float* bw1;     // [batch][16][2]
  float* stat;    // mean1[16], rstd1[16], mean2[32], rstd2[32]
  float* pw2;     // [batch][12832]
  float* pw1;     // [batch][160]
  float* loss;    // [1]
};

__global__ __launch_bounds__(kCvThreads) void k_cv_conv1(MnistConvArgs a) {
  __shared__ float img[784];
  __shared__ float z[kCvZ1];
  __shared__ float red[kCvThreads];
  __shared__ float msh[kCvC1];
  const int s = blockIdx.x, tid = threadIdx.x;
  const float* src = a.images + (size_t)a.idx[s] * 784;
  for (int k = tid; k < 784; k += kCvThreads) img[k] = src[k];
  __syncthreads();
  float* zo = a.z1 + (size_t)s * kCvZ1;
  for (int o = tid; o < kCvZ1; o += kCvThreads) {
    const int c = o & 15, pos = o >> 4, oy = pos / 26, ox = pos - oy * 26;
    float acc = 0.0f;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) acc = __builtin_fmaf(img[(oy + ky) * 28 + ox + kx], a.w1[(ky * 3 + kx) * kCvC1 + c], acc);
    const float v = acc + a.b1[c];
    z[o] = v;
    zo[o] = v;
  }
  __syncthreads();
  if (a.bn) cv_sample_stats<kCvC1>(z, kCvP1, red, msh, a.st1 + (size_t)s * kCvC1 * 2);
}

__global__ __launch_bounds__(kCvThreads) void k_cv_conv2(MnistConvArgs a) {
  __shared__ float p1[kCvA1];
  __shared__ float z[kCvZ2];
  __shared__ float red[kCvThreads];
  __shared__ float mean1[kCvC1], rstd1[kCvC1], msh[kCvC2];
  const int s = blockIdx.x, tid = threadIdx.x;
  if (a.bn) {
    cv_merge_stats<kCvC1>(a.st1, a.batch, (float)kCvP1, red, mean1, rstd1);
    if (s == 0 && tid < kCvC1) { a.stat[tid] = mean1[tid]; a.stat[16 + tid] = rstd1[tid]; }
  }
  // BN1 -> ReLU -> 2x2 max-pool (the first maximum of the window in row-major order, like the reference's MaxPoolGrad)
  const float* zi = a.z1 + (size_t)s * kCvZ1;
  int* am = a.am1 + (size_t)s * kCvA1;
  float* po = a.p1 + (size_t)s * kCvA1;
  for (int o = tid; o < kCvA1; o += kCvThreads) {
    const int c = o & 15, pos = o >> 4, py = pos / 13, px = pos - py * 13;
    float best = 0.0f;
    int arg = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      float v = zi[((2 * py + (w >> 1)) * 26 + 2 * px + (w & 1)) * kCvC1 + c];
      if (a.bn) v = __builtin_fmaf(a.g1[c], (v - mean1[c]) * rstd1[c], a.be1[c]);
      v = fmaxf(v, 0.0f);
      if (w == 0 || v > best) { best = v; arg = w; }
    }
    p1[o] = best;
    po[o] = best;
    am[o] = arg;
  }
  __syncthreads();
  // conv2: thread = (output channel co, position group g); positions q = g, g + 8, ... (<= 11 of them)
  {
    const int co = tid & 31, g = tid >> 5;
    int base[11];
    float acc[11];
#pragma unroll
    for (int i = 0; i < 11; ++i) {
      const int q = g + 8 * i, qq = q < kCvP2 ? q : 0, oy = qq / 9, ox = qq - oy * 9;
      base[i] = (oy * 13 + ox) * kCvC1;
      acc[i] = 0.0f;
    }
    for (int ky = 0; ky < 5; ++ky)
      for (int kx = 0; kx < 5; ++kx) {
        const int off = (ky * 13 + kx) * kCvC1;
        const float* wr = a.w2 + (ky * 5 + kx) * kCvC1 * kCvC2 + co;
#pragma unroll 4
        for (int ci = 0; ci < kCvC1; ++ci) {
          const float w = wr[ci * kCvC2];
#pragma unroll
          for (int i = 0; i < 11; ++i) acc[i] = __builtin_fmaf(p1[base[i] + off + ci], w, acc[i]);
        }
      }
    float* zo = a.z2 + (size_t)s * kCvZ2;
#pragma unroll
    for (int i = 0; i < 11; ++i) {
      const int q = g + 8 * i;
      if (q < kCvP2) {
        const float v = acc[i] + a.b2[co];
        z[q * kCvC2 + co] = v;
        zo[q * kCvC2 + co] = v;
      }
    }
  }
  __syncthreads();
  if (a.bn) cv_sample_stats<kCvC2>(z, kCvP2, red, msh, a.st2 + (size_t)s * kCvC2 * 2);
}

__global__ __launch_bounds__(kCvThreads) void k_cv_head(MnistConvArgs a) {
  __shared__ float z[kCvZ2];
  __shared__ float y[kCvZ2];
  __shared__ float dy[kCvZ2];
  __shared__ float fv[kCvNF];
  __shared__ int am[kCvNF];
  __shared__ float red[kCvThreads];
  __shared__ float mean2[kCvC2], rstd2[kCvC2];
  __shared__ float part[kCvOut][16];
  __shared__ float logit[16], dz[16];
  const int s = blockIdx.x, tid = threadIdx.x;
  if (a.bn) {
    cv_merge_stats<kCvC2>(a.st2, a.batch, (float)kCvP2, red, mean2, rstd2);
    if (s == 0 && tid < kCvC2) { a.stat[32 + tid] = mean2[tid]; a.stat[64 + tid] = rstd2[tid]; }
  }
  const float* zi = a.z2 + (size_t)s * kCvZ2;
  for (int o = tid; o < kCvZ2; o += kCvThreads) {
    const int c = o & 31;
    const float v = zi[o];
    z[o] = v;
    y[o] = a.bn ? __builtin_fmaf(a.g2[c], (v - mean2[c]) * rstd2[c], a.be2[c]) : v;
    dy[o] = 0.0f;
  }
  __syncthreads();
  // ReLU -> 2x2 max-pool over rows / columns 0..7; flatten (h * 4 + w) * 32 + c
  for (int o = tid; o < kCvNF; o += kCvThreads) {
    const int c = o & 31, pos = o >> 5, py = pos >> 2, px = pos & 3;
    float best = 0.0f;
    int arg = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int q = (2 * py + (w >> 1)) * 9 + 2 * px + (w & 1);
      const float v = fmaxf(y[q * kCvC2 + c], 0.0f);
      if (w == 0 || v > best) { best = v; arg = q; }
    }
    fv[o] = best;
    am[o] = arg;
  }
  __syncthreads();
  // fc: logit o = bias + sum_k f_k W[k, o]; 16 k-slices per logit, summed in slice order
  if (tid < kCvOut * 16) {
    const int o = tid >> 4, sl = tid & 15;
    float acc = 0.0f;
    for (int k = sl; k < kCvNF; k += 16) acc = __builtin_fmaf(fv[k], a.wf[k * kCvOut + o], acc);
    part[o][sl] = acc;
  }
  __syncthreads();
  const float invB = 1.0f / (float)a.batch;
  if (tid == 0) {
    const int lab = a.labels[a.idx[s]];
    for (int o = 0; o < kCvOut; ++o) {
      float t = a.bf[o];
      for (int k = 0; k < 16; ++k) t += part[o][k];
      logit[o] = t;
    }
    // the reference's quirk: the logits pass through a ReLU before the cross-entropy (DM/problems.py:345)
    float r[kCvOut], rmax = 0.0f;
    for (int o = 0; o < kCvOut; ++o) { r[o] = fmaxf(logit[o], 0.0f); rmax = fmaxf(rmax, r[o]); }
    float se = 0.0f;
    for (int o = 0; o < kCvOut; ++o) se += expf(r[o] - rmax);
    const float lse = rmax + logf(se);
    a.loss_s[s] = lse - r[lab];
    for (int o = 0; o < kCvOut; ++o) {
      const float d = (expf(r[o] - lse) - (o == lab ? 1.0f : 0.0f)) * invB;
      dz[o] = logit[o] > 0.0f ? d : 0.0f;
    }
    if (a.want_grad)
      for (int o = 0; o < 16; ++o) a.dlog[(size_t)s * 16 + o] = o < kCvOut ? dz[o] : 0.0f;
  }
  __syncthreads();
  if (!a.want_grad) return;
  float* fo = a.f + (size_t)s * kCvNF;
  // dL/df -> the argmax of its window (the windows do not overlap) -> ReLU2
  for (int k = tid; k < kCvNF; k += kCvThreads) {
    fo[k] = fv[k];
    float d = 0.0f;
#pragma unroll
    for (int o = 0; o < kCvOut; ++o) d = __builtin_fmaf(a.wf[k * kCvOut + o], dz[o], d);
    const int c = k & 31, at = am[k] * kCvC2 + c;
    dy[at] = y[at] > 0.0f ? d : 0.0f;
  }
  __syncthreads();
  float* d2 = a.d2 + (size_t)s * kCvZ2;
  for (int o = tid; o < kCvZ2; o += kCvThreads) d2[o] = dy[o];
  if (a.bn) cv_sample_bwd_sums<kCvC2>(dy, z, kCvP2, mean2, rstd2, red, a.bw2 + (size_t)s * kCvC2 * 2);
}

__global__ __launch_bounds__(kCvThreads) void k_cv_mid(MnistConvArgs a) {
  // LDS: dz2 | p1 | W2[ky] while the conv2 input gradient is formed, then the whole [676][16] dL/dy1 of the sample
  __shared__ float pool[kCvZ1];
  __shared__ float red[kCvThreads];
  __shared__ float ma[kCvC2], mb[kCvC2], mean1[kCvC1], rstd1[kCvC1];
  float* dz = pool;
  float* p1 = pool + kCvZ2;
  float* ws = pool + kCvZ2 + kCvA1;             // [kx][ci][co], rows padded to 33 (bank spread over ci)
  static_assert(kCvZ2 + kCvA1 + 5 * kCvC1 * 33 <= kCvZ1, "k_cv_mid LDS carve-up");
  const int s = blockIdx.x, tid = threadIdx.x;
  const float* d2 = a.d2 + (size_t)s * kCvZ2;
  if (a.bn) {
    cv_merge_means<kCvC2>(a.bw2, a.batch, (float)kCvP2, red, ma, mb);
    const float* zi = a.z2 + (size_t)s * kCvZ2;
    for (int o = tid; o < kCvZ2; o += kCvThreads) {
      const int c = o & 31;
      const float r = a.stat[64 + c], xh = (zi[o] - a.stat[32 + c]) * r;
      dz[o] = a.g2[c] * r * (d2[o] - ma[c] - xh * mb[c]);
    }
    if (tid < kCvC1) { mean1[tid] = a.stat[tid]; rstd1[tid] = a.stat[16 + tid]; }
  } else {
    for (int o = tid; o < kCvZ2; o += kCvThreads) dz[o] = d2[o];          // (k_cv_head applied ReLU2 already)
  }
  const float* pi = a.p1 + (size_t)s * kCvA1;
  for (int o = tid; o < kCvA1; o += kCvThreads) p1[o] = pi[o];
  __syncthreads();
  // this sample's dW2[ky, kx, ci, co] = sum_q p1[q + (ky, kx), ci] dz[q, co], and db2
  float* pw = a.pw2 + (size_t)s * kCvPW2;
  for (int o = tid; o < kCvNW2; o += kCvThreads) {
    const int co = o & 31, r = o >> 5, ci = r & 15, kk = r >> 4, ky = kk / 5, kx = kk - ky * 5;
    const int off = (ky * 13 + kx) * kCvC1 + ci;
    float acc = 0.0f;
    for (int oy = 0; oy < 9; ++oy)
#pragma unroll
      for (int ox = 0; ox < 9; ++ox) acc = __builtin_fmaf(p1[(oy * 13 + ox) * kCvC1 + off], dz[(oy * 9 + ox) * kCvC2 + co], acc);
    pw[o] = acc;
  }
  if (tid < kCvC2) {
    float t = 0.0f;
    for (int q = 0; q < kCvP2; ++q) t += dz[q * kCvC2 + tid];
    pw[kCvNW2 + tid] = t;
  }
  // conv2 input gradient dp1[iy, ix, ci] = sum_{ky, kx, co} dz[iy - ky, ix - kx, co] W2[ky, kx, ci, co]
  float acc[11];
#pragma unroll
  for (int i = 0; i < 11; ++i) acc[i] = 0.0f;
  for (int ky = 0; ky < 5; ++ky) {
    __syncthreads();
    for (int o = tid; o < 5 * kCvC1 * kCvC2; o += kCvThreads) {
      const int co = o & 31, r = o >> 5;
      ws[r * 33 + co] = a.w2[(ky * 5) * kCvC1 * kCvC2 + o];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 11; ++i) {
      const int o = tid + kCvThreads * i;
      if (o < kCvA1) {
        const int ci = o & 15, pos = o >> 4, iy = pos / 13, ix = pos - iy * 13, oy = iy - ky;
        if (oy >= 0 && oy < 9)
          for (int kx = 0; kx < 5; ++kx) {
            const int ox = ix - kx;
            if (ox < 0 || ox >= 9) continue;
            const float* dr = dz + (oy * 9 + ox) * kCvC2;
            const float* wr = ws + (kx * kCvC1 + ci) * 33;
            float t = acc[i];
#pragma unroll 8
            for (int co = 0; co < kCvC2; ++co) t = __builtin_fmaf(dr[co], wr[co], t);
            acc[i] = t;
          }
      }
    }
  }
  __syncthreads();
  // pool-1 backward (to the argmax of each window) -> ReLU1 -> dL/dy1 (BN) or dL/dz1, formed in LDS
  float* d1s = pool;
  for (int o = tid; o < kCvZ1; o += kCvThreads) d1s[o] = 0.0f;
  __syncthreads();
  const float* zi = a.z1 + (size_t)s * kCvZ1;
  const int* am = a.am1 + (size_t)s * kCvA1;
#pragma unroll
  for (int i = 0; i < 11; ++i) {
    const int o = tid + kCvThreads * i;
    if (o < kCvA1) {
      const int c = o & 15, pos = o >> 4, py = pos / 13, px = pos - py * 13, w = am[o];
      const int at = ((2 * py + (w >> 1)) * 26 + 2 * px + (w & 1)) * kCvC1 + c;
      float yv = zi[at];
      if (a.bn) yv = __builtin_fmaf(a.g1[c], (yv - mean1[c]) * rstd1[c], a.be1[c]);
      d1s[at] = yv > 0.0f ? acc[i] : 0.0f;
    }
  }
  __syncthreads();
  float* d1 = a.d1 + (size_t)s * kCvZ1;
  for (int o = tid; o < kCvZ1; o += kCvThreads) d1[o] = d1s[o];
  if (a.bn) cv_sample_bwd_sums<kCvC1>(d1s, zi, kCvP1, mean1, rstd1, red, a.bw1 + (size_t)s * kCvC1 * 2);
}

__global__ __launch_bounds__(kCvThreads) void k_cv_first(MnistConvArgs a) {
  __shared__ float img[784];
  __shared__ float dz[kCvZ1];
  __shared__ float red[kCvThreads];
  __shared__ float ma[kCvC1], mb[kCvC1];
  const int s = blockIdx.x, tid = threadIdx.x;
  if (a.bn) cv_merge_means<kCvC1>(a.bw1, a.batch, (float)kCvP1, red, ma, mb);
  const float* src = a.images + (size_t)a.idx[s] * 784;
  for (int k = tid; k < 784; k += kCvThreads) img[k] = src[k];
  const float* d1 = a.d1 + (size_t)s * kCvZ1;
  const float* zi = a.z1 + (size_t)s * kCvZ1;
  for (int o = tid; o < kCvZ1; o += kCvThreads) {
    const int c = o & 15;
    if (a.bn) {
      const float r = a.stat[16 + c], xh = (zi[o] - a.stat[c]) * r;
      dz[o] = a.g1[c] * r * (d1[o] - ma[c] - xh * mb[c]);
    } else {
      dz[o] = d1[o];
    }
  }
  __syncthreads();
  // this sample's dW1[ky, kx, c] = sum_pos img[pos + (ky, kx)] dz[pos, c]; db1[c] = sum_pos dz[pos, c]
  float* pw = a.pw1 + (size_t)s * kCvPW1;
  if (tid < kCvNW1) {
    const int c = tid & 15, kk = tid >> 4, ky = kk / 3, kx = kk - ky * 3;
    float acc = 0.0f;
    for (int oy = 0; oy < 26; ++oy)
      for (int ox = 0; ox < 26; ++ox)
        acc = __builtin_fmaf(img[(oy + ky) * 28 + ox + kx], dz[(oy * 26 + ox) * kCvC1 + c], acc);
    pw[tid] = acc;
  } else if (tid < kCvPW1) {
    const int c = tid - kCvNW1;
    float acc = 0.0f;
    for (int p = 0; p < kCvP1; ++p) acc += dz[p * kCvC1 + c];
    pw[tid] = acc;
  }
}

// the minibatch sums, one thread per coordinate, in sample order
__global__ __launch_bounds__(kCvThreads) void k_cv_grad(MnistConvArgs a) {
  long i = (long)blockIdx.x * kCvThreads + threadIdx.x;
  const int B = a.batch;
  if (i == 0) {
    float t = 0.0f;
    for (int s = 0; s < B; ++s) t += a.loss_s[s];
    a.loss[0] = t / (float)B;
  }
  if (!a.want_grad) return;
  if (i < kCvPW1) {                                  // dW1, db1
    if (i >= kCvNW1 && a.bn) {
      a.gb1[i - kCvNW1] = cv_bn_bias_grad(a.st1, a.bw1, a.stat, a.stat + 16, a.g1, kCvC1, (int)(i - kCvNW1), B, (float)kCvP1);
      return;
    }
    float t = 0.0f;
    for (int s = 0; s < B; ++s) t += a.pw1[(size_t)s * kCvPW1 + i];
    if (i < kCvNW1) a.gw1[i] = t; else a.gb1[i - kCvNW1] = t;
    return;
  }
  i -= kCvPW1;
  if (i < kCvPW2) {                                  // dW2, db2
    if (i >= kCvNW2 && a.bn) {
      a.gb2[i - kCvNW2] = cv_bn_bias_grad(a.st2, a.bw2, a.stat + 32, a.stat + 64, a.g2, kCvC2, (int)(i - kCvNW2), B, (float)kCvP2);
      return;
    }
    float t = 0.0f;
    for (int s = 0; s < B; ++s) t += a.pw2[(size_t)s * kCvPW2 + i];
    if (i < kCvNW2) a.gw2[i] = t; else a.gb2[i - kCvNW2] = t;
    return;
  }
  i -= kCvPW2;
  if (i < kCvNF * kCvOut) {                          // fc weights
    const int k = (int)(i / kCvOut), o = (int)(i - (long)k * kCvOut);
    float t = 0.0f;
    for (int s = 0; s < B; ++s) t = __builtin_fmaf(a.f[(size_t)s * kCvNF + k], a.dlog[(size_t)s * 16 + o], t);
    a.gwf[i] = t;
    return;
  }
  i -= kCvNF * kCvOut;
  if (i < kCvOut) {                                  // fc bias
    float t = 0.0f;
    for (int s = 0; s < B; ++s) t += a.dlog[(size_t)s * 16 + i];
    a.gbf[i] = t;
    return;
  }
  i -= kCvOut;
  if (!a.bn) return;
  if (i < 2 * kCvC1) {                               // gamma1 = sum dy1 xhat1, beta1 = sum dy1
    const int c = (int)(i >> 1), j = (int)(i & 1);
    float t = 0.0f;
    for (int s = 0; s < B; ++s) t += a.bw1[((size_t)s * kCvC1 + c) * 2 + (1 - j)];
    (j == 0 ? a.gg1 : a.gbe1)[c] = t;
    return;
  }
  i -= 2 * kCvC1;
  if (i < 2 * kCvC2) {
    const int c = (int)(i >> 1), j = (int)(i & 1);
    float t = 0.0f;
    for (int s = 0; s < B; ++s) t += a.bw2[((size_t)s * kCvC2 + c) * 2 + (1 - j)];
    (j == 0 ? a.gg2 : a.gbe2)[c] = t;
  }
}

constexpr long kCvGradThreads = kCvPW1 + kCvPW2 + kCvNF * kCvOut + kCvOut + 2 * (kCvC1 + kCvC2);

}  // namespace l2o
