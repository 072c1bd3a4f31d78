// l2o_nas.h -- problems.NAS (DM/problems.py:540-634): the NAS-cell conv net on CIFAR-10, loss and gradients of one
// minibatch.  Included by l2o_nets.hip (host side: l2o_nas_fg there).
//
// Four layers L = relu([batch norm](conv 3x3 SAME + bias)) of 16 channels at 32x32 -- node0 (from the 3-channel image),
// n02 and node1 (both from node0) and n13 (from node1) -- then node3 = avg_pool3x3(node1) + n02 + n13 + node0, its mean
// over the positions, fc 16x10, ReLU and the mean softmax cross-entropy.  Activations NHWC, weights HWIO = the row-major
// [9 C_in][16] GEMM operand.  Only the PRE-activations z are stored; a consumer applies the layer's per-channel
// (scale, shift) and the ReLU while it stages its operand, and a gradient w.r.t. z,
//   dz = gamma rstd (dy - mean(dy) - xhat mean(dy xhat)),   dy = dL/d(bn output) with the ReLU mask applied,
// is likewise formed while it is staged, from z, dy and seven per-channel numbers (NsP*).  Without batch norm those numbers
// are the identity (scale 1, shift 0, ..., the two means 0) and the same kernels run.
// Two facts keep the backward pass short: dL/dnode3 is u[b][c] / 1024 at every position (u = dL/dnf), so the dy of n13 and
// n02 need no array (u / 1024 under the layer's own ReLU mask); and the adjoint of the average pool applied to a
// position-constant field is that constant times k(y) k(x), k = 5/6, 7/6, 1, ..., 1, 7/6, 5/6 (the sum over the windows a
// cell is in of 1 / their valid count), so there is no pool kernel: the same factor gives the forward mean of the pooled
// node1 as a weighted mean of node1.
// The GEMMs run on v_mfma_f32_16x16x4_f32 (exact fp32: a k-ordered fmaf chain).  A workgroup of 4 waves owns a strip of 8
// image rows (256 pixels) of one sample, staged once into LDS with its halo (10 x 34 cells; the zero padding is written
// there), pixel-major with a row of 17 floats per 16 channels:
//   k_ns_conv<CG, NOUT, MODE>  rows = pixels, reduction = (tap, channel of the staged operand), columns = NOUT
//        NS_RAW / NS_ACT: forward.  <3,16> node0; <16,32> n02 and node1 as ONE GEMM; <16,16> n13.  Epilogue: + bias
//        NS_DZ: input gradient, the weights read flipped (tap -> 8 - tap) and transposed.  <16,16> n13 -> node1;
//               <32,16> (n02, node1) -> node0 as ONE GEMM with a reduction of 9 x 32.  Epilogue: + the position-constant
//               part (u / 1024, times k k for the pool), then the ReLU mask of the layer below
//   k_ns_wgrad<CIN, NOUT>      rows = (tap, c_in), reduction = pixels, columns = NOUT; a workgroup walks the strips
//        blockIdx.x, + gridDim.x, ..., its four waves a quarter of each strip; the waves' accumulators are added in wave
//        order, every workgroup writes its partial, and k_ns_wsum adds the partials in a fixed order
// Batch-norm statistics: per-sample (mean, M2) partials (cv_sample_stats) merged in a fixed order (cv_merge_stats), both of
// l2o_conv_bn.h; the backward sums (sum dy, sum dy xhat) likewise per sample, then in sample order.  Under batch norm
// the gradient of a conv bias is 0 in exact arithmetic; it is written as that analytic 0 (not in cv_bn_bias_grad's
// factored form).  No atomics anywhere.
#pragma once
#include "l2o_common.h"
#include "l2o_conv_bn.h"
#include "../../include/l2o_nas_abi.h"

constexpr int kNsThreads = 256;
constexpr int kNsMaxBatch = 1024;
constexpr int kNsC = 16, kNsClasses = 10;
constexpr int kNsPix = 1024;                  // positions of one sample
constexpr int kNsStrip = 256;                 // pixels of a strip: 8 rows of 32
constexpr int kNsHalo = 10 * 34;              // cells of a strip with its halo
constexpr int kNsPlane = kNsHalo * 17;        // floats of 16 staged channels of a halo tile
constexpr int kNsDPlane = kNsStrip * 17;      // ... of a strip without halo
constexpr int kNsLayers = 4;                  // node0, n02, node1, n13: the order of the variables and of the NsP blocks
// the per-channel numbers of a layer, [7][16] floats
constexpr int NsPScale = 0, NsPShift = 16, NsPMean = 32, NsPRstd = 48, NsPGr = 64, NsPM1 = 80, NsPM2 = 96, kNsP = 112;
constexpr int NS_RAW = 0, NS_ACT = 1, NS_DZ = 2;
constexpr int kNsWPart = 144 * 32;            // floats of one weight-gradient partial (the largest: [144][32])

typedef float ns_f32x4 __attribute__((ext_vector_type(4)));

inline int ns_wgrad_groups(int batch) { return 4 * batch < 256 ? 4 * batch : 256; }

// 16 channels of a staged operand
struct NsSrc {
  const float* z;     // [M][ldz] pre-activations (NS_RAW: the image [M][3])
  const float* dy;    // NS_DZ: [M][16] dL/d(bn output), masked; NULL: v[b][c] under the mask of z
  const float* P;     // the layer's NsP block
  int ldz;
};
struct NsChan {
  float scale, shift, mean, rstd, gr, m1, m2;
};
template <int MODE>
__device__ __forceinline__ NsChan ns_chan(const float* P, int c) {
  NsChan p = {1.0f, 0.0f, 0.0f, 1.0f, 1.0f, 0.0f, 0.0f};
  p.scale = P[NsPScale + c]; p.shift = P[NsPShift + c];
  if (MODE == NS_DZ) {
    p.mean = P[NsPMean + c]; p.rstd = P[NsPRstd + c]; p.gr = P[NsPGr + c]; p.m1 = P[NsPM1 + c]; p.m2 = P[NsPM2 + c];
  }
  return p;
}
__device__ __forceinline__ float ns_dy(const NsSrc& s, const NsChan& p, const float* v, size_t m, int c, float z) {
  return s.dy ? s.dy[m * 16 + c] : (fmaf(p.scale, z, p.shift) > 0.0f ? v[(m >> 10) * 16 + c] : 0.0f);
}
// the staged value of pixel m, channel c of the group: the layer's output (NS_ACT) or the gradient w.r.t. its z (NS_DZ)
template <int MODE>
__device__ __forceinline__ float ns_value(const NsSrc& s, const NsChan& p, const float* v, size_t m, int c) {
  const float z = s.z[m * s.ldz + c];
  if (MODE == NS_ACT) return fmaxf(fmaf(p.scale, z, p.shift), 0.0f);
  const float dy = ns_dy(s, p, v, m, c, z);
  return p.gr * ((dy - p.m1) - ((z - p.mean) * p.rstd) * p.m2);
}
// group grp (0 / 1) of a two-group operand, by value (no indexed access to kernel arguments)
__device__ __forceinline__ NsSrc ns_pick(const NsSrc& s0, const NsSrc& s1, int grp) {
  NsSrc s;
  s.z = grp ? s1.z : s0.z; s.dy = grp ? s1.dy : s0.dy; s.P = grp ? s1.P : s0.P; s.ldz = grp ? s1.ldz : s0.ldz;
  return s;
}
__device__ __forceinline__ float ns_pool_k(int t) {
  return (t == 0 || t == 31) ? 5.0f / 6.0f : ((t == 1 || t == 30) ? 7.0f / 6.0f : 1.0f);
}

// the strip rows y0 .. y0 + 7 of sample b with a halo of one cell, C channels: sIn[(c >> 4) kNsPlane + cell * 17 + (c & 15)]
// (C == 3: sIn[cell * 3 + c]); cells outside the image are 0
template <int MODE, int C>
__device__ __forceinline__ void ns_stage_halo(float* sIn, const NsSrc& s0, const NsSrc& s1, const float* v, int b, int y0) {
  const int tid = threadIdx.x;
  if constexpr (C == 3) {
    for (int e = tid; e < kNsHalo * 3; e += kNsThreads) {
      const int cell = e / 3, c = e - 3 * cell;
      const int hy = cell / 34, hx = cell - 34 * hy;
      const int y = y0 + hy - 1, x = hx - 1;
      float val = 0.0f;
      if ((unsigned)y < 32u && (unsigned)x < 32u) val = s0.z[((size_t)b * kNsPix + y * 32 + x) * 3 + c];
      sIn[e] = val;
    }
  } else {
    const int c = tid % C, grp = c >> 4, cc = c & 15;
    const NsSrc s = ns_pick(s0, s1, grp);
    const NsChan p = ns_chan<MODE>(s.P, cc);
    for (int cell = tid / C; cell < kNsHalo; cell += kNsThreads / C) {
      const int hy = cell / 34, hx = cell - 34 * hy;
      const int y = y0 + hy - 1, x = hx - 1;
      float val = 0.0f;
      if ((unsigned)y < 32u && (unsigned)x < 32u) val = ns_value<MODE>(s, p, v, (size_t)b * kNsPix + y * 32 + x, cc);
      sIn[grp * kNsPlane + cell * 17 + cc] = val;
    }
  }
}

struct NsConv {
  NsSrc src[2];        // the staged operand, 16 channels each (CG == 3: src[0].z is the image)
  const float* v;      // [B][16] u / 1024
  const float* w[2];   // forward: the weights of output columns 0-15 / 16-31, [9 CG][16]; NS_DZ: of staged channels 0-15 / 16-31
  const float* bias[2];
  float* out;          // forward: z [M][NOUT]; NS_DZ: dy of the layer below [M][16]
  const float* zb;     // NS_DZ: the z of the layer below [M][ldzb] and its NsP block
  const float* Pb;
  int ldzb, pool;      // pool: the position-constant part is v k(y) k(x) (the average pool's adjoint), else v
};

template <int CG, int NOUT, int MODE>
__global__ __launch_bounds__(kNsThreads) void k_ns_conv(const NsConv a) {
  constexpr int CP = CG == 3 ? 3 : 17;
  constexpr int K = 9 * CG, KS = (K + 3) / 4;           // reduction length; MFMA steps
  constexpr int NB = NOUT / 16;
  constexpr int SW = NOUT == 32 ? 48 : 16;               // row stride of the weights in LDS (the four k of a step: own banks)
  constexpr int NIN = CG == 3 ? kNsHalo * 3 : (CG / 16) * kNsPlane;
  __shared__ float sIn[NIN];
  __shared__ float sW[KS * 4 * SW];
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, lg = lane >> 4;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.x >> 2, y0 = 8 * (blockIdx.x & 3);

  for (int e = tid; e < KS * 4 * NOUT; e += kNsThreads) {
    const int k = e / NOUT, n = e - k * NOUT;
    float val = 0.0f;
    if (k < K) {
      if (MODE == NS_DZ) {                                // B(k = (tap, c), n = ci) = w_{c >> 4}[8 - tap][ci][c & 15]
        const int tap = k / CG, c = k - tap * CG;
        val = (c < 16 ? a.w[0] : a.w[1])[((8 - tap) * 16 + n) * 16 + (c & 15)];
      } else {
        val = (n < 16 ? a.w[0] : a.w[1])[k * 16 + (n & 15)];
      }
    }
    sW[k * SW + n] = val;
  }
  ns_stage_halo<MODE, CG>(sIn, a.src[0], a.src[1], a.v, b, y0);
  __syncthreads();

  ns_f32x4 acc[4][NB];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[t][nb] = ns_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  // tile t of the wave: row 2 wv + (t >> 1) of the strip, x = 16 (t & 1) + li
  int base[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) base[t] = ((2 * wv + (t >> 1)) * 34 + 16 * (t & 1) + li) * CP;
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    int off;
    bool kok = true;
    if constexpr (CG == 3) {
      const int k = 4 * s + lg;
      kok = k < K;
      const int tap = kok ? k / 3 : 0, c = kok ? k - 3 * tap : 0;
      off = ((tap / 3) * 34 + (tap % 3)) * 3 + c;
    } else {
      const int tap = (4 * s) / CG, c0 = (4 * s) % CG;    // compile-time under the unroll
      off = ((tap / 3) * 34 + (tap % 3)) * 17 + (c0 >> 4) * kNsPlane + (c0 & 15) + lg;
    }
    float bv[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) bv[nb] = sW[(4 * s + lg) * SW + nb * 16 + li];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const float av = kok ? sIn[base[t] + off] : 0.0f;
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[t][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[nb], acc[t][nb], 0, 0, 0);
    }
  }

  // ---- epilogue: D[row = 4 lg + r][col = li] of each 16 x 16 tile
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int y = y0 + 2 * wv + (t >> 1);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int x = 16 * (t & 1) + 4 * lg + r;
      const size_t m = (size_t)b * kNsPix + y * 32 + x;
      if (MODE == NS_DZ) {
        float val = a.v[b * 16 + li];
        if (a.pool) val *= ns_pool_k(y) * ns_pool_k(x);
        val += acc[t][0][r];
        const float zb = a.zb[m * a.ldzb + li];
        a.out[m * 16 + li] = fmaf(a.Pb[NsPScale + li], zb, a.Pb[NsPShift + li]) > 0.0f ? val : 0.0f;
      } else {
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) a.out[m * NOUT + nb * 16 + li] = acc[t][nb][r] + a.bias[nb][li];
      }
    }
  }
}

struct NsWgrad {
  NsSrc a;             // the layer's input: NS_ACT of the layer below (CIN == 3: the image)
  NsSrc dz[2];         // the gradient w.r.t. the layer's z, 16 output channels each
  const float* v;
  float* part;         // [gridDim.x][9 CIN][NOUT]
  int nstrips;         // 4 B
};

template <int CIN, int NOUT>
__global__ __launch_bounds__(kNsThreads) void k_ns_wgrad(const NsWgrad a) {
  constexpr int CP = CIN == 3 ? 3 : 17;
  constexpr int K = 9 * CIN, RT = (K + 15) / 16;         // rows; row tiles
  constexpr int NB = NOUT / 16;
  constexpr int NIN = CIN == 3 ? kNsHalo * 3 : kNsPlane;
  __shared__ float sIn[NIN];
  __shared__ float sDz[NB * kNsDPlane];                  // (and the waves' sum [RT 16][NOUT] at the end)
  static_assert(RT * 16 * NOUT <= NB * kNsDPlane, "the waves' sum fits the dz tile");
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, lg = lane >> 4;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);

  ns_f32x4 acc[RT][NB];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[rt][nb] = ns_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  // row 16 rt + li = (tap, c_in): its offset in the halo tile
  int aoff[RT];
  bool aok[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    if constexpr (CIN == 3) {
      const int k = 16 * rt + li;
      aok[rt] = k < K;
      const int tap = aok[rt] ? k / 3 : 0, c = aok[rt] ? k - 3 * tap : 0;
      aoff[rt] = ((tap / 3) * 34 + (tap % 3)) * 3 + c;
    } else {
      aok[rt] = true;
      aoff[rt] = ((rt / 3) * 34 + (rt % 3)) * 17 + li;
    }
  }
  const int cz = tid % NOUT, grp = cz >> 4, cc = cz & 15;
  const NsSrc zs = ns_pick(a.dz[0], a.dz[1], grp);
  const NsChan zp = ns_chan<NS_DZ>(zs.P, cc);

  for (int st = blockIdx.x; st < a.nstrips; st += gridDim.x) {
    const int b = st >> 2, y0 = 8 * (st & 3);
    __syncthreads();                                      // every wave is done with the previous strip
    ns_stage_halo<CIN == 3 ? NS_RAW : NS_ACT, CIN>(sIn, a.a, a.a, a.v, b, y0);
    for (int pix = tid / NOUT; pix < kNsStrip; pix += kNsThreads / NOUT)
      sDz[grp * kNsDPlane + pix * 17 + cc] = ns_value<NS_DZ>(zs, zp, a.v, (size_t)b * kNsPix + y0 * 32 + pix, cc);
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 16; ++s) {                        // the wave's 64 pixels, 4 per step
      const int r = 2 * wv + (s >> 3), x = 4 * (s & 7) + lg;
      float bv[NB];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) bv[nb] = sDz[nb * kNsDPlane + (r * 32 + x) * 17 + li];
      const int pa = (r * 34 + x) * CP;
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        const float av = aok[rt] ? sIn[pa + aoff[rt]] : 0.0f;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[rt][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[nb], acc[rt][nb], 0, 0, 0);
      }
    }
  }

  // ---- the four waves' accumulators, added in wave order
  for (int w = 0; w < 4; ++w) {
    __syncthreads();
    if (wv == w) {
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float* q = sDz + (16 * rt + 4 * lg + r) * NOUT + nb * 16 + li;
            *q = w == 0 ? acc[rt][nb][r] : *q + acc[rt][nb][r];
          }
    }
  }
  __syncthreads();
  float* part = a.part + (size_t)blockIdx.x * K * NOUT;
  for (int e = tid; e < K * NOUT; e += kNsThreads) part[e] = sDz[e];
}

// dW = the sum of the partials [groups][K][NOUT]; column n goes to g{n >> 4}[k][n & 15].  A workgroup owns kNsWsE entries;
// eight slices of ceil(groups / 8) consecutive groups are summed in group order by eight threads per entry, then the
// slices in slice order (one thread walking 256 partials alone waits 256 dependent loads out)
constexpr int kNsWsE = 32;
__global__ __launch_bounds__(kNsThreads) void k_ns_wsum(const float* __restrict__ part, int groups, int K, int NOUT,
                                                        float* __restrict__ g0, float* __restrict__ g1) {
  __shared__ float red[kNsThreads];
  const int tid = threadIdx.x, le = tid & (kNsWsE - 1), sl = tid / kNsWsE;
  const int total = K * NOUT, e = blockIdx.x * kNsWsE + le;
  const int per = (groups + 7) / 8;
  const int z1 = min(groups, (sl + 1) * per);
  float s = 0.0f;
  if (e < total)
    for (int z = sl * per; z < z1; ++z) s += part[(size_t)z * total + e];
  red[tid] = s;
  __syncthreads();
  if (sl != 0 || e >= total) return;
  float t = red[le];
  for (int k = 1; k < 8; ++k) t += red[k * kNsWsE + le];
  const int k = e / NOUT, n = e - k * NOUT;
  (n < 16 ? g0 : g1)[k * 16 + (n & 15)] = t;
}

// ---- batch norm, forward: per-sample (mean, M2) of C channels of z [M][C]; then the merge and the layers' NsP blocks
template <int C>
__global__ __launch_bounds__(kNsThreads) void k_ns_stats(const float* __restrict__ z, float* __restrict__ part) {
  __shared__ float red[kNsThreads];
  __shared__ float msh[C];
  const int b = blockIdx.x;
  l2o::cv_sample_stats<C>(z + (size_t)b * kNsPix * C, kNsPix, red, msh, part + (size_t)b * C * 2);
}
struct NsBn {
  const float* part;       // [B][C][2]
  const float* gamma[2];   // of channels 0-15 / 16-31
  const float* beta[2];
  float* P;                // the NsP block of channels 0-15; the next block is that of channels 16-31
  int B;
};
template <int C>
__global__ __launch_bounds__(kNsThreads) void k_ns_bn(const NsBn a) {
  __shared__ float red[kNsThreads];
  __shared__ float mean[C];
  __shared__ float rstd[C];
  l2o::cv_merge_stats<C>(a.part, a.B, (float)kNsPix, red, mean, rstd);
  const int tid = threadIdx.x;
  if (tid < C) {
    const int l = tid >> 4, c = tid & 15;
    float* P = a.P + l * kNsP;
    const float gr = (l ? a.gamma[1] : a.gamma[0])[c] * rstd[tid];
    P[NsPMean + c] = mean[tid];
    P[NsPRstd + c] = rstd[tid];
    P[NsPGr + c] = gr;
    P[NsPScale + c] = gr;
    P[NsPShift + c] = fmaf(-gr, mean[tid], (l ? a.beta[1] : a.beta[0])[c]);
  }
}
// without batch norm: the identity in all four blocks
__global__ __launch_bounds__(kNsThreads) void k_ns_identity(float* __restrict__ P) {
  for (int e = threadIdx.x; e < kNsLayers * kNsP; e += kNsThreads) {
    const int f = (e % kNsP) / 16 * 16;
    P[e] = (f == NsPScale || f == NsPRstd || f == NsPGr) ? 1.0f : 0.0f;
  }
}

// ---- batch norm, backward: per-sample (sum dy, sum dy xhat) of C channels, then the sums in sample order, the two means
// of the NsP blocks and the gradients of gamma, beta and the conv bias
struct NsBwd {
  NsSrc src[2];
  const float* v;
  float* part;             // [B][C][2]
  float* P;                // as NsBn
  float* ggamma[2];        // NULL without batch norm
  float* gbeta[2];
  float* gbias[2];
  int B, bn;
};
template <int C>
__global__ __launch_bounds__(kNsThreads) void k_ns_bwd_sums(const NsBwd a) {
  __shared__ float red[2 * kNsThreads];
  constexpr int L = kNsThreads / C;
  const int tid = threadIdx.x, c = tid % C, l = tid / C, grp = c >> 4, cc = c & 15;
  const int b = blockIdx.x;
  const NsSrc s = ns_pick(a.src[0], a.src[1], grp);
  const NsChan p = ns_chan<NS_ACT>(s.P, cc);
  const float mean = s.P[NsPMean + cc], rstd = s.P[NsPRstd + cc];
  float s0 = 0.0f, s1 = 0.0f;
  for (int q = l; q < kNsPix; q += L) {
    const size_t m = (size_t)b * kNsPix + q;
    const float z = s.z[m * s.ldz + cc];
    const float d = ns_dy(s, p, a.v, m, cc, z);
    s0 += d;
    s1 = fmaf(d, (z - mean) * rstd, s1);
  }
  red[tid] = s0;
  red[kNsThreads + tid] = s1;
  __syncthreads();
  if (tid < C) {
    float t0 = 0.0f, t1 = 0.0f;
    for (int k = 0; k < L; ++k) { t0 += red[k * C + tid]; t1 += red[kNsThreads + k * C + tid]; }
    a.part[((size_t)b * C + tid) * 2] = t0;
    a.part[((size_t)b * C + tid) * 2 + 1] = t1;
  }
}
template <int C>
__global__ __launch_bounds__(kNsThreads) void k_ns_bwd_fin(const NsBwd a) {
  __shared__ float red[2 * kNsThreads];
  constexpr int L = kNsThreads / C;
  const int tid = threadIdx.x, c = tid % C, l = tid / C;
  float s0 = 0.0f, s1 = 0.0f;
  for (int b = l; b < a.B; b += L) {
    s0 += a.part[((size_t)b * C + c) * 2];
    s1 += a.part[((size_t)b * C + c) * 2 + 1];
  }
  red[tid] = s0;
  red[kNsThreads + tid] = s1;
  __syncthreads();
  if (tid < C) {
    float t0 = 0.0f, t1 = 0.0f;
    for (int k = 0; k < L; ++k) { t0 += red[k * C + tid]; t1 += red[kNsThreads + k * C + tid]; }
    const int g = tid >> 4, cc = tid & 15;
    float* P = a.P + g * kNsP;
    if (a.bn) {
      const float N = (float)kNsPix * (float)a.B;
      P[NsPM1 + cc] = t0 / N;
      P[NsPM2 + cc] = t1 / N;
      (g ? a.ggamma[1] : a.ggamma[0])[cc] = t1;
      (g ? a.gbeta[1] : a.gbeta[0])[cc] = t0;
      (g ? a.gbias[1] : a.gbias[0])[cc] = 0.0f;                              // (the analytic value: batch norm removes a per-channel shift)
    } else {
      (g ? a.gbias[1] : a.gbias[0])[cc] = t0;
    }
  }
}

// ---- the head
struct NsHead {
  const float* z0;         // [M][16]
  const float* zz;         // [M][32]: n02, node1
  const float* z13;        // [M][16]
  const float* P;          // the four NsP blocks
  const float* wfc;        // [16][10]
  const float* bfc;        // [10]
  const int32_t* labels;
  const int32_t* idx;
  float* nf;               // [B][16]
  float* dlog;             // [B][16] dL/dout (the 1 / B and the logits' ReLU mask included); entries 10..15 are 0
  float* v;                // [B][16] dL/dnf / 1024
  float* loss_s;           // [B]
  float* loss;
  float* gwfc;
  float* gbfc;
  int B, n_data;
};
// one workgroup per sample: nf = the mean over the positions of k k node1 + n02 + n13 + node0 (16 lanes per channel, each
// its 64 positions in order, then the lanes in order), fc, ReLU, the cross-entropy, and dL/dnf
__global__ __launch_bounds__(kNsThreads) void k_ns_head(const NsHead h) {
  __shared__ float red[kNsThreads];
  __shared__ float snf[16];
  __shared__ float sd[16];
  const int tid = threadIdx.x, c = tid & 15, l = tid >> 4, b = blockIdx.x;
  const NsChan p0 = ns_chan<NS_ACT>(h.P, c), p02 = ns_chan<NS_ACT>(h.P + kNsP, c);
  const NsChan p1 = ns_chan<NS_ACT>(h.P + 2 * kNsP, c), p13 = ns_chan<NS_ACT>(h.P + 3 * kNsP, c);
  float s = 0.0f;
  for (int q = l; q < kNsPix; q += 16) {
    const size_t m = (size_t)b * kNsPix + q;
    const float a0 = fmaxf(fmaf(p0.scale, h.z0[m * 16 + c], p0.shift), 0.0f);
    const float a02 = fmaxf(fmaf(p02.scale, h.zz[m * 32 + c], p02.shift), 0.0f);
    const float a1 = fmaxf(fmaf(p1.scale, h.zz[m * 32 + 16 + c], p1.shift), 0.0f);
    const float a13 = fmaxf(fmaf(p13.scale, h.z13[m * 16 + c], p13.shift), 0.0f);
    s += fmaf(ns_pool_k(q >> 5) * ns_pool_k(q & 31), a1, (a02 + a13) + a0);
  }
  red[tid] = s;
  __syncthreads();
  if (tid < 16) {
    float t = 0.0f;
    for (int k = 0; k < 16; ++k) t += red[k * 16 + tid];
    t *= 1.0f / (float)kNsPix;
    snf[tid] = t;
    h.nf[b * 16 + tid] = t;
  }
  __syncthreads();
  if (tid == 0) {
    const int row = min(max(h.idx[b], 0), h.n_data - 1);
    const int label = h.labels[row];
    float o[kNsClasses], e[kNsClasses];
    float omax = 0.0f;
    for (int j = 0; j < kNsClasses; ++j) {
      float t = 0.0f;
      for (int k = 0; k < 16; ++k) t = fmaf(snf[k], h.wfc[k * kNsClasses + j], t);
      o[j] = fmaxf(t + h.bfc[j], 0.0f);
      omax = fmaxf(omax, o[j]);
    }
    float es = 0.0f, olabel = 0.0f;
    for (int j = 0; j < kNsClasses; ++j) { e[j] = expf(o[j] - omax); es += e[j]; if (j == label) olabel = o[j]; }
    h.loss_s[b] = logf(es) - (olabel - omax);
    const float inv_b = 1.0f / (float)h.B;
    for (int j = 0; j < 16; ++j) {
      float d = 0.0f;
      if (j < kNsClasses && o[j] > 0.0f) d = (e[j] / es - (j == label ? 1.0f : 0.0f)) * inv_b;
      sd[j] = d;
      h.dlog[b * 16 + j] = d;
    }
  }
  __syncthreads();
  if (tid < 16) {
    float u = 0.0f;
    for (int j = 0; j < kNsClasses; ++j) u = fmaf(h.wfc[tid * kNsClasses + j], sd[j], u);
    h.v[b * 16 + tid] = u * (1.0f / (float)kNsPix);
  }
}
// the mean loss (a fixed tree over the samples); with gradients (gwfc != NULL) fc_weights' gradient nf^T dlog and
// fc_bias', sums over the samples in sample order
__global__ __launch_bounds__(kNsThreads) void k_ns_head_sum(const NsHead h) {
  __shared__ float red[kNsThreads];
  const int tid = threadIdx.x;
  float s = 0.0f;
  for (int b = tid; b < h.B; b += kNsThreads) s += h.loss_s[b];
  red[tid] = s;
  __syncthreads();
  for (int w = kNsThreads / 2; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  if (tid == 0) h.loss[0] = red[0] / (float)h.B;
  if (!h.gwfc) return;
  if (tid < 16 * kNsClasses) {
    const int c = tid / kNsClasses, j = tid - c * kNsClasses;
    float t = 0.0f;
    for (int b = 0; b < h.B; ++b) t = fmaf(h.nf[b * 16 + c], h.dlog[b * 16 + j], t);
    h.gwfc[tid] = t;
  } else if (tid < 16 * kNsClasses + kNsClasses) {
    const int j = tid - 16 * kNsClasses;
    float t = 0.0f;
    for (int b = 0; b < h.B; ++b) t += h.dlog[b * 16 + j];
    h.gbfc[j] = t;
  }
}
