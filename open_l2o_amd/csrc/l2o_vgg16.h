// l2o_vgg16.h -- problems.vgg16_cifar10 (DM/problems.py:637-694, DM/vgg16.py): VGG-16 on CIFAR-10 without batch norm,
// loss and gradients of one minibatch.  Included by l2o_nets.hip (host side: l2o_vgg16_fg there).
//
// Thirteen 3x3 SAME convolutions in five blocks of (2, 2, 3, 3, 3) layers, ReLU after each, max-pool 2x2 after each block,
// then linear x10, softmax, and a softmax cross-entropy that takes the probabilities as logits.  Activations NHWC, weights
// HWIO = the row-major [9 C_in][C_out] GEMM operand.  Everything GEMM-shaped is ONE kernel template, k_vg_gemm<MODE>, an
// implicit GEMM C[r][n] = sum_q A(r, q) B(q, n) on v_mfma_f32_32x32x2_f32 (exact fp32: a q-ordered fmaf chain), with the
// zero padding done in the gather (no im2col in memory):
//   VG_FWD    r = pixel m (of B H W), q = k = (tap, c_in), n = c_out:  A = x gathered, B = w;  bias + ReLU in the epilogue
//   VG_DGRAD  r = pixel m, q = (tap, c_out), n = c_in:  A = dy gathered, B = w read flipped (tap -> 8 - tap) and transposed;
//             the epilogue applies the ReLU mask of the layer below (its stored output > 0) where there is one
//   VG_WGRAD  r = k = (tap, c_in), q = pixel m, n = c_out:  A = x gathered (transposed), B = dy;  the reduction over the
//             B H W pixels is split over gridDim.z, every split writes its partial [9 C_in + 1][C_out] -- the last row is
//             the bias gradient's partial, the column sums of the dy values the row-tile-0 workgroups stage anyway -- and
//             k_vg_wsum adds the partials in split order
// A workgroup is 4 waves on a 64 x 64 tile (a 32 x 32 accumulator per wave), 32 reduction indices per LDS tile, the next
// tile's operands fetched into registers while this one is multiplied.  `dy` is always the gradient w.r.t. a layer's
// PRE-activation (ReLU mask applied), so a layer's backward is wgrad + dgrad and nothing else.
// Only the post-ReLU activations are kept (the mask is y > 0 and the pool's arg-max is recomputed from them: first
// candidate in row-major window order, strict >, as torch; a window of four zeros routes to the first candidate and the
// mask zeroes it).
#pragma once
#include "l2o_common.h"
#include "../../include/l2o_vgg16_abi.h"

constexpr int kVgLayers = 13;             // conv layers
constexpr int kVgMaxBatch = 1024;
constexpr int kVgClasses = 10;
constexpr int kVgBM = 64, kVgBN = 64, kVgBK = 32;   // workgroup tile: rows, columns, reduction indices per LDS tile
constexpr int kVgLd = 65;                 // LDS row stride (odd: the k-fast writes of the gathered operand spread over the banks)
constexpr int kVgThreads = 256;
constexpr int VG_FWD = 0, VG_DGRAD = 1, VG_WGRAD = 2;

typedef float vg_f32x16 __attribute__((ext_vector_type(16)));

// one conv layer of the plan: its input is lw-sized (W = H = 1 << lw) with cin channels; pool: a max-pool follows it
struct VgLayer {
  int lw, cin, cout, pool;
};
inline void vg_plan(const int32_t* channels, VgLayer* L) {
  const int per_block[5] = {2, 2, 3, 3, 3};
  int l = 0, cin = 3;
  for (int b = 0; b < 5; ++b)
    for (int i = 0; i < per_block[b]; ++i, ++l) {
      L[l].lw = 5 - b; L[l].cin = cin; L[l].cout = channels[b]; L[l].pool = (i == per_block[b] - 1);
      cin = channels[b];
    }
}
// the split of a weight gradient's reduction over the B H W pixels: a function of the shape alone.  `per` reduction tiles
// (of kVgBK pixels) per split, at least 8, aiming at >= 1024 workgroups; returns the number of splits
inline int vg_wgrad_splits(int batch, const VgLayer& L, int* per_out) {
  const long M = (long)batch << (2 * L.lw);
  const int qtiles = (int)((M + kVgBK - 1) / kVgBK);
  const int tiles = ((9 * L.cin + kVgBM - 1) / kVgBM) * ((L.cout + kVgBN - 1) / kVgBN);
  int splits = 1024 / tiles;
  if (splits > qtiles / 8) splits = qtiles / 8;
  if (splits < 1) splits = 1;
  const int per = (qtiles + splits - 1) / splits;
  *per_out = per;
  return (qtiles + per - 1) / per;
}

struct VgGemm {
  const float* a;     // the gathered operand: FWD / WGRAD x [M][cin], DGRAD dy [M][cout]
  const float* b;     // FWD / DGRAD w [9 cin][cout], WGRAD dy [M][cout]
  const float* aux;   // FWD bias [cout]; DGRAD the stored output of the layer below [M][cin] (its ReLU mask) or NULL
  float* out;         // FWD y [M][cout]; DGRAD dx [M][cin]; WGRAD partials [splits][9 cin + 1][cout]
  int M, lw, cin, cout, per;
};

template <int MODE>
__global__ __launch_bounds__(kVgThreads) void k_vg_gemm(const VgGemm g) {
  __shared__ float sA[kVgBK * kVgLd];
  __shared__ float sB[kVgBK * kVgLd];
  __shared__ float sBias[4 * kVgBN];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int M = g.M, lw = g.lw, W = 1 << lw, cin = g.cin, cout = g.cout;
  const int K9 = 9 * cin;
  // rows, columns, reduction length and the channel count of the gathered array
  const int R = MODE == VG_WGRAD ? K9 : M;
  const int N = MODE == VG_DGRAD ? cin : cout;
  const int Cg = MODE == VG_DGRAD ? cout : cin;
  const int Q = MODE == VG_WGRAD ? M : 9 * Cg;
  const int r0 = blockIdx.x * kVgBM, n0 = blockIdx.y * kVgBN;
  int q_begin = 0, q_end = Q;
  if (MODE == VG_WGRAD) {
    q_begin = blockIdx.z * g.per * kVgBK;
    q_end = min(Q, q_begin + g.per * kVgBK);
  }
  const float* __restrict__ ga = g.a;
  const float* __restrict__ gb = g.b;

  // the value of the gathered array that pixel m sees through tap (dy, dx) at channel c: 0 outside the image
  auto gather = [&](int m, int dy, int dx, int c) -> float {
    const int y = (m >> lw) & (W - 1), x = m & (W - 1);
    const bool ok = (unsigned)(y + dy) < (unsigned)W && (unsigned)(x + dx) < (unsigned)W;
    return ok ? ga[(size_t)(m + dy * W + dx) * Cg + c] : 0.0f;
  };

  float ra[8], rb[8];
  float bsum = 0.0f;
  const int f32 = tid & 31, s32 = tid >> 5;     // the (fast 32, slow 8) thread map
  const int f64 = tid & 63, s64 = tid >> 6;     // the (fast 64, slow 4) thread map
  // WGRAD: this thread's row k = (tap, c) is the same for every tile
  int wk_c = 0, wk_dy = 0, wk_dx = 0;
  bool wk_ok = false;
  if (MODE == VG_WGRAD) {
    const int k = r0 + f64;
    wk_ok = k < R;
    const int tap = k / cin;
    wk_c = k - tap * cin; wk_dy = tap / 3 - 1; wk_dx = tap - 3 * (tap / 3) - 1;
  }
  auto fetch = [&](int q0) {
    if (MODE == VG_WGRAD) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int m = q0 + s64 + 4 * j;
        const bool in = m < q_end;
        ra[j] = (in && wk_ok) ? gather(m, wk_dy, wk_dx, wk_c) : 0.0f;
        rb[j] = (in && n0 + f64 < N) ? gb[(size_t)m * cout + n0 + f64] : 0.0f;
      }
    } else {
      const int k = q0 + f32;
      const bool kok = k < Q;
      const int tap = k / Cg, c = k - tap * Cg;
      const int dy = tap / 3 - 1, dx = tap - 3 * (tap / 3) - 1;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int m = r0 + s32 + 8 * j;
        ra[j] = (kok && m < M) ? gather(m, dy, dx, c) : 0.0f;
      }
      if (MODE == VG_FWD) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int kb = q0 + s64 + 4 * j;
          rb[j] = (kb < Q && n0 + f64 < N) ? gb[(size_t)kb * cout + n0 + f64] : 0.0f;
        }
      } else {                                  // w flipped and transposed: B(q = (tap, co), n = ci) = w[8 - tap][ci][co]
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int ci = n0 + s32 + 8 * j;
          rb[j] = (kok && ci < N) ? gb[((size_t)(8 - tap) * cin + ci) * cout + c] : 0.0f;
        }
      }
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (MODE == VG_WGRAD) {
        sA[(s64 + 4 * j) * kVgLd + f64] = ra[j];
        sB[(s64 + 4 * j) * kVgLd + f64] = rb[j];
        bsum += rb[j];                          // (read only by the row-tile-0 workgroups)
      } else {
        sA[f32 * kVgLd + s32 + 8 * j] = ra[j];
        if (MODE == VG_FWD) sB[(s64 + 4 * j) * kVgLd + f64] = rb[j];
        else sB[f32 * kVgLd + s32 + 8 * j] = rb[j];
      }
    }
  };

  vg_f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
  const int wm = wv & 1, wn = wv >> 1;
  const float* pa = sA + (lane >> 5) * kVgLd + 32 * wm + (lane & 31);
  const float* pb = sB + (lane >> 5) * kVgLd + 32 * wn + (lane & 31);
  if (q_begin < q_end) fetch(q_begin);
  for (int q0 = q_begin; q0 < q_end; q0 += kVgBK) {
    __syncthreads();                            // every wave is done with the previous tile
    stage();
    __syncthreads();
    if (q0 + kVgBK < q_end) fetch(q0 + kVgBK);  // in flight while this tile is multiplied
#pragma unroll
    for (int s = 0; s < kVgBK / 2; ++s)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[2 * s * kVgLd], pb[2 * s * kVgLd], acc, 0, 0, 0);
  }

  // ---- epilogue: D[row = (i & 3) + 8 (i >> 2) + 4 (lane >> 5)][col = lane & 31] of the wave's 32 x 32 tile
  const int n = n0 + 32 * wn + (lane & 31);
  if (MODE == VG_WGRAD) {
    float* part = g.out + (size_t)blockIdx.z * (K9 + 1) * cout;
    if (blockIdx.x == 0) {                      // the bias gradient's partial: column sums of this split's dy rows
      sBias[s64 * kVgBN + f64] = bsum;
      __syncthreads();
      if (s64 == 0 && n0 + f64 < N)
        part[(size_t)K9 * cout + n0 + f64] = ((sBias[f64] + sBias[kVgBN + f64]) + sBias[2 * kVgBN + f64]) + sBias[3 * kVgBN + f64];
    }
    if (n < N) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int r = r0 + 32 * wm + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
        if (r < R) part[(size_t)r * cout + n] = acc[i];
      }
    }
  } else if (n < N) {
    const float bias = MODE == VG_FWD ? g.aux[n] : 0.0f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int r = r0 + 32 * wm + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
      if (r < R) {
        float v = acc[i];
        if (MODE == VG_FWD) v = fmaxf(v + bias, 0.0f);
        else if (g.aux) v = g.aux[(size_t)r * N + n] > 0.0f ? v : 0.0f;
        g.out[(size_t)r * N + n] = v;
      }
    }
  }
}

// dW[e] (e < nW) and db[e - nW] = the sum over the splits, in split order, of the partials [splits][nW + cout]
__global__ __launch_bounds__(kVgThreads) void k_vg_wsum(const float* __restrict__ part, int splits, int nW, int cout,
                                                        float* __restrict__ dW, float* __restrict__ db) {
  const int e = blockIdx.x * kVgThreads + threadIdx.x;
  const int total = nW + cout;
  if (e >= total) return;
  float s = 0.0f;
  for (int z = 0; z < splits; ++z) s += part[(size_t)z * total + e];
  if (e < nW) dW[e] = s;
  else db[e - nW] = s;
}

// the minibatch's images, gathered: x0[b] = images[indices[b]] (an index outside the data set is clamped into it)
__global__ __launch_bounds__(kVgThreads) void k_vg_gather(const float* __restrict__ images, const int32_t* __restrict__ idx,
                                                          int n_data, float* __restrict__ x0) {
  const int b = blockIdx.x;
  const int row = min(max(idx[b], 0), n_data - 1);
  const float4* src = reinterpret_cast<const float4*>(images + (size_t)row * 3072);
  float4* dst = reinterpret_cast<float4*>(x0 + (size_t)b * 3072);
  for (int e = threadIdx.x; e < 768; e += kVgThreads) dst[e] = src[e];
}

// max-pool 2x2 stride 2 of a [B][W][W][C] array (W = 1 << lw): out [B][W/2][W/2][C]; `total` = B (W/2)^2 C
__global__ __launch_bounds__(kVgThreads) void k_vg_pool(const float* __restrict__ a, float* __restrict__ out, int lw, int C,
                                                        size_t total) {
  const size_t e = (size_t)blockIdx.x * kVgThreads + threadIdx.x;
  if (e >= total) return;
  const int W = 1 << lw, Wo = W >> 1;
  const size_t p = e / C;                      // pooled pixel (b, yo, xo)
  const int c = (int)(e - p * C);
  const int xo = (int)(p & (Wo - 1)), yo = (int)((p >> (lw - 1)) & (Wo - 1));
  const size_t b = p >> (2 * (lw - 1));
  const float* q = a + (((b << lw) + 2 * yo) * W + 2 * xo) * C + c;
  out[e] = fmaxf(fmaxf(q[0], q[C]), fmaxf(q[(size_t)W * C], q[(size_t)W * C + C]));
}

// max-pool backward + the ReLU mask of the layer that fed the pool: dy[b][y][x][c] = dout of its window if (y, x) is the
// window's first maximum and a > 0, else 0.  Every entry of dy is written.
__global__ __launch_bounds__(kVgThreads) void k_vg_pool_bwd(const float* __restrict__ a, const float* __restrict__ dout,
                                                            float* __restrict__ dy, int lw, int C, size_t total) {
  const size_t e = (size_t)blockIdx.x * kVgThreads + threadIdx.x;
  if (e >= total) return;
  const int W = 1 << lw, Wo = W >> 1;
  const size_t p = e / C;
  const int c = (int)(e - p * C);
  const int xo = (int)(p & (Wo - 1)), yo = (int)((p >> (lw - 1)) & (Wo - 1));
  const size_t b = p >> (2 * (lw - 1));
  const size_t base = (((b << lw) + 2 * yo) * W + 2 * xo) * C + c;
  const size_t off[4] = {0, (size_t)C, (size_t)W * C, (size_t)W * C + C};
  int best = 0;
  float vb = a[base];
#pragma unroll
  for (int i = 1; i < 4; ++i) {
    const float v = a[base + off[i]];
    if (v > vb) { vb = v; best = i; }
  }
  const float gv = vb > 0.0f ? dout[e] : 0.0f;
#pragma unroll
  for (int i = 0; i < 4; ++i) dy[base + off[i]] = i == best ? gv : 0.0f;
}

struct VgHead {
  const float* a13;        // [B][2][2][C] the last conv layer's output
  const float* wfc;        // [C][10]
  const float* bfc;        // [10]
  const int32_t* labels;
  const int32_t* idx;
  float* pooled;           // [B][C]
  float* dz;               // [B][16]: dL/dz (the 1 / B included); entries 10..15 are 0
  float* loss_s;           // [B]
  float* dy13;             // [B][2][2][C] gradient w.r.t. the last conv layer's pre-activation, or NULL (forward only)
  float* loss;
  float* gwfc;
  float* gbfc;
  int B, C, n_data;
};

// one wave per sample: pool 5, the linear layer, softmax, the cross-entropy on the probabilities, dL/dz through both
// softmaxes, and (with gradients) the way back through the linear layer and pool 5 to the last conv layer
__global__ __launch_bounds__(64) void k_vg_head(const VgHead h) {
  __shared__ float sp[512];
  __shared__ float sz[64 * kVgClasses];
  __shared__ float sd[16];
  const int b = blockIdx.x, lane = threadIdx.x, C = h.C;
  const float* a = h.a13 + (size_t)b * 4 * C;
  float part[kVgClasses];
#pragma unroll
  for (int j = 0; j < kVgClasses; ++j) part[j] = 0.0f;
  for (int c = lane; c < C; c += 64) {
    const float p = fmaxf(fmaxf(a[c], a[C + c]), fmaxf(a[2 * C + c], a[3 * C + c]));
    sp[c] = p;
    h.pooled[(size_t)b * C + c] = p;
#pragma unroll
    for (int j = 0; j < kVgClasses; ++j) part[j] = fmaf(p, h.wfc[c * kVgClasses + j], part[j]);
  }
#pragma unroll
  for (int j = 0; j < kVgClasses; ++j) sz[lane * kVgClasses + j] = part[j];
  __syncthreads();
  if (lane < 16) {
    float z = 0.0f;
    if (lane < kVgClasses) {
      for (int l = 0; l < 64; ++l) z += sz[l * kVgClasses + lane];
      z += h.bfc[lane];
    }
    sd[lane] = z;
  }
  __syncthreads();
  if (lane == 0) {
    const int row = min(max(h.idx[b], 0), h.n_data - 1);
    const int label = h.labels[row];
    float z[kVgClasses], p[kVgClasses], q[kVgClasses];
    float zmax = sd[0];
    for (int j = 1; j < kVgClasses; ++j) zmax = fmaxf(zmax, sd[j]);
    float zs = 0.0f;
    for (int j = 0; j < kVgClasses; ++j) { z[j] = expf(sd[j] - zmax); zs += z[j]; }
    float pmax = 0.0f;
    for (int j = 0; j < kVgClasses; ++j) { p[j] = z[j] / zs; pmax = fmaxf(pmax, p[j]); }
    float qs = 0.0f, plabel = 0.0f;
    for (int j = 0; j < kVgClasses; ++j) { q[j] = expf(p[j] - pmax); qs += q[j]; if (j == label) plabel = p[j]; }
    h.loss_s[b] = logf(qs) - (plabel - pmax);
    // dL/dp = (softmax(p) - onehot) / B;  dL/dz = p (dL/dp - sum_j dL/dp_j p_j)
    const float inv_b = 1.0f / (float)h.B;
    float dp[kVgClasses], s = 0.0f;
    for (int j = 0; j < kVgClasses; ++j) {
      dp[j] = (q[j] / qs - (j == label ? 1.0f : 0.0f)) * inv_b;
      s = fmaf(dp[j], p[j], s);
    }
    for (int j = 0; j < 16; ++j) {
      const float d = j < kVgClasses ? p[j] * (dp[j] - s) : 0.0f;
      sd[j] = d;
      h.dz[(size_t)b * 16 + j] = d;
    }
  }
  __syncthreads();
  if (!h.dy13) return;
  float* dy = h.dy13 + (size_t)b * 4 * C;
  for (int c = lane; c < C; c += 64) {
    float gp = 0.0f;
#pragma unroll
    for (int j = 0; j < kVgClasses; ++j) gp = fmaf(h.wfc[c * kVgClasses + j], sd[j], gp);
    int best = 0;
    float vb = a[c];
#pragma unroll
    for (int i = 1; i < 4; ++i) {
      const float v = a[i * C + c];
      if (v > vb) { vb = v; best = i; }
    }
    const float gv = vb > 0.0f ? gp : 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) dy[i * C + c] = i == best ? gv : 0.0f;
  }
}

// block 0: the mean loss (a fixed tree over the samples).  With gradients, blocks 1..: fc/weights' gradient pooled^T dz and
// (the last block) fc/biases' gradient, sums over the samples in sample order
__global__ __launch_bounds__(kVgThreads) void k_vg_head_sum(const VgHead h) {
  __shared__ float red[kVgThreads];
  const int tid = threadIdx.x;
  if (blockIdx.x == 0) {
    float s = 0.0f;
    for (int b = tid; b < h.B; b += kVgThreads) s += h.loss_s[b];
    red[tid] = s;
    __syncthreads();
    for (int w = kVgThreads / 2; w > 0; w >>= 1) {
      if (tid < w) red[tid] += red[tid + w];
      __syncthreads();
    }
    if (tid == 0) h.loss[0] = red[0] / (float)h.B;
    return;
  }
  const int e = (blockIdx.x - 1) * kVgThreads + tid;
  const int nW = h.C * kVgClasses;
  if (e < nW) {
    const int c = e / kVgClasses, j = e - c * kVgClasses;
    float s = 0.0f;
    for (int b = 0; b < h.B; ++b) s = fmaf(h.pooled[(size_t)b * h.C + c], h.dz[(size_t)b * 16 + j], s);
    h.gwfc[e] = s;
  } else if (e < nW + kVgClasses) {
    const int j = e - nW;
    float s = 0.0f;
    for (int b = 0; b < h.B; ++b) s += h.dz[(size_t)b * 16 + j];
    h.gbfc[j] = s;
  }
}
