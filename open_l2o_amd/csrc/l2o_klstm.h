// l2o_klstm.h -- KernelDeepLSTM (DM/networks.py:303-351): one LSTM per (c_in, c_out) convolution filter.  A variable
// [kw, kh, c_in, c_out] is, in memory, a [K = kw kh][N = c_in c_out] matrix: row j = a kh + b the patch position, column
// n = ci c_out + co the filter.  The net of filter n reads the K gradients of its patch at once (identity), or their 2K
// LogAndSign features (column 2j: max(log|g| / k, -1), column 2j + 1: clip(g e^k, -1, 1)), and emits the K updates.
//
// k_klstm_step, the forward step.  One 64-lane wave per 16 filters; lane (c, q) = (lane & 15, lane >> 4) owns the hidden
// units u = 4 t + q of filter n0 + c in every layer.  The gate pre-activations z = [x, h] w_gates + b_gates run TRANSPOSED
// on the matrix cores with the exact-fp32 v_mfma_f32_16x16x4_f32 (l2o_common.h: mfma16), the project's tile convention:
//     D[rho][c] += A[rho][k] B[k][c]     A: 16 gate columns of w_gates (from LDS), B: the activations of the 16 filters
// The gate columns of tile t are permuted so that row rho = 4 q + r is gate r (i, j, f, o) of unit 4 t + q: after the last
// k-step every lane holds the four gates of the units it owns, and the h it computes is the B operand (k = 4 kk + q) of the
// next layer and the next step.  4 H gate columns = H / 4 tiles (H a multiple of 4); the reduction runs over the input
// padded with zero rows to a multiple of 4, then over H.  The weights are staged once per workgroup in LDS, in fragment order
// (conflict-free reads); the workgroup's four waves then walk the 16-filter tiles with a grid stride, so the staging is
// amortised over N / (64 gridDim) tiles.  Gates, cell update and the K-wide Linear head are fp32 VALU (accurate expf /
// tanhf / logf: the recurrent state is compared with float64 at the 1e-6 level); the head's sum over the four q lanes of a
// filter is an xor butterfly, whose result is the same bits in all four lanes.
// State (l2o_klstm_state_floats): unit-major, per layer h [H][N] then c [H][N] -- lanes over n coalesce.  state_in may be
// state_out (a lane reads what it owns before it writes it).  No atomics; rows past N load nothing and store nothing.
//
// k_klstm_bwd_step, one BPTT step of the first-order meta-gradient (g_t is a constant: nothing flows into the
// preprocessing).  One thread per filter, fp32 VALU, weights through the scalar unit: the contract of k_cwlstm_generic_bwd
// (l2o_generic.h) with a K-wide dd and the unit-major state / carry layout.  It recomputes the step from the state before
// it and emits act_l [N][in_l + H_l], dz_l [N][4 H_l], h_last [N][H_L], dd [N][K]; the host contracts them (l2o_atb /
// l2o_colsum).  Until the backward sweep overwrites them, dz_l holds the gate activations and tc [sum H][N] tanh(c').
// Included by l2o_bwd.hip.
#pragma once
#include "l2o_common.h"

namespace l2o {

constexpr int kKlMaxL = 2;
constexpr int kKlMaxH = 32;
constexpr int kKlMaxK = 49;                // 7 x 7
constexpr int kKlWaves = 4;
constexpr int kKlThreads = 64 * kKlWaves;
constexpr int kKlMaxBlocks = 1024;

struct KlParams {
  int K, in, in_pad, n_layers, H[kKlMaxL], pre, tanh_output;
  float scale, k_inv, exp_k;
  const float* wg[kKlMaxL];
  const float* bg[kKlMaxL];
  const float *wl, *bl;
  const float* g;          // [K][N]
  const float* st_in;
  float* st_out;
  float* x;                // [K][N] in-out
  long N;
  int ntiles;
};

// LDS floats of k_klstm_step: per layer the weight fragments [(in_pad_l + H_l) / 4][H_l / 4][64] and the bias fragments
// [H_l / 4][4][4], then w_lin [H_L][K] and b_lin [K] -- kl_weight_floats -- and per wave the B operands of its tile,
// [in_pad / 4 + 3 * max H / 4][64]: the input features, h(t-1) of the layer at hand, and h(t) of the two layers
__host__ __device__ inline int kl_weight_floats(const KlParams& p) {
  int n = 0, inp = p.in_pad;
  for (int l = 0; l < p.n_layers; ++l) { n += (inp + p.H[l]) * 4 * p.H[l] + 4 * p.H[l]; inp = p.H[l]; }
  return (n + p.H[p.n_layers - 1] * p.K + p.K + 3) / 4 * 4;
}
__host__ __device__ inline int kl_max_nt(const KlParams& p) {
  int m = 0;
  for (int l = 0; l < p.n_layers; ++l) m = p.H[l] / 4 > m ? p.H[l] / 4 : m;
  return m;
}
__host__ __device__ inline int kl_lds_floats(const KlParams& p) {
  return kl_weight_floats(p) + kKlWaves * (p.in_pad / 4 + 3 * kl_max_nt(p)) * 64;
}

__device__ __forceinline__ float kl_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

__device__ __forceinline__ float kl_feature(const KlParams& p, int k, bool live, long n) {
  if (k >= p.in || !live) return 0.0f;
  if (p.pre == L2O_PRE_LOGSIGN) {                            // DM/preprocess.py:63-70, the pairs interleaved
    const float gv = p.g[(long)(k >> 1) * p.N + n];
    return (k & 1) ? fminf(fmaxf(gv * p.exp_k, -1.0f), 1.0f)
                   : fmaxf(logf(fabsf(gv) + 1.1920928955078125e-07f) * p.k_inv, -1.0f);
  }
  return p.g[(long)k * p.N + n];
}

// Every loop below has a run-time trip count and the operands of the matrix products come from LDS, so the register
// footprint does not depend on (K, H): the B operands of a tile sit in the wave's own LDS rows, each word written and read
// by the same lane (an indexable register file: no barrier).
__global__ __launch_bounds__(kKlThreads) void k_klstm_step(KlParams p) {
  extern __shared__ float kl_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, q = lane >> 4;
  // ---- stage the weights: fragment order, gate columns permuted, the input rows padded with zeros to a multiple of 4
  {
    float* at = kl_lds;
    int inw = p.in, inp = p.in_pad;
    for (int l = 0; l < p.n_layers; ++l) {
      const int H = p.H[l], G = 4 * H, nt = H / 4, total = (inp + H) * G;
      const float* w = p.wg[l];
      for (int i = tid; i < total; i += kKlThreads) {
        const int ln = i & 63, s = i >> 6, t = s % nt, kk = s / nt;
        const int rho = ln & 15, k = 4 * kk + (ln >> 4);
        const int col = (rho & 3) * H + 4 * t + (rho >> 2);
        float v = 0.0f;
        if (k < inw) v = w[k * G + col];
        else if (k >= inp) v = w[(inw + k - inp) * G + col];
        at[i] = v;
      }
      at += total;
      for (int i = tid; i < G; i += kKlThreads) at[i] = p.bg[l][(i & 3) * H + 4 * (i >> 4) + ((i >> 2) & 3)];
      at += G;
      inw = inp = H;
    }
    const int HL = p.H[p.n_layers - 1];
    for (int i = tid; i < HL * p.K; i += kKlThreads) at[i] = p.wl[i];
    for (int i = tid; i < p.K; i += kKlThreads) at[HL * p.K + i] = p.bl[i];
  }
  const int HL = p.H[p.n_layers - 1], mnt = kl_max_nt(p), nkx = p.in_pad / 4;
  float* bx = kl_lds + kl_weight_floats(p) + wave * (nkx + 3 * mnt) * 64 + lane;   // features: bx[kk * 64]
  float* bh = bx + nkx * 64;                                                        // h(t-1) of the layer: bh[kk * 64]
  __syncthreads();
  // ---- the wave's tiles (no barrier below: the waves may leave at different times)
  for (int tile = blockIdx.x * kKlWaves + wave; tile < p.ntiles; tile += gridDim.x * kKlWaves) {
    const long n = (long)tile * 16 + c;
    const bool live = n < p.N;
    for (int kk = 0; kk < nkx; ++kk) bx[kk * 64] = kl_feature(p, 4 * kk + q, live, n);
    const float* wf = kl_lds;
    const float* bin = bx;                                   // the B operands of the layer's input part
    int nk_in = nkx;
    long off = 0;
    for (int l = 0; l < p.n_layers; ++l) {
      const int H = p.H[l], nt = H / 4;
      const float* sin = p.st_in + off * p.N;
      float* sout = p.st_out + off * p.N;
      const float* bf = wf + (nk_in + nt) * nt * 64;
      float* bn = bh + (1 + (l & 1)) * mnt * 64;             // h(t) of the layer: bn[t * 64]
      // all of h(t-1) is read before any of h(t) is stored: state_in may be state_out
      for (int kk = 0; kk < nt; ++kk) bh[kk * 64] = live ? sin[(long)(4 * kk + q) * p.N + n] : 0.0f;
      // two gate tiles at a time (two independent accumulator chains); an odd last one is computed twice, stored once
      for (int t0 = 0; t0 < nt; t0 += 2) {
        const int t1 = t0 + 1 < nt ? t0 + 1 : t0;
        f32x4 a0 = *reinterpret_cast<const f32x4*>(bf + (t0 * 4 + q) * 4);
        f32x4 a1 = *reinterpret_cast<const f32x4*>(bf + (t1 * 4 + q) * 4);
        const float* w0 = wf + t0 * 64 + lane;
        const float* w1 = wf + t1 * 64 + lane;
        for (int kk = 0; kk < nk_in; ++kk) {
          const float b = bin[kk * 64];
          a0 = mfma16(w0[kk * nt * 64], b, a0);
          a1 = mfma16(w1[kk * nt * 64], b, a1);
        }
        for (int kk = 0; kk < nt; ++kk) {
          const float b = bh[kk * 64];
          a0 = mfma16(w0[(nk_in + kk) * nt * 64], b, a0);
          a1 = mfma16(w1[(nk_in + kk) * nt * 64], b, a1);
        }
        // snt.LSTM on the four gates (i, j, f, o) the lane holds of unit 4 t + q
        for (int half = 0; half < 2; ++half) {
          const int t = half ? t1 : t0;
          if (half && t1 == t0) break;
          const f32x4 z = half ? a1 : a0;
          const float cp = live ? sin[(long)(H + 4 * t + q) * p.N + n] : 0.0f;
          const float cn = kl_sigmoid(z[2] + 1.0f) * cp + kl_sigmoid(z[0]) * tanhf(z[1]);
          const float hn = tanhf(cn) * kl_sigmoid(z[3]);
          bn[t * 64] = hn;
          if (live) {
            sout[(long)(4 * t + q) * p.N + n] = hn;
            sout[(long)(H + 4 * t + q) * p.N + n] = cn;
          }
        }
      }
      wf = bf + 4 * H;
      nk_in = nt;
      bin = bn;                                              // this layer's h(t) feeds the next (its h(t-1) rows are free)
      off += 2 * H;
    }
    // ---- Linear(H_L -> K), (tanh) * scale, x += delta; h_L(t) is in bin[t * 64]
    const float* wl = wf;
    const float* bl = wl + HL * p.K;
    for (int j = 0; j < p.K; ++j) {
      float s = 0.0f;
      for (int t = 0; t < HL / 4; ++t) s = __builtin_fmaf(bin[t * 64], wl[(4 * t + q) * p.K + j], s);
      s += __shfl_xor(s, 16);
      s += __shfl_xor(s, 32);
      s += bl[j];
      if (p.tanh_output) s = tanhf(s);
      if (live && q == (j & 3)) p.x[(long)j * p.N + n] += s * p.scale;
    }
  }
}

// ---------------------------------------------------------------------------
constexpr int kKlBwdThreads = 64;
constexpr int kKlBwdRow = 2 * kKlMaxK + kKlMaxH + 1;         // [features (<= 98) | h_prev (<= 32)], odd stride

struct KlBwdParams {
  int K, in, n_layers, H[kKlMaxL], pre, tanh_output;
  float scale, k_inv, exp_k;
  const float* wg[kKlMaxL];
  const float* bg[kKlMaxL];
  const float *wl, *bl;
  const float* g;          // [K][N] the step's gradient
  const float* st_prev;    // state before the step
  const float* dx_next;    // [K][N] dL/d(delta_t)
  const float* carry_in;   // state layout: dL/dh_l(t), dL/dc_l(t) from step t + 1
  float* carry_out;        // ... for step t - 1
  float* act[kKlMaxL];     // [N][in_l + H_l]
  float* dz[kKlMaxL];      // [N][4 H_l]
  float* tc;               // scratch [sum_l H_l][N]
  float* h_last;           // [N][H_L]
  float* dd;               // [N][K]
  long N;
};

__global__ __launch_bounds__(kKlBwdThreads) void k_klstm_bwd_step(KlBwdParams p) {
  __shared__ float row[kKlBwdThreads][kKlBwdRow];
  __shared__ float nxt[kKlBwdThreads][kKlMaxH + 1];           // a layer's h(t); then dL/dh arriving from above
  const int t = threadIdx.x;
  const long n = (long)blockIdx.x * kKlBwdThreads + t;
  if (n >= p.N) return;                                      // (no cross-thread traffic: dead threads just leave)
  const int L = p.n_layers;
  // ---- forward, layer by layer
  for (int k = 0; k < p.in; ++k) {
    float f;
    if (p.pre == L2O_PRE_LOGSIGN) {
      const float gv = p.g[(long)(k >> 1) * p.N + n];
      f = (k & 1) ? fminf(fmaxf(gv * p.exp_k, -1.0f), 1.0f)
                  : fmaxf(logf(fabsf(gv) + 1.1920928955078125e-07f) * p.k_inv, -1.0f);
    } else {
      f = p.g[(long)k * p.N + n];
    }
    row[t][k] = f;
  }
  {
    int width = p.in;
    long off = 0, tco = 0;
    for (int l = 0; l < L; ++l) {
      const int H = p.H[l], KA = width + H, G = 4 * H;
      const float* hprev = p.st_prev + off * p.N;
      const float* cprev = p.st_prev + (off + H) * p.N;
      for (int u = 0; u < H; ++u) row[t][width + u] = hprev[(long)u * p.N + n];
      float* arow = p.act[l] + n * (long)KA;
      for (int k = 0; k < KA; ++k) arow[k] = row[t][k];
      const l2o_cfp wg = (l2o_cfp)p.wg[l];
      const l2o_cfp bg = (l2o_cfp)p.bg[l];
      float* gates = p.dz[l] + n * (long)G;                  // gate ACTIVATIONS until the backward sweep
      for (int u = 0; u < H; ++u) {
        float zi = bg[u], zj = bg[H + u], zf = bg[2 * H + u], zo = bg[3 * H + u];
        for (int k = 0; k < KA; ++k) {
          const float av = row[t][k];
          zi = __builtin_fmaf(av, wg[k * G + u], zi);
          zj = __builtin_fmaf(av, wg[k * G + H + u], zj);
          zf = __builtin_fmaf(av, wg[k * G + 2 * H + u], zf);
          zo = __builtin_fmaf(av, wg[k * G + 3 * H + u], zo);
        }
        const float gi = kl_sigmoid(zi), gj = tanhf(zj), gf = kl_sigmoid(zf + 1.0f), go = kl_sigmoid(zo);
        const float th = tanhf(gf * cprev[(long)u * p.N + n] + gi * gj);
        gates[u] = gi; gates[H + u] = gj; gates[2 * H + u] = gf; gates[3 * H + u] = go;
        p.tc[(tco + u) * p.N + n] = th;
        nxt[t][u] = th * go;
      }
      for (int u = 0; u < H; ++u) row[t][u] = nxt[t][u];     // next layer's input (same thread: no barrier)
      width = H;
      off += 2 * H;
      tco += H;
    }
  }
  // ---- output Linear and its adjoint: row[t][0 .. HL) = h_L(t), nxt[t][] <- dL/dh_L(t) from the head
  const int HL = p.H[L - 1];
  const l2o_cfp wl = (l2o_cfp)p.wl;
  const l2o_cfp bl = (l2o_cfp)p.bl;
  for (int u = 0; u < HL; ++u) { p.h_last[n * (long)HL + u] = row[t][u]; nxt[t][u] = 0.0f; }
  for (int j = 0; j < p.K; ++j) {
    float ddv = p.dx_next[(long)j * p.N + n] * p.scale;
    if (p.tanh_output) {
      float s = bl[j];
      for (int u = 0; u < HL; ++u) s = __builtin_fmaf(row[t][u], wl[u * p.K + j], s);
      const float th = tanhf(s);
      ddv *= 1.0f - th * th;
    }
    p.dd[n * (long)p.K + j] = ddv;
    for (int u = 0; u < HL; ++u) nxt[t][u] = __builtin_fmaf(ddv, wl[u * p.K + j], nxt[t][u]);
  }
  // ---- backward, top layer first
  long off = 0, tco = 0;
  for (int l = 0; l < L; ++l) { off += 2 * p.H[l]; tco += p.H[l]; }
  for (int l = L - 1; l >= 0; --l) {
    const int H = p.H[l], G = 4 * H;
    const int inw = l == 0 ? p.in : p.H[l - 1];
    const int KA = inw + H;
    off -= 2 * H;
    tco -= H;
    float* dzr = p.dz[l] + n * (long)G;
    for (int u = 0; u < H; ++u) {
      const float gi = dzr[u], gj = dzr[H + u], gf = dzr[2 * H + u], go = dzr[3 * H + u];
      const float th = p.tc[(tco + u) * p.N + n];
      const float cpv = p.st_prev[(off + H + u) * p.N + n];
      const float dhu = nxt[t][u] + p.carry_in[(off + u) * p.N + n];
      const float dc = p.carry_in[(off + H + u) * p.N + n] + dhu * go * (1.0f - th * th);
      p.carry_out[(off + H + u) * p.N + n] = dc * gf;
      dzr[u] = dc * gj * gi * (1.0f - gi);
      dzr[H + u] = dc * gi * (1.0f - gj * gj);
      dzr[2 * H + u] = dc * cpv * gf * (1.0f - gf);
      dzr[3 * H + u] = dhu * th * go * (1.0f - go);
    }
    // d[input_l | h_l(t-1)] = dz_l W_l^T; the patch features of layer 0 are constants of the first-order gradient
    const l2o_cfp wg = (l2o_cfp)p.wg[l];
    for (int k = (l == 0 ? inw : 0); k < KA; ++k) {
      float s = 0.0f;
      for (int qq = 0; qq < G; ++qq) s = __builtin_fmaf(dzr[qq], wg[k * G + qq], s);
      if (k >= inw) p.carry_out[(off + (k - inw)) * p.N + n] = s;     // dL/dh_l(t-1)
      else nxt[t][k] = s;                                              // layer l - 1's dL/dh
    }
  }
}

}  // namespace l2o
