// l2o_twin.h -- Twin-L2O: the evaluation unroll of two per-coordinate two-layer LSTM optimizers over a minimax objective
// (l2o_twin_abi.h), all iterations of all instances in one persistent launch.
//
// k_twin_unroll.  One workgroup of eight waves per 16 coordinate rows; lane (c, q) = (lane & 15, lane >> 4) of every wave is
// row c of the tile.  An instance's `dim` rows never straddle a tile: a tile takes ipt = 16 / dim whole instances in its
// first ipt dim row slots (the rest, and instances past n_inst, are dead: they load nothing and store nothing), so the
// matrix game's A v and A^T u see the value just stepped without leaving the workgroup.
// The gate pre-activations run TRANSPOSED on the matrix cores in exact fp32 (l2o_common.h: mfma16), the project's tile
// convention: D[rho][c] += A[rho][k] B[k][c], A 16 gate columns, B the activations of the 16 rows.  The gate columns of
// tile t are permuted so that row rho = 4 q + r is gate r (i, f, g, o) of unit 4 t + q: a lane ends up holding the four gates
// of a unit and the h' it computes is the B operand (k = 4 kk + q) of the next layer and the next step.  The H / 4 gate
// tiles of a layer (H padded to a multiple of 4 with inert units: zero weights, zero state) are split over the eight waves,
// tile t to wave t & 7, two tiles (two accumulator chains) in flight per wave; h' goes through LDS, one barrier per layer.
// Weights: both networks do not fit in LDS (H = 50: 133 KB each), so every wave STREAMS the A fragments of its own tiles
// from the re-packed buffer (k_twin_pack: fragment order, one float4 per lane per four k-steps, contiguous per tile) every
// iteration, two float4 loads ahead of the MFMAs that use them; both packs sit in every XCD's L2 after the first iteration.
// theta lives in registers (every wave holds the same copy; other coordinates of an instance are read with __shfl), the
// states in LDS: per network h1 and h2 twice (the step reads the old while tiles of the new are written), c1, c2 once
// (a lane reads and writes only what it owns).  Gates, cell update and the head are fp32 VALU with accurate expf / tanhf /
// sinf / cosf; the head's sum over the four q lanes is an xor butterfly, the same bits in all four lanes and all eight waves.
#pragma once
#include "l2o_common.h"

namespace l2o {

constexpr int kTwWaves = 8;
constexpr int kTwThreads = 64 * kTwWaves;
constexpr int kTwMaxH = 96;
constexpr int kTwMaxDim = 16;

// ---- the re-packed weights of one network (floats; nt = ceil(H / 4) gate tiles, ntp = nt rounded up to a multiple of 4) ----
//   sp1 [nt][64]                 layer 1, the special k-step: k = 0 input g, 1 input s (0 when n_in = 1), 2 b_ih1, 3 b_hh1
//   hh1 [nt][ntp / 4][64][4]     layer 1, w_hh1: k-step kk = 4 k4 + j in word j of lane's float4; zero past H
//   sp2 [nt][64]                 layer 2, the special k-step: k = 0 b_ih2, 1 b_hh2, 2 and 3 zero
//   ih2, hh2                     as hh1
//   wl [4 ntp], bl [4]           the head: w_out zero-padded, b_out in word 0
__host__ __device__ inline int tw_nt(int H) { return (H + 3) / 4; }
__host__ __device__ inline int tw_ntp(int H) { return (tw_nt(H) + 3) / 4 * 4; }
__host__ __device__ inline int tw_off_sp1(int, int) { return 0; }
__host__ __device__ inline int tw_off_hh1(int nt, int) { return nt * 64; }
__host__ __device__ inline int tw_off_sp2(int nt, int ntp) { return tw_off_hh1(nt, ntp) + nt * ntp * 64; }
__host__ __device__ inline int tw_off_ih2(int nt, int ntp) { return tw_off_sp2(nt, ntp) + nt * 64; }
__host__ __device__ inline int tw_off_hh2(int nt, int ntp) { return tw_off_ih2(nt, ntp) + nt * ntp * 64; }
__host__ __device__ inline int tw_off_wl(int nt, int ntp) { return tw_off_hh2(nt, ntp) + nt * ntp * 64; }
__host__ __device__ inline int tw_off_bl(int nt, int ntp) { return tw_off_wl(nt, ntp) + 4 * ntp; }
__host__ __device__ inline int tw_pack_floats(int H) { return tw_off_bl(tw_nt(H), tw_ntp(H)) + 4; }
// LDS floats of one network: h1 x 2, h2 x 2, c1, c2 ([ntp][64] each), wl [4 ntp], bl [4]
__host__ __device__ inline int tw_lds_net_floats(int H) { return 6 * tw_ntp(H) * 64 + 4 * tw_ntp(H) + 4; }

struct TwPackParams {
  int H, n_in;
  const float *w_ih1, *w_hh1, *b_ih1, *b_hh1, *w_ih2, *w_hh2, *b_ih2, *b_hh2, *w_out, *b_out;
  float* out;
};

// element j of a [nt][ntp / 4][64][4] stream of the [4H][H] matrix w
__device__ __forceinline__ float tw_stream_elem(const float* w, int H, int ntp, int j) {
  const int t = j / (ntp * 64), r = j % (ntp * 64);
  const int k4 = r >> 8, ln = (r >> 2) & 63, kk = 4 * k4 + (r & 3);
  const int rho = ln & 15, unit = 4 * t + (rho >> 2), k = 4 * kk + (ln >> 4);
  return (unit < H && k < H) ? w[((rho & 3) * H + unit) * H + k] : 0.0f;
}

__global__ __launch_bounds__(256) void k_twin_pack(TwPackParams p) {
  const int H = p.H, nt = tw_nt(H), ntp = tw_ntp(H), total = tw_pack_floats(H);
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    float v = 0.0f;
    if (i < tw_off_hh1(nt, ntp) || (i >= tw_off_sp2(nt, ntp) && i < tw_off_ih2(nt, ntp))) {
      const bool l2 = i >= tw_off_sp2(nt, ntp);
      const int j = l2 ? i - tw_off_sp2(nt, ntp) : i;
      const int t = j >> 6, rho = j & 15, kq = (j >> 4) & 3, unit = 4 * t + (rho >> 2), row = (rho & 3) * H + unit;
      if (unit < H) {
        if (l2) v = kq == 0 ? p.b_ih2[row] : (kq == 1 ? p.b_hh2[row] : 0.0f);
        else if (kq < 2) v = kq < p.n_in ? p.w_ih1[row * p.n_in + kq] : 0.0f;
        else v = kq == 2 ? p.b_ih1[row] : p.b_hh1[row];
      }
    } else if (i < tw_off_sp2(nt, ntp)) {
      v = tw_stream_elem(p.w_hh1, H, ntp, i - tw_off_hh1(nt, ntp));
    } else if (i < tw_off_hh2(nt, ntp)) {
      v = tw_stream_elem(p.w_ih2, H, ntp, i - tw_off_ih2(nt, ntp));
    } else if (i < tw_off_wl(nt, ntp)) {
      v = tw_stream_elem(p.w_hh2, H, ntp, i - tw_off_hh2(nt, ntp));
    } else if (i < tw_off_bl(nt, ntp)) {
      const int u = i - tw_off_wl(nt, ntp);
      v = u < H ? p.w_out[u] : 0.0f;
    } else if (i == tw_off_bl(nt, ntp)) {
      v = p.b_out[0];
    }
    p.out[i] = v;
  }
}

struct TwNetParams {
  int H, nt, ntp, n_in;
  const float* pack;
  float* state;            // [4][H][rows]
};

struct TwParams {
  TwNetParams net[2];      // 0: min (odd k), 1: max (even k)
  int kind, n_inst, dim, ipt;
  int iter0, n_iter, n_sign;
  float rescale, out_mul;
  const float* sign_lr;
  const float* data;
  float* theta;
  float* curve;
  float* fval;
  float* delta;
};

__host__ __device__ inline int tw_lds_floats(const TwParams& p) {
  return tw_lds_net_floats(p.net[0].H) + tw_lds_net_floats(p.net[1].H) + 16 * kTwMaxDim;
}

__device__ __forceinline__ float tw_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// acc0 / acc1 += (tiles t0 / t1 of a weight stream) x (scale * B): nk4 float4 per lane and tile, B [4 nk4][64] in LDS.  The
// loads run two float4 ahead of the MFMAs (the last ones are repeated, harmlessly, instead of branching).
__device__ __forceinline__ void tw_stream(f32x4& acc0, f32x4& acc1, const float4* __restrict__ a0,
                                          const float4* __restrict__ a1, const float* b, int nk4, float scale) {
  float4 x0 = a0[0], x1 = a1[0];
  const int i1 = nk4 > 1 ? 64 : 0;
  float4 y0 = a0[i1], y1 = a1[i1];
  for (int k4 = 0; k4 < nk4; ++k4) {
    const int in = (k4 + 2 < nk4 ? k4 + 2 : nk4 - 1) * 64;
    const float4 z0 = a0[in], z1 = a1[in];
    const float* bk = b + k4 * 256;
    const float b0 = scale * bk[0], b1 = scale * bk[64], b2 = scale * bk[128], b3 = scale * bk[192];
    acc0 = mfma16(x0.x, b0, acc0); acc1 = mfma16(x1.x, b0, acc1);
    acc0 = mfma16(x0.y, b1, acc0); acc1 = mfma16(x1.y, b1, acc1);
    acc0 = mfma16(x0.z, b2, acc0); acc1 = mfma16(x1.z, b2, acc1);
    acc0 = mfma16(x0.w, b3, acc0); acc1 = mfma16(x1.w, b3, acc1);
    x0 = y0; x1 = y1; y0 = z0; y1 = z1;
  }
}

// One LSTM layer of the wave's gate tiles (t = wave, wave + 8, ...; two at a time, an odd last one is computed twice and
// stored once).  sp: the special k-step's fragments, its B operand bsp in a register; then the stream sa over ba (scaled by
// sca) and, when sb is not NULL, sb over bb (scaled by scb).  c: the layer's cell state, multiplied by `rescale` as it is
// read; hn: where h' goes.
__device__ __forceinline__ void tw_layer(const float* __restrict__ sp, float bsp, const float* __restrict__ sa,
                                         const float* ba, float sca, const float* __restrict__ sb, const float* bb,
                                         float scb, float* c, float* hn, int nt, int ntp, int wave, int lane,
                                         float rescale) {
  for (int t0 = wave; t0 < nt; t0 += 2 * kTwWaves) {
    const int t1 = t0 + kTwWaves < nt ? t0 + kTwWaves : t0;
    const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    f32x4 acc0 = mfma16(sp[t0 * 64 + lane], bsp, zero);
    f32x4 acc1 = mfma16(sp[t1 * 64 + lane], bsp, zero);
    tw_stream(acc0, acc1, reinterpret_cast<const float4*>(sa + (long)t0 * ntp * 64) + lane,
              reinterpret_cast<const float4*>(sa + (long)t1 * ntp * 64) + lane, ba + lane, ntp / 4, sca);
    if (sb)
      tw_stream(acc0, acc1, reinterpret_cast<const float4*>(sb + (long)t0 * ntp * 64) + lane,
                reinterpret_cast<const float4*>(sb + (long)t1 * ntp * 64) + lane, bb + lane, ntp / 4, scb);
    for (int half = 0; half < 2; ++half) {
      if (half && t1 == t0) break;
      const int t = half ? t1 : t0;
      const f32x4 z = half ? acc1 : acc0;
      const float cp = rescale * c[t * 64 + lane];
      const float cn = tw_sigmoid(z[1]) * cp + tw_sigmoid(z[0]) * tanhf(z[2]);
      c[t * 64 + lane] = cn;
      hn[t * 64 + lane] = tw_sigmoid(z[3]) * tanhf(cn);
    }
  }
}

// (l2o_twin_train.h holds a sibling copy of this kernel and of tw_layer, k_twin_record / tw_layer_rec, with the stores of the
// meta-training history added: a template flag here changed this kernel's schedule.  Any change to the arithmetic below must
// be repeated there; tests/test_twin_train.py holds the two to the same bits.)
__global__ __launch_bounds__(kTwThreads) void k_twin_unroll(TwParams p) {
  extern __shared__ float tw_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, q = lane >> 4;
  const int dim = p.dim, li = c / dim, d = c - li * dim;
  const long inst = (long)blockIdx.x * p.ipt + li;
  const bool live = li < p.ipt && inst < p.n_inst;
  const long rows = (long)p.n_inst * dim, row = inst * dim + d;
  const int cb = (lane & 48) + li * dim;                      // the lane of coordinate 0 of this lane's instance
  float* const lds0 = tw_lds;
  float* const lds1 = tw_lds + tw_lds_net_floats(p.net[0].H);
  float* const amat = lds1 + tw_lds_net_floats(p.net[1].H);         // kind 4: [ipt][dim][dim]
  const float kPi = 3.14159265358979323846f;

  // ---- LDS: zero (the padded units and k-steps stay zero), then the states, the heads and the instances' matrices
  const int lds_total = tw_lds_floats(p);
  for (int i = tid; i < lds_total; i += kTwThreads) tw_lds[i] = 0.0f;
  __syncthreads();
  for (int n = 0; n < 2; ++n) {
    const TwNetParams& nn = p.net[n];
    const int sz = nn.ntp * 64;
    float* L = n ? lds1 : lds0;
    for (int t = wave; t < nn.nt; t += kTwWaves) {
      const int u = 4 * t + q;
      if (live && u < nn.H) {
        L[t * 64 + lane] = nn.state[(long)u * rows + row];                          // h1 (buffer 0)
        L[4 * sz + t * 64 + lane] = nn.state[((long)nn.H + u) * rows + row];        // c1
        L[2 * sz + t * 64 + lane] = nn.state[(2L * nn.H + u) * rows + row];         // h2 (buffer 0)
        L[5 * sz + t * 64 + lane] = nn.state[(3L * nn.H + u) * rows + row];         // c2
      }
    }
    const float* hd = nn.pack + tw_off_wl(nn.nt, nn.ntp);
    for (int i = tid; i < 4 * nn.ntp + 4; i += kTwThreads) L[6 * sz + i] = hd[i];
  }
  if (p.kind == 4) {
    const int per = dim * dim, n_here = p.ipt * per;
    for (int i = tid; i < n_here; i += kTwThreads) {
      const long ins = (long)blockIdx.x * p.ipt + i / per;
      if (ins < p.n_inst) amat[i] = p.data[ins * per + i % per];
    }
  }
  float u = 0.0f, v = 0.0f, pa = 0.0f, pb = 0.0f;
  if (live) {
    u = p.theta[inst * 2 * dim + d];
    v = p.theta[inst * 2 * dim + dim + d];
    if (p.kind != 4) { pa = p.data[inst * 2]; pb = p.data[inst * 2 + 1]; }
  }
  __syncthreads();

  int par = 0;                                                // bit n: which h buffer of network n is current
  for (int it = 0; it < p.n_iter; ++it) {
    const int k = p.iter0 + it, n = (k & 1) ^ 1;              // odd k: min, even k: max
    // ---- df/du and df/dv at (u, v)
    float gu, gv;
    if (p.kind == 1) {
      gu = 2.0f * u * pa;
      gv = -2.0f * pb * v;
    } else if (p.kind == 2) {
      gu = 2.0f * u * pa + 2.0f * v;
      gv = -2.0f * pb * v + 2.0f * u;
    } else if (p.kind == 3) {
      const float ph = pa * kPi * u;
      gu = -pb * v * cosf(ph) * pa * kPi;
      gv = -pb * sinf(ph);
    } else {
      gu = gv = 0.0f;
      for (int j = 0; j < dim; ++j) {
        const int src = (lane & 48) | ((cb + j) & 15);
        const float uj = __shfl(u, src), vj = __shfl(v, src);
        const float adj = live ? amat[(li * dim + d) * dim + j] : 0.0f;
        const float ajd = live ? amat[(li * dim + j) * dim + d] : 0.0f;
        gu = __builtin_fmaf(adj, vj, gu);
        gv = __builtin_fmaf(ajd, uj, gv);
      }
    }
    const TwNetParams& nn = p.net[n];
    const int nt = nn.nt, ntp = nn.ntp, sz = ntp * 64, cur = (par >> n) & 1;
    float* L = n ? lds1 : lds0;
    const float g = n ? gv : gu, s = n ? gu : gv;
    // ---- layer 1: [g, s, 1, 1] and rescale * h1
    const float xin = q == 0 ? g : (q == 1 ? (nn.n_in == 2 ? s : 0.0f) : 1.0f);
    float* h1n = L + (cur ^ 1) * sz;
    tw_layer(nn.pack + tw_off_sp1(nt, ntp), xin, nn.pack + tw_off_hh1(nt, ntp), L + cur * sz, p.rescale, nullptr, nullptr,
             0.0f, L + 4 * sz, h1n, nt, ntp, wave, lane, p.rescale);
    __syncthreads();
    // ---- layer 2: [1, 1, 0, 0], h1' and rescale * h2
    float* h2n = L + (2 + (cur ^ 1)) * sz;
    tw_layer(nn.pack + tw_off_sp2(nt, ntp), q < 2 ? 1.0f : 0.0f, nn.pack + tw_off_ih2(nt, ntp), h1n, 1.0f,
             nn.pack + tw_off_hh2(nt, ntp), L + (2 + cur) * sz, p.rescale, L + 5 * sz, h2n, nt, ntp, wave, lane, p.rescale);
    __syncthreads();
    par ^= 1 << n;
    // ---- the head (every wave: the same bits) and the step
    const float* wl = L + 6 * sz;
    float dl = 0.0f;
    for (int t = 0; t < nt; ++t) dl = __builtin_fmaf(h2n[t * 64 + lane], wl[4 * t + q], dl);
    dl += __shfl_xor(dl, 16);
    dl += __shfl_xor(dl, 32);
    dl += wl[4 * ntp];
    float step;
    if (k <= p.n_sign) step = (dl > 0.0f ? 1.0f : (dl < 0.0f ? -1.0f : 0.0f)) * p.sign_lr[k - 1];
    else step = dl * p.out_mul;
    if (n) v += step; else u += step;
    // ---- records (wave 0)
    if (wave == 0) {
      const long rec = (long)it * p.n_inst + inst;
      if (p.curve && live && q == 0) {
        p.curve[rec * 2 * dim + d] = u;
        p.curve[rec * 2 * dim + dim + d] = v;
      }
      if (p.delta && live && q == 0) p.delta[rec * dim + d] = dl;
      if (p.fval) {
        float f;
        if (p.kind == 1) f = pa * u * u - pb * v * v;
        else if (p.kind == 2) f = pa * u * u - pb * v * v + 2.0f * v * u;
        else if (p.kind == 3) f = -pb * v * sinf(kPi * u * pa);
        else {
          float av = 0.0f;
          for (int j = 0; j < dim; ++j) {
            const float vj = __shfl(v, (lane & 48) | ((cb + j) & 15));
            av = __builtin_fmaf(live ? amat[(li * dim + d) * dim + j] : 0.0f, vj, av);
          }
          const float ua = u * av;
          f = 0.0f;
          for (int j = 0; j < dim; ++j) f += __shfl(ua, (lane & 48) | ((cb + j) & 15));
        }
        if (live && q == 0 && d == 0) p.fval[rec] = f;
      }
    }
  }

  // ---- write back: theta (wave 0), every wave the state tiles it owns
  if (wave == 0 && live && q == 0) {
    p.theta[inst * 2 * dim + d] = u;
    p.theta[inst * 2 * dim + dim + d] = v;
  }
  for (int n = 0; n < 2; ++n) {
    const TwNetParams& nn = p.net[n];
    const int sz = nn.ntp * 64, cur = (par >> n) & 1;
    const float* L = n ? lds1 : lds0;
    for (int t = wave; t < nn.nt; t += kTwWaves) {
      const int un = 4 * t + q;
      if (live && un < nn.H) {
        nn.state[(long)un * rows + row] = L[cur * sz + t * 64 + lane];
        nn.state[((long)nn.H + un) * rows + row] = L[4 * sz + t * 64 + lane];
        nn.state[(2L * nn.H + un) * rows + row] = L[(2 + cur) * sz + t * 64 + lane];
        nn.state[(3L * nn.H + un) * rows + row] = L[5 * sz + t * 64 + lane];
      }
    }
  }
}

}  // namespace l2o
