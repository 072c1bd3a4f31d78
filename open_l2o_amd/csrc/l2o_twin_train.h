// l2o_twin_train.h -- Twin-L2O meta-training (l2o_twin_train_abi.h): one segment's recording forward, its BPTT and the
// weight-gradient contraction.  Tile convention, gate layout and weight stream: l2o_twin.h, which this header builds on.
//
// k_twin_record.  k_twin_unroll's text with stores added (a sibling, not a template argument: k_twin_unroll keeps its
// instructions): every iteration leaves one record -- what its BPTT step and the contraction read -- in the history.
// k_twin_bptt.    One workgroup per (row tile, network); the two networks' backward passes share nothing.  It walks the
// network's iterations of the segment in reverse: seed g_delta from the recorded point, head, layer-2 cell, W_ih2^T dz2 into
// layer 1 and W_hh2^T dz2 into the carry, layer-1 cell, W_hh1^T dz1 into the carry; the carries are multiplied by `rescale`.
// The products W^T dz run on the fp32 MFMA from the transposed fragments of k_twin_pack_t: the contraction chunk
// (gate tile t, gate r) is exactly register r of the dz tile t as the cell phase leaves it, so dz goes through LDS untouched.
// It writes g_delta and both layers' dz per iteration to scratch.
// k_twin_wgrad.   dW = sum over rows x iterations of dz in^T, one wave per 16 x 16 tile of a gradient, on the fp32 MFMA:
// a wave walks tiles, iterations and the four row chunks of a tile in a fixed order (no atomics: two runs give the same bits).
#pragma once
#include "l2o_twin.h"

namespace l2o {

constexpr int kTwMaxNt = (kTwMaxH + 3) / 4;      // 24, a multiple of 4: also the largest ntp

// ---- one iteration's record (floats; nt of the network that steps): [0, 64) the 16 rows' g, s, then u, v after the step;
// then per layer (nt * 448 each) the activated gates [nt][64][4] (i, f, g, o), rescale * c [nt][64], the h the step read
// [nt][64] and the h' it wrote [nt][64], all in the lane order of the LDS tiles (unit 4 t + q of row c at t * 64 + 16 q + c).
__host__ __device__ inline int tw_rec_layer_floats(int nt) { return nt * 448; }
__host__ __device__ inline int tw_rec_floats(int nt) { return 64 + 2 * tw_rec_layer_floats(nt); }
// ---- one iteration's backward scratch: g_delta [16], g_delta in double [16] (32 floats), then per layer dz [nt][4][64]
// (register r of lane (c, q): gate r of unit 4 t + q, row c)
constexpr int kTwDzHead = 48;
__host__ __device__ inline int tw_dz_floats(int nt) { return kTwDzHead + 2 * nt * 256; }

// tw_layer (l2o_twin.h) with the record's stores; the arithmetic is the same text.
__device__ __forceinline__ void tw_layer_rec(const float* __restrict__ sp, float bsp, const float* __restrict__ sa,
                                             const float* ba, float sca, const float* __restrict__ sb, const float* bb,
                                             float scb, float* c, float* hn, int nt, int ntp, int wave, int lane,
                                             float rescale, float* __restrict__ rec) {
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
      const float gf = tw_sigmoid(z[1]), gi = tw_sigmoid(z[0]), gg = tanhf(z[2]);
      const float cn = gf * cp + gi * gg;
      c[t * 64 + lane] = cn;
      const float go = tw_sigmoid(z[3]);
      hn[t * 64 + lane] = go * tanhf(cn);
      reinterpret_cast<float4*>(rec)[t * 64 + lane] = make_float4(gi, gf, gg, go);
      rec[nt * 256 + t * 64 + lane] = cp;
    }
  }
}

// (df/du, df/dv) of this lane's row at (u, v), as k_twin_unroll computes them
__device__ __forceinline__ void tw_grad_uv(int kind, float u, float v, float pa, float pb, const float* amat, int dim, int li,
                                           int d, int cb, int lane, bool live, float& gu, float& gv) {
  const float kPi = 3.14159265358979323846f;
  if (kind == 1) {
    gu = 2.0f * u * pa;
    gv = -2.0f * pb * v;
  } else if (kind == 2) {
    gu = 2.0f * u * pa + 2.0f * v;
    gv = -2.0f * pb * v + 2.0f * u;
  } else if (kind == 3) {
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
}

// df / d(own variable) of network n (0: u, 1: v) of this lane's row at (u, v) in double: the seed of the BPTT.  The b_out
// gradient is the plain sum of the seeds, of both signs (sum |g| / |sum g| = 24 in a tested seesaw case): evaluated in float
// the seed's own roundings show there beside the float32 error of the recorded point, which is the forward's and stays.
__device__ __forceinline__ double tw_seed_own(int kind, int n, double u, double v, double pa, double pb, const float* amat,
                                              int dim, int li, int d, int cb, int lane, bool live) {
  const double kPi = 3.14159265358979323846;
  if (kind == 1) return n ? -2.0 * pb * v : 2.0 * u * pa;
  if (kind == 2) return n ? -2.0 * pb * v + 2.0 * u : 2.0 * u * pa + 2.0 * v;
  if (kind == 3) return n ? -pb * sin(pa * kPi * u) : -pb * v * cos(pa * kPi * u) * pa * kPi;
  double g = 0.0;
  for (int j = 0; j < dim; ++j) {
    const int src = (lane & 48) | ((cb + j) & 15);
    const double oj = __shfl(n ? u : v, src);                  // A v for u, A^T u for v
    const float a = live ? (n ? amat[(li * dim + j) * dim + d] : amat[(li * dim + d) * dim + j]) : 0.0f;
    g += (double)a * oj;
  }
  return g;
}

// k_twin_unroll (l2o_twin.h) that also leaves iteration it's record at hist + (tile * n_iter + it) * rec_stride.
__global__ __launch_bounds__(kTwThreads) void k_twin_record(TwParams p, float* __restrict__ hist, long rec_stride) {
  extern __shared__ float tw_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, q = lane >> 4;
  const int dim = p.dim, li = c / dim, d = c - li * dim;
  const long inst = (long)blockIdx.x * p.ipt + li;
  const bool live = li < p.ipt && inst < p.n_inst;
  const long rows = (long)p.n_inst * dim, row = inst * dim + d;
  const int cb = (lane & 48) + li * dim;
  float* const lds0 = tw_lds;
  float* const lds1 = tw_lds + tw_lds_net_floats(p.net[0].H);
  float* const amat = lds1 + tw_lds_net_floats(p.net[1].H);
  const float kPi = 3.14159265358979323846f;

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
        L[t * 64 + lane] = nn.state[(long)u * rows + row];
        L[4 * sz + t * 64 + lane] = nn.state[((long)nn.H + u) * rows + row];
        L[2 * sz + t * 64 + lane] = nn.state[(2L * nn.H + u) * rows + row];
        L[5 * sz + t * 64 + lane] = nn.state[(3L * nn.H + u) * rows + row];
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

  int par = 0;
  for (int it = 0; it < p.n_iter; ++it) {
    const int k = p.iter0 + it, n = (k & 1) ^ 1;
    float gu, gv;
    tw_grad_uv(p.kind, u, v, pa, pb, amat, dim, li, d, cb, lane, live, gu, gv);
    const TwNetParams& nn = p.net[n];
    const int nt = nn.nt, ntp = nn.ntp, sz = ntp * 64, cur = (par >> n) & 1;
    float* L = n ? lds1 : lds0;
    float* const rec = hist + ((long)blockIdx.x * p.n_iter + it) * rec_stride;
    float* const rec1 = rec + 64;
    float* const rec2 = rec1 + tw_rec_layer_floats(nt);
    const float g = n ? gv : gu, s = n ? gu : gv;
    const float xin = q == 0 ? g : (q == 1 ? (nn.n_in == 2 ? s : 0.0f) : 1.0f);
    float* h1n = L + (cur ^ 1) * sz;
    tw_layer_rec(nn.pack + tw_off_sp1(nt, ntp), xin, nn.pack + tw_off_hh1(nt, ntp), L + cur * sz, p.rescale, nullptr, nullptr,
                 0.0f, L + 4 * sz, h1n, nt, ntp, wave, lane, p.rescale, rec1);
    __syncthreads();
    float* h2n = L + (2 + (cur ^ 1)) * sz;
    tw_layer_rec(nn.pack + tw_off_sp2(nt, ntp), q < 2 ? 1.0f : 0.0f, nn.pack + tw_off_ih2(nt, ntp), h1n, 1.0f,
                 nn.pack + tw_off_hh2(nt, ntp), L + (2 + cur) * sz, p.rescale, L + 5 * sz, h2n, nt, ntp, wave, lane, p.rescale,
                 rec2);
    __syncthreads();
    for (int t = wave; t < nt; t += kTwWaves) {                 // the h each layer read and the h' it wrote
      const int o = nt * 320 + t * 64 + lane;
      rec1[o] = L[cur * sz + t * 64 + lane];
      rec1[o + nt * 64] = h1n[t * 64 + lane];
      rec2[o] = L[(2 + cur) * sz + t * 64 + lane];
      rec2[o + nt * 64] = h2n[t * 64 + lane];
    }
    par ^= 1 << n;
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
    if (wave == 0) {
      if (q == 0) {
        rec[c] = g;
        rec[16 + c] = nn.n_in == 2 ? s : 0.0f;
        rec[32 + c] = u;
        rec[48 + c] = v;
      }
      const long recno = (long)it * p.n_inst + inst;
      if (p.curve && live && q == 0) {
        p.curve[recno * 2 * dim + d] = u;
        p.curve[recno * 2 * dim + dim + d] = v;
      }
      if (p.delta && live && q == 0) p.delta[recno * dim + d] = dl;
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
        if (live && q == 0 && d == 0) p.fval[recno] = f;
      }
    }
  }

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

// ---- the transposed fragments of one network: [3 = w_hh1, w_ih2, w_hh2][NT = ntp / 4][nt][64][4].  Output tile T of
// W^T dz holds unit 4 (4 T + j) + q in register j of lane (c, q) (so register j is LDS tile 4 T + j); the k-step (t, r)
// contracts gate r of units 4 t ... 4 t + 3: word r of lane (m, q)'s float4 is W[r H + 4 t + q][4 (4 T + (m & 3)) + (m >> 2)].
__host__ __device__ inline int tw_packt_mat_floats(int H) { return tw_ntp(H) / 4 * tw_nt(H) * 256; }
__host__ __device__ inline int tw_packt_floats(int H) { return 3 * tw_packt_mat_floats(H); }

struct TwPackTParams {
  int H;
  const float *w_hh1, *w_ih2, *w_hh2;
  float* out;
};

__global__ __launch_bounds__(256) void k_twin_pack_t(TwPackTParams p) {
  const int H = p.H, nt = tw_nt(H), per = tw_packt_mat_floats(H), total = 3 * per;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int mat = i / per, j = i % per;
    const int T = j / (nt * 256), t = (j >> 8) % nt, ln = (j >> 2) & 63, r = j & 3, m = ln & 15;
    const int unit = 4 * t + (ln >> 4), k = 4 * (4 * T + (m & 3)) + (m >> 2);
    const float* w = mat == 0 ? p.w_hh1 : (mat == 1 ? p.w_ih2 : p.w_hh2);
    p.out[i] = (unit < H && k < H) ? w[((long)r * H + unit) * H + k] : 0.0f;
  }
}

struct TwBpNet {
  int H, nt, ntp, n_in;
  const float* packt;
  const float* w_out;
};

struct TwBpParams {
  TwBpNet net[2];
  int kind, n_inst, dim, ipt;
  int iter0, n_iter, n_sign;
  float rescale, out_mul, loss_scale;
  const float* data;
  const float* inst_weight;
  const float* hist;
  long rec_stride;
  float* dz;
  long dz_stride;
};

// W^T dz of output tile T: fr the matrix' fragments, dz [nt][4][64] in LDS
__device__ __forceinline__ f32x4 tw_wt_dz(const float* __restrict__ fr, const float* dz, int T, int nt, int lane) {
  const float4* a = reinterpret_cast<const float4*>(fr + (long)T * nt * 256) + lane;
  f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int t = 0; t < nt; ++t) {
    const float4 x = a[t * 64];
    const float* b = dz + t * 256 + lane;
    acc = mfma16(x.x, b[0], acc);
    acc = mfma16(x.y, b[64], acc);
    acc = mfma16(x.z, b[128], acc);
    acc = mfma16(x.w, b[192], acc);
  }
  return acc;
}

// The cell's backward of the wave's gate tiles: dh [nt][64] (the whole dL/dh'), dc the carry into c' (replaced by the carry
// into the c the step read: rescale * dc' * f); dz to LDS and to `out`.  gd * wl is the head's share (layer 2; wl NULL: none).
__device__ __forceinline__ void tw_cell_bwd(const float* __restrict__ rec, const float* dh, float* dc, float gd, const float* wl,
                                            float* dzl, float* __restrict__ out, int nt, int wave, int lane, float rescale) {
  const int q = lane >> 4;
  for (int t = wave; t < nt; t += kTwWaves) {
    const float4 a = reinterpret_cast<const float4*>(rec)[t * 64 + lane];     // i, f, g, o
    const float cp = rec[nt * 256 + t * 64 + lane];
    float dht = dh[t * 64 + lane];
    if (wl) dht = __builtin_fmaf(gd, wl[4 * t + q], dht);
    const float tc = tanhf(a.y * cp + a.x * a.z);
    const float dcn = dht * a.w * (1.0f - tc * tc) + dc[t * 64 + lane];
    const float dzv[4] = {dcn * a.z * a.x * (1.0f - a.x), dcn * cp * a.y * (1.0f - a.y), dcn * a.x * (1.0f - a.z * a.z),
                          dht * tc * a.w * (1.0f - a.w)};
    dc[t * 64 + lane] = rescale * (dcn * a.y);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      dzl[(t * 4 + r) * 64 + lane] = dzv[r];
      out[(t * 4 + r) * 64 + lane] = dzv[r];
    }
  }
}

__global__ __launch_bounds__(kTwThreads) void k_twin_bptt(TwBpParams p) {
  __shared__ float dzl[kTwMaxNt * 256];
  __shared__ float dh1[kTwMaxNt * 64], dh2[kTwMaxNt * 64], dc1[kTwMaxNt * 64], dc2[kTwMaxNt * 64];
  __shared__ float wl[4 * kTwMaxNt];
  __shared__ float amat[16 * kTwMaxDim];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15;
  const int tile = blockIdx.x >> 1, n = blockIdx.x & 1;
  const int dim = p.dim, li = c / dim, d = c - li * dim;
  const long inst = (long)tile * p.ipt + li;
  const bool live = li < p.ipt && inst < p.n_inst;
  const int cb = (lane & 48) + li * dim;
  const TwBpNet& nn = p.net[n];
  const int nt = nn.nt, NT = nn.ntp / 4, per = tw_packt_mat_floats(nn.H);

  for (int i = tid; i < kTwMaxNt * 64; i += kTwThreads) dh1[i] = dh2[i] = dc1[i] = dc2[i] = 0.0f;
  for (int i = tid; i < 4 * kTwMaxNt; i += kTwThreads) wl[i] = i < nn.H ? nn.w_out[i] : 0.0f;
  for (int i = tid; i < 16 * kTwMaxDim; i += kTwThreads) amat[i] = 0.0f;
  __syncthreads();
  if (p.kind == 4) {
    const int pe = dim * dim, n_here = p.ipt * pe;
    for (int i = tid; i < n_here; i += kTwThreads) {
      const long ins = (long)tile * p.ipt + i / pe;
      if (ins < p.n_inst) amat[i] = p.data[ins * pe + i % pe];
    }
  }
  float pa = 0.0f, pb = 0.0f, wgt = 1.0f;
  if (live) {
    if (p.kind != 4) { pa = p.data[inst * 2]; pb = p.data[inst * 2 + 1]; }
    if (p.inst_weight) wgt = p.inst_weight[inst];
  }
  __syncthreads();

  for (int it = p.n_iter - 1; it >= 0; --it) {
    const int k = p.iter0 + it;
    if (((k & 1) ^ 1) != n) continue;
    const float* rec = p.hist + ((long)tile * p.n_iter + it) * p.rec_stride;
    const float* rec1 = rec + 64;
    const float* rec2 = rec1 + tw_rec_layer_floats(nt);
    float* out = p.dz + ((long)tile * p.n_iter + it) * p.dz_stride;
    // ---- the seed: w_k s_k out_mul (df/d own variable)(the point after iteration k) m loss_scale, 0 under the sign rule
    const double own = tw_seed_own(p.kind, n, rec[32 + c], rec[48 + c], pa, pb, amat, dim, li, d, cb, lane, live);
    const double ws = (it == p.n_iter - 1 ? 1.0 : 2.0) * (n ? -1.0 : 1.0);
    const double gdd = (live && k > p.n_sign) ? ws * (double)p.out_mul * own * (double)wgt * (double)p.loss_scale : 0.0;
    const float gd = (float)gdd;
    if (wave == 0 && lane < 16) {
      out[c] = gd;
      reinterpret_cast<double*>(out + 16)[c] = gdd;
    }
    // ---- the head and the layer-2 cell
    tw_cell_bwd(rec2, dh2, dc2, gd, wl, dzl, out + kTwDzHead + nt * 256, nt, wave, lane, p.rescale);
    __syncthreads();
    for (int j = wave; j < 2 * NT; j += kTwWaves) {            // dh1' += W_ih2^T dz2; the carry dh2 = rescale W_hh2^T dz2
      const int hh = j >= NT, T = hh ? j - NT : j;
      const f32x4 acc = tw_wt_dz(nn.packt + (1 + hh) * per, dzl, T, nt, lane);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int o = (4 * T + r) * 64 + lane;
        if (hh) dh2[o] = p.rescale * acc[r];
        else dh1[o] += acc[r];
      }
    }
    __syncthreads();
    // ---- the layer-1 cell
    tw_cell_bwd(rec1, dh1, dc1, 0.0f, nullptr, dzl, out + kTwDzHead, nt, wave, lane, p.rescale);
    __syncthreads();
    for (int T = wave; T < NT; T += kTwWaves) {                // the carry dh1 = rescale W_hh1^T dz1
      const f32x4 acc = tw_wt_dz(nn.packt, dzl, T, nt, lane);
#pragma unroll
      for (int r = 0; r < 4; ++r) dh1[(4 * T + r) * 64 + lane] = p.rescale * acc[r];
    }
    __syncthreads();
  }
}

// ---- the contraction.  Jobs of one network, one wave each (nK = ceil(H / 16) column tiles):
//   0 dz1 x [g, s, 1]     nt       w_ih1 and the layer-1 biases      4 dz2 x [., ., 1]      nt    the layer-2 biases
//   1 dz1 x rescale h1    nt nK    w_hh1                             5 g_delta x h2'        nK    w_out
//   2 dz2 x h1'           nt nK    w_ih2                             6 sum of g_delta       1     b_out (VALU, double)
//   3 dz2 x rescale h2    nt nK    w_hh2
__host__ __device__ inline int tw_wg_jobs(int H) { const int nt = tw_nt(H), nK = (H + 15) / 16; return nt * (2 + 3 * nK) + nK + 1; }

struct TwWgNet {
  int H, nt, n_in;
  float *w_ih1, *w_hh1, *b_ih1, *b_hh1, *w_ih2, *w_hh2, *b_ih2, *b_hh2, *w_out, *b_out;
};

struct TwWgParams {
  TwWgNet net[2];
  int tiles, iter0, n_iter;
  float rescale;
  const float* hist;
  long rec_stride;
  const float* dz;
  long dz_stride;
};

__global__ __launch_bounds__(64) void k_twin_wgrad(TwWgParams p) {
  const int jobs0 = tw_wg_jobs(p.net[0].H);
  const int n = (int)blockIdx.x >= jobs0;
  const TwWgNet& nn = p.net[n];
  const int H = nn.H, nt = nn.nt, nK = (H + 15) / 16;
  int j = (int)blockIdx.x - (n ? jobs0 : 0), type, t = 0, K = 0;
  if (j < nt) { type = 0; t = j; }
  else if ((j -= nt) < 3 * nt * nK) { type = 1 + j / (nt * nK); t = (j % (nt * nK)) / nK; K = j % nK; }
  else if ((j -= 3 * nt * nK) < nt) { type = 4; t = j; }
  else if ((j -= nt) < nK) { type = 5; K = j; }
  else type = 6;
  const int lane = threadIdx.x, m = lane & 15, q = lane >> 4;
  // A: lane (m, q) holds gate row m = 4 q' + r' of the tile for row 4 ch + q of the chunk
  const int a_layer = (type == 0 || type == 1) ? 0 : 1;
  const int a_off = type >= 5 ? 0 : kTwDzHead + a_layer * nt * 256 + (t * 4 + (m & 3)) * 64 + 16 * (m >> 2);
  // B: lane (m, q) holds input column m of the tile for the same row
  const bool special = type == 0 || type == 4;
  const int unit = 16 * K + m;
  const int b_layer = (type == 1 || type == 2) ? 0 : 1, b_new = type == 2 || type == 5;
  const int b_off = special ? (m < 2 ? 16 * m : 0)
                            : 64 + b_layer * tw_rec_layer_floats(nt) + nt * (b_new ? 384 : 320) + (unit >> 2) * 64 + 16 * (unit & 3);
  const bool b_load = special ? m < 2 : unit < H;
  const float b_const = (special && m == 2) ? 1.0f : 0.0f;
  const float b_scale = (type == 1 || type == 3) ? p.rescale : 1.0f;
  const bool a_load = type < 5 || m == 0;                      // (type 5: g_delta is row 0 of its one-row tile)

  if (type == 6) {                                             // b_out: the sum of the seeds, in double, in a fixed order
    double sum = 0.0;
    for (int tile = 0; tile < p.tiles; ++tile)
      for (int it = 0; it < p.n_iter; ++it) {
        if ((((p.iter0 + it) & 1) ^ 1) != n) continue;
        const double* gd = reinterpret_cast<const double*>(p.dz + ((long)tile * p.n_iter + it) * p.dz_stride + 16);
        for (int r = 0; r < 16; ++r) sum += gd[r];
      }
    if (lane == 0) nn.b_out[0] = (float)sum;
    return;
  }
  f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int tile = 0; tile < p.tiles; ++tile) {
    for (int it = 0; it < p.n_iter; ++it) {
      if ((((p.iter0 + it) & 1) ^ 1) != n) continue;
      const float* rec = p.hist + ((long)tile * p.n_iter + it) * p.rec_stride;
      const float* dz = p.dz + ((long)tile * p.n_iter + it) * p.dz_stride;
      float a[4], b[4];
#pragma unroll
      for (int ch = 0; ch < 4; ++ch) {
        const int row = 4 * ch + q;
        a[ch] = a_load ? dz[a_off + row] : 0.0f;
        b[ch] = b_load ? b_scale * rec[b_off + row] : b_const;
      }
#pragma unroll
      for (int ch = 0; ch < 4; ++ch) acc = mfma16(a[ch], b[ch], acc);
    }
  }
  // D: register r of lane (m, q) is gate r of unit 4 t + q (torch row r H + unit) against input column m of the tile
  const int u_out = 4 * t + q;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long row = (long)r * H + u_out;
    const float v = acc[r];
    if (type == 0 && u_out < H) {
      if (m < nn.n_in) nn.w_ih1[row * nn.n_in + m] = v;
      if (m == 2) nn.b_ih1[row] = nn.b_hh1[row] = v;
    } else if (type >= 1 && type <= 3 && u_out < H && unit < H) {
      float* w = type == 1 ? nn.w_hh1 : (type == 2 ? nn.w_ih2 : nn.w_hh2);
      w[row * H + unit] = v;
    } else if (type == 4 && u_out < H && m == 2) {
      nn.b_ih2[row] = nn.b_hh2[row] = v;
    } else if (type == 5 && q == 0 && r == 0 && unit < H) {
      nn.w_out[unit] = v;
    }
  }
}

}  // namespace l2o
