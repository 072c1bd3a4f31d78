// l2o_confocal_unroll.h -- the fused persistent unroll for problems.confocal_microscopy_3d: T optimizer steps on one batch
// row in ONE launch (l2o_confocal_unroll / l2o_confocal_unroll_record).  Builds on l2o_confocal.h (the voxel model);
// written for gfx950 only.
//
// The rows of the confocal optimizee are independent problems (no batch norm, no minibatch; the loss is a plain mean over
// rows), so a row lives on one CU for all T steps, like a quadratic problem in k_unroll: one 256-thread workgroup (four
// waves, one per SIMD) per row, no cross-workgroup protocol, no status word.  Replaces, per step, the six launches of the
// step path (k_cf_slab, k_cf_reduce, the x-scale multiplies, k_cwlstm_step) and the Python around them.
//
//   LDS   : the row's TARGET VOLUME, already divided by its norm (it is constant over the unroll: built once from the
//           simulated points' tables -- or read once from `img` -- instead of P more multiply-adds per voxel and step;
//           4 V bytes, 86 KB at 28^3, 128 KB at 32^3, dynamic), the fitted points' tables (9 KB), two residual planes
//           (8 KB), x, x s, s, the RNNProp moments and the 6P + 1 reduced gradients.  25 KB static + 128 KB < 160 KB.
//   VGPR  : the LSTM state of the wave's tile (a row has 6P + 1 <= 49 coordinates = at most four 16-coordinate tiles: wave
//           w owns variables 16 w .. 16 w + 15, state never leaves its registers) and the bf16x3 optimizer weights pinned
//           in the accumulation half of the register file, as in k_unroll_cu.
//   HBM   : x / state / moments once in, once out; fx_part[t][b] per step; the history when recording.
//
// STATE LAYOUT: the coordinate (variable v, row b) lives in variable v's OWN packed state (l2o_state_floats(1, batch)
// floats: its batch rows are its coordinates) at tile b / 16, coordinate b % 16.  Lane (c, q) of wave w owns variable
// 16 w + c of this row, so it reads the 20 floats of lane 16 q + b % 16 of tile b / 16 of that variable's buffer, and
// writes them back the same way: the Python-side buffers keep their layout, and the step path, the recording path and
// back-propagation through time interoperate with no conversion.
//
// Per step: x s -> tables (cf_axis) -> all ry planes as k_cf_slab walks a slab (one residual plane in LDS, double
// buffered: one barrier per plane; sum r^2, sum r, the T1 / T2 contractions; the residual volume is never stored) ->
// the 6P + 1 gradients and the row loss into LDS in a fixed order (no atomics: two launches give the same bits) ->
// fx_part[t][b] -> waves w < ceil((6P + 1) / 16): g = grad s / batch, preprocess / RNNProp inputs, the LSTM, x += delta.
// Dead lanes (coordinate >= 6P + 1) feed zeros and write nothing; a wave with no tile skips the optimizer phase.
//
// SEVERAL INSTANCES (l2o_confocal_unroll_multi, include/l2o_confocal_multi_abi.h): the same kernel body with MULTI = true --
// workgroup i serves row i % batch of instance i / batch and reads its pointers from the instance's table in device memory
// (CfPtrs) instead of the kernel arguments.  Everything after the prologue is the same code, so the bits are the same.
#pragma once
#include "l2o_confocal.h"
#include "l2o_lstm_bx3.h"
#include "../../include/l2o_confocal_multi_abi.h"

namespace l2o {

// what every form of the unroll takes: the network, the shape (ONE descriptor for all instances), the step count
struct CfUnrollCommon {
  NetParams np;
  int batch, P, rx, ry, rz, inference, T;
  float rb;                           // 1 / batch
  float p1_hi, p1_lo, p2_hi, p2_lo;   // beta^step0 as float-float
};

// one instance: its buffers are kernel arguments
struct CfUnrollArgs : CfUnrollCommon {
  const float* img;                   // inference: [batch][ry][rx][rz]
  float* fx_part;                     // [T + 1][batch]
  // recording: device table [4][kCfMaxVars] of the history buffers st / g / m / v (k_cf_hist_table fills it)
  float* const* htab;
  float* x[kCfMaxVars];               // [batch] each
  float* st[kCfMaxVars];              // packed state of the variable, l2o_state_floats(1, batch) floats
  float* m[kCfMaxVars];               // RNNProp moments [batch], else unused
  float* v[kCfMaxVars];
  const float* xs[kCfMaxVars];        // x-scale [batch] or NULL (= 1)
  const float* sim[kCfMaxVars];       // simulation parameters [batch] (unused with inference)
};

// several instances (l2o_confocal_unroll_multi): N x six tables of 49 pointers cannot be kernel arguments, so every
// instance has a table of kCfInstPtrs pointers in device scratch -- [x | st | m | v | xs | sim][kCfMaxVars], the history
// table [st | g | m | v][kCfMaxVars] of a recording launch (the single form's htab), then img, fx_part and fx.
// k_cf_inst_table / k_cf_hist_table write it ahead of the unroll, in stream order.
constexpr int kCfTabHist = 6 * kCfMaxVars, kCfTabImg = 10 * kCfMaxVars, kCfTabFxPart = kCfTabImg + 1, kCfTabFx = kCfTabImg + 2;
constexpr int kCfInstPtrs = kCfTabImg + 4;
struct CfUnrollMultiArgs : CfUnrollCommon {
  float* const* tab;                  // [n_inst][kCfInstPtrs]
};

// where the kernel's pointers come from -- the ONE difference between the two forms.  row(): the batch row of this workgroup
// (several instances: workgroup i serves row i % batch of instance i / batch).
template <bool MULTI> struct CfPtrs;
template <> struct CfPtrs<false> {
  typedef CfUnrollArgs Args;
  const CfUnrollArgs& a;
  __device__ explicit CfPtrs(const CfUnrollArgs& a_) : a(a_) {}
  __device__ int row() const { return blockIdx.x; }
  __device__ float* x(int k) const { return a.x[k]; }
  __device__ float* st(int k) const { return a.st[k]; }
  __device__ float* m(int k) const { return a.m[k]; }
  __device__ float* v(int k) const { return a.v[k]; }
  __device__ const float* xs(int k) const { return a.xs[k]; }
  __device__ const float* sim(int k) const { return a.sim[k]; }
  __device__ const float* img() const { return a.img; }
  __device__ float* fx_part() const { return a.fx_part; }
  __device__ float* const* htab() const { return a.htab; }
};
template <> struct CfPtrs<true> {
  typedef CfUnrollMultiArgs Args;
  float* const* tab;                  // this instance's table
  int b;
  __device__ explicit CfPtrs(const CfUnrollMultiArgs& a) {
    const int inst = blockIdx.x / a.batch;
    b = blockIdx.x - inst * a.batch;
    tab = a.tab + (size_t)inst * kCfInstPtrs;
  }
  __device__ int row() const { return b; }
  __device__ float* x(int k) const { return tab[k]; }
  __device__ float* st(int k) const { return tab[kCfMaxVars + k]; }
  __device__ float* m(int k) const { return tab[2 * kCfMaxVars + k]; }
  __device__ float* v(int k) const { return tab[3 * kCfMaxVars + k]; }
  __device__ const float* xs(int k) const { return tab[4 * kCfMaxVars + k]; }
  __device__ const float* sim(int k) const { return tab[5 * kCfMaxVars + k]; }
  __device__ const float* img() const { return tab[kCfTabImg]; }
  __device__ float* fx_part() const { return tab[kCfTabFxPart]; }
  __device__ float* const* htab() const { return tab + kCfTabHist; }
};

// the history pointers of a recording launch do not fit the kernel arguments beside the six tables above: a launch of
// its own leaves them in device scratch ahead of the unroll (stream order)
struct CfHistPtrs { float* p[4][kCfMaxVars]; };
__global__ void k_cf_hist_table(CfHistPtrs h, float** tab) {
  const int i = threadIdx.x;
  if (i < 4 * kCfMaxVars) tab[i] = h.p[i / kCfMaxVars][i % kCfMaxVars];
}

// the multi form's tables: one instance's pointers arrive as kernel arguments and are written out (as k_cf_hist_table)
struct CfInstPtrs { float* p[6][kCfMaxVars]; float* img; float* fx_part; float* fx; };
__global__ void k_cf_inst_table(CfInstPtrs h, float** tab) {
  const int i = threadIdx.x;
  if (i < 6 * kCfMaxVars) tab[i] = h.p[i / kCfMaxVars][i % kCfMaxVars];
  else if (i == 6 * kCfMaxVars) tab[kCfTabImg] = h.img;
  else if (i == 6 * kCfMaxVars + 1) tab[kCfTabFxPart] = h.fx_part;
  else if (i == 6 * kCfMaxVars + 2) tab[kCfTabFx] = h.fx;
}

// every instance's batch mean, in k_reduce_fx's order (the same bits): block (t, instance)
__global__ void k_cf_reduce_fx_multi(float* const* tab, int B, float inv_b) {
  float* const* it = tab + (size_t)blockIdx.y * kCfInstPtrs;
  const float* fx_part = it[kCfTabFxPart];
  const int t = blockIdx.x, lane = threadIdx.x;   // 64 threads
  float acc = 0.0f;
  for (int b = lane; b < B; b += 64) acc += fx_part[(size_t)t * B + b];
  acc = wave_sum64(acc);
  if (lane == 0) it[kCfTabFx][t] = acc * inv_b;
}

// rnnprop_inputs (l2o_common.h) with the two moment updates' multiply-adds SPELLED OUT.  `beta1 * m + omb1 * g` leaves the
// compiler the choice of which product to fuse, and it chose differently in the MULTI = true instantiation than in the
// single form (1-ulp moments, measured); written as the fmaf the single form has always been compiled to, both forms --
// and any later instantiation -- round alike.  The rest is rnnprop_inputs' arithmetic, which has no such choice in it.
__device__ __forceinline__ void cf_rnnprop_inputs(float g, float& m, float& v, float beta1, float beta2, float omb1,
                                                  float omb2, float om1, float om2, float& m_tilde, float& g_tilde) {
  const float mg = omb1 * g, vg = omb2 * g * g;
  m = __builtin_fmaf(beta1, m, mg);
  v = __builtin_fmaf(beta2, v, vg);
  const float m_hat = m * fast_rcp(om1);
  const float v_hat = v * fast_rcp(om2);
  const float inv = fast_rcp(__builtin_amdgcn_sqrtf(v_hat) + 1e-8f);
  m_tilde = m_hat * inv;
  g_tilde = g * inv;
}

template <int PRE, bool HIST, bool MULTI = false>
__global__ __launch_bounds__(kCfThreads) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_cf_unroll(
    typename CfPtrs<MULTI>::Args a) {
  const CfPtrs<MULTI> pt(a);
  extern __shared__ float cf_tg[];                                                     // [ry][rx][rz] target / its norm
  __shared__ float sE[3][kCfMaxPts][32], sDc[3][kCfMaxPts][32], sDs[3][kCfMaxPts][32];   // the fitted points' tables
  __shared__ float sT[3][kCfMaxPts][32];                                               // the simulated points' E (prologue)
  __shared__ float sGram[3][kCfMaxPts][kCfMaxPts + 1];
  __shared__ float sCy[kCfMaxPts][32];                                                 // I0 / 8 Ey[iy] per point
  __shared__ float sR[2][32][33];                                                      // two planes of the residual
  __shared__ float sSim[kCfMaxVars + 3], sCs[kCfMaxPts];
  __shared__ float xL[64], xsL[64], scL[64], mL[64], vL[64], sG[64];
  __shared__ float red[4];
  __shared__ __attribute__((aligned(16))) float bias_s[bx::kBiasWords];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, q = lane >> 4;
  const int b = pt.row(), B = a.batch;
  const int P = a.P, nv = 6 * P + 1, rx = a.rx, ry = a.ry, rz = a.rz;
  const int V = rx * ry * rz;
  const bool sim = !a.inference;

  // ---- the row's values, scales and moments ------------------------------------------------------------------------------
  if (tid < 64) {
    const bool live = tid < nv;
    const float xv = live ? pt.x(tid)[b] : 0.f;
    const float sc = (live && pt.xs(tid)) ? pt.xs(tid)[b] : 1.f;
    xL[tid] = xv; scL[tid] = sc; xsL[tid] = xv * sc;
    mL[tid] = (PRE == L2O_PRE_FC_ELU && live) ? pt.m(tid)[b] : 0.f;
    vL[tid] = (PRE == L2O_PRE_FC_ELU && live) ? pt.v(tid)[b] : 0.f;
    sG[tid] = 0.f;
  } else if (sim && tid < 64 + nv) {
    sSim[tid - 64] = pt.sim(tid - 64)[b];
  }
  // ---- the LSTM: weights, and the state of this lane's coordinate out of the variable's own packed buffer ------------------
  const int var = 16 * wv + c;
  const bool live = var < nv;
  const bool has_tile = 16 * wv < nv;                                                   // (wave-uniform)
  const int st_lane = 16 * q + (b & 15);
  const size_t st_tile = (size_t)(b >> 4) * kStateFloatsPerTile;
  const size_t st_floats = (size_t)((B + kTile - 1) / kTile) * kStateFloatsPerTile;
  TileState s;
#pragma unroll
  for (int t5 = 0; t5 < kNT; ++t5) { s.h1[t5] = 0.f; s.c1[t5] = 0.f; s.h2[t5] = 0.f; s.c2[t5] = 0.f; }
  if (live) load_tile_state(s, pt.st(var) + st_tile, st_lane);
  constexpr bool PK = bx::packed_default(PRE);
  bx::NetWB<PRE, PK> w;
  bx::load_netw<PRE, true, PK>(w, a.np.wpack, lane);
  bx::stage_bias(bias_s, a.np.wpack, PRE, tid, kCfThreads);
  bx::set_bias(w, bias_s, q);
#pragma unroll
  for (int ch = 0; ch < bx::NetWB<PRE, PK>::NCH; ++ch)
#pragma unroll
    for (int t5 = 0; t5 < kNT; ++t5)
#pragma unroll
      for (int s3 = 0; s3 < bx::frags(PK); ++s3) asm volatile("" : "+a"(w.a[ch][t5][s3]));
  float p1h = a.p1_hi, p1l = a.p1_lo, p2h = a.p2_hi, p2l = a.p2_lo;
  float om1 = 1.0f, om2 = 1.0f;
  __syncthreads();

  // the voxels of a plane: thread (ix0, iz) takes ix = ix0, ix0 + 8, ...
  const int iz = tid & 31, ix0 = tid >> 5;

  // ---- the target, divided by its norm, into LDS (constant over the unroll) ------------------------------------------------
  if (sim) {
    if (tid < kCfMaxPts) sCs[tid] = tid < P ? 0.125f * (0.5f + 1.5f * sSim[6 * tid]) : 0.f;
    for (int i = tid; i < 3 * P * 32; i += kCfThreads) {
      const int axis = i / (P * 32), rem = i - axis * (P * 32), p = rem >> 5, k = rem & 31;
      const int R = axis == 0 ? rx : axis == 1 ? ry : rz;
      float E = 0.f, d0, d1;
      if (k < R) cf_axis(0.5f + ((float)R - 1.5f) * sSim[6 * p + 1 + axis], 2.f + 2.f * sSim[6 * p + (axis < 2 ? 4 : 5)], k, E, d0, d1);
      sT[axis][p][k] = E;
    }
    __syncthreads();
    // 1 / norm in the exact separable Gram form of k_cf_slab
    for (int i = tid; i < 3 * P * (P + 1); i += kCfThreads) {
      const int axis = i / (P * (P + 1)), rem = i - axis * (P * (P + 1)), p = rem / (P + 1), qq = rem - p * (P + 1);
      const int R = axis == 0 ? rx : axis == 1 ? ry : rz;
      float sum = 0.f;
      if (qq < P) for (int k = 0; k < R; ++k) sum = fmaf(sT[axis][p][k], sT[axis][qq][k], sum);
      else for (int k = 0; k < R; ++k) sum += sT[axis][p][k];
      sGram[axis][p][qq < P ? qq : kCfMaxPts] = sum;
    }
    __syncthreads();
    const float bgs = sSim[6 * P];
    float n2 = 0.f, lin = 0.f;                       // every thread the same arithmetic: no broadcast needed
    for (int p = 0; p < P; ++p) {
      for (int qq = 0; qq < P; ++qq) n2 = fmaf(sCs[p] * sCs[qq], sGram[0][p][qq] * sGram[1][p][qq] * sGram[2][p][qq], n2);
      lin = fmaf(sCs[p], sGram[0][p][kCfMaxPts] * sGram[1][p][kCfMaxPts] * sGram[2][p][kCfMaxPts], lin);
    }
    n2 += 2.f * bgs * lin + (float)V * bgs * bgs;
    const float inv = 1.0f / sqrtf(fmaxf(n2, 1e-12f));
    if (iz < rz) {
      for (int iy = 0; iy < ry; ++iy)
        for (int ix = ix0; ix < rx; ix += 8) {
          float tg = bgs;
          for (int p = 0; p < P; ++p) tg = fmaf(sCs[p] * sT[1][p][iy], sT[0][p][ix] * sT[2][p][iz], tg);
          cf_tg[(iy * rx + ix) * rz + iz] = tg * inv;
        }
    }
  } else {
    const float* row = pt.img() + (size_t)b * V;
    float n2 = 0.f;
    for (int i = tid; i < V; i += kCfThreads) { const float t = row[i]; cf_tg[i] = t; n2 = fmaf(t, t, n2); }
    n2 = cf_block_sum(n2, red);
    const float inv = 1.0f / sqrtf(fmaxf(n2, 1e-12f));
    for (int i = tid; i < V; i += kCfThreads) cf_tg[i] *= inv;                           // (every thread its own elements)
  }
  __syncthreads();

  float* const* htab = pt.htab();
  const int pp = tid >> 5, k = tid & 31;                                                // contraction role: point pp, index k
  for (int t = 0;; ++t) {
    const bool want_g = t < a.T || HIST;                                                // (recording: the gradient at x_T too)
    // ---- the fitted points' tables at x s --------------------------------------------------------------------------------
    for (int i = tid; i < 3 * P * 32; i += kCfThreads) {
      const int axis = i / (P * 32), rem = i - axis * (P * 32), p = rem >> 5, kk = rem & 31;
      const int R = axis == 0 ? rx : axis == 1 ? ry : rz;
      float E = 0.f, dc = 0.f, ds = 0.f;
      if (kk < R) cf_axis(0.5f + ((float)R - 1.5f) * xsL[6 * p + 1 + axis], 2.f + 2.f * xsL[6 * p + (axis < 2 ? 4 : 5)], kk, E, dc, ds);
      sE[axis][p][kk] = E; sDc[axis][p][kk] = dc; sDs[axis][p][kk] = ds;
      if (axis == 1) sCy[p][kk] = 0.125f * (0.5f + 1.5f * xsL[6 * p]) * E;
    }
    __syncthreads();
    // ---- the planes: residual, its sums, the contractions ---------------------------------------------------------------
    const float bg = xsL[6 * P];
    const bool grad_thread = want_g && pp < P;
    float acc_l = 0.f, acc_b = 0.f, gx = 0.f, gz = 0.f, ay0 = 0.f, asy = 0.f;
    for (int iy = 0; iy < ry; ++iy) {
      float (*R)[33] = sR[iy & 1];
      if (iz < rz) {
        for (int ix = ix0; ix < rx; ix += 8) {
          float pr = bg;
          for (int p = 0; p < P; ++p) pr = fmaf(sCy[p][iy], sE[0][p][ix] * sE[2][p][iz], pr);
          const float r = pr - cf_tg[(iy * rx + ix) * rz + iz];
          R[ix][iz] = r;
          acc_l = fmaf(r, r, acc_l);
          acc_b += r;
        }
      }
      // one barrier per plane: a thread writes plane iy + 1 into the other buffer only after this barrier, which every
      // thread reaches after its contraction of plane iy - 1 (the last reader of that buffer)
      __syncthreads();
      if (grad_thread) {
        float t1 = 0.f, t2 = 0.f;
        if (k < rx) for (int jz = 0; jz < rz; ++jz) t1 = fmaf(R[k][jz], sE[2][pp][jz], t1);
        if (k < rz) for (int jx = 0; jx < rx; ++jx) t2 = fmaf(R[jx][k], sE[0][pp][jx], t2);
        const float ey = sE[1][pp][iy], u = sE[0][pp][k] * t1;
        gx = fmaf(ey, t1, gx);
        gz = fmaf(ey, t2, gz);
        ay0 = fmaf(sDc[1][pp][iy], u, ay0);
        asy = fmaf(sDs[1][pp][iy], u, asy);
      }
    }
    // ---- the row loss and the 6P + 1 gradients, fixed order ------------------------------------------------------------
    const float loss = cf_block_sum(acc_l, red);
    if (tid == 0) pt.fx_part()[(size_t)t * B + b] = loss;
    if (!want_g) break;                                                                 // (uniform)
    const float sum_r = cf_block_sum(acc_b, red);
    {
      const int p = pp < P ? pp : 0;
      float g6[6];
      g6[0] = sE[0][p][k] * gx;                           // I0
      g6[1] = sDc[0][p][k] * gx;                          // x0
      g6[2] = ay0;                                        // y0
      g6[3] = sDc[2][p][k] * gz;                          // z0
      g6[4] = fmaf(sDs[0][p][k], gx, asy);                // sigma_xy: the x and the y axis
      g6[5] = sDs[2][p][k] * gz;                          // sigma_z
#pragma unroll
      for (int j = 0; j < 6; ++j) g6[j] = cf_half_sum(g6[j]);
      if (pp < P && k == 0) {
        const float c2 = 2.f * (0.125f * (0.5f + 1.5f * xsL[6 * p]));
        sG[6 * p + 0] = 0.25f * 1.5f * g6[0];
        sG[6 * p + 1] = c2 * ((float)rx - 1.5f) * g6[1];
        sG[6 * p + 2] = c2 * ((float)ry - 1.5f) * g6[2];
        sG[6 * p + 3] = c2 * ((float)rz - 1.5f) * g6[3];
        sG[6 * p + 4] = c2 * 2.f * g6[4];
        sG[6 * p + 5] = c2 * 2.f * g6[5];
      }
      if (tid == 0) sG[6 * P] = 2.f * sum_r;
    }
    __syncthreads();

    // ---- the optimizer network on this wave's tile -----------------------------------------------------------------------
    if (has_tile) {
      const float sc = scL[var];
      const float gv = live ? sG[var] * a.rb * sc : 0.f;
      if (HIST && t == a.T) {                                                           // the gradient at x_T, then done
        if (live && q == 0) htab[kCfMaxVars + var][(size_t)t * B + b] = gv;
      } else {
        if (HIST && live) {
          float* hs = htab[var] + (size_t)t * st_floats + st_tile;
          store_tile_state(s, hs, st_lane);
          if (b == B - 1) {                                                             // the unused coordinates of the last tile
            TileState z;
#pragma unroll
            for (int t5 = 0; t5 < kNT; ++t5) { z.h1[t5] = 0.f; z.c1[t5] = 0.f; z.h2[t5] = 0.f; z.c2[t5] = 0.f; }
            for (int cc = (b & 15) + 1; cc < kTile; ++cc) store_tile_state(z, hs, 16 * q + cc);
          }
          if (q == 0) htab[kCfMaxVars + var][(size_t)t * B + b] = gv;
        }
        float in0, in1;
        if (PRE == L2O_PRE_FC_ELU) {
          om1 = 1.0f - p1h; om2 = 1.0f - p2h;
          float m = mL[var], v = vL[var];
          cf_rnnprop_inputs(gv, m, v, a.np.beta1, a.np.beta2, a.np.omb1, a.np.omb2, om1, om2, in0, in1);
          if (!live) { in0 = 0.0f; in1 = 0.0f; }
          if (live && q == 0) {
            mL[var] = m; vL[var] = v;
            if (HIST) {
              htab[2 * kCfMaxVars + var][(size_t)(t + 1) * B + b] = m;
              htab[3 * kCfMaxVars + var][(size_t)(t + 1) * B + b] = v;
            }
          }
        } else {
          preprocess_grad<PRE>(gv, a.np.k_inv_ln2, a.np.exp_k, in0, in1);
        }
        float d = bx::tile_step<PRE>(w, s, in0, in1, q);
        if (a.np.tanh_output) d = tanhf_(d);
        d *= a.np.scale;
        if (live && q == 0) { const float xn = xL[var] + d; xL[var] = xn; xsL[var] = xn * sc; }
      }
    }
    if (HIST && t == a.T) break;
    if (PRE == L2O_PRE_FC_ELU) {                              // beta^k as a float-float running product
      float hi = p1h * a.np.beta1, er = __builtin_fmaf(p1h, a.np.beta1, -hi);
      float lo = __builtin_fmaf(p1l, a.np.beta1, er), sum = hi + lo;
      p1l = lo - (sum - hi); p1h = sum;
      hi = p2h * a.np.beta2; er = __builtin_fmaf(p2h, a.np.beta2, -hi);
      lo = __builtin_fmaf(p2l, a.np.beta2, er); sum = hi + lo;
      p2l = lo - (sum - hi); p2h = sum;
    }
    __syncthreads();                                          // x s of the next step complete, sG free
  }

  // ---- write back: x, moments, LSTM state (the coordinates of this row only) ---------------------------------------------
  __syncthreads();
  if (tid < nv) {
    pt.x(tid)[b] = xL[tid];
    if (PRE == L2O_PRE_FC_ELU) { pt.m(tid)[b] = mL[tid]; pt.v(tid)[b] = vL[tid]; }
  }
  if (live) store_tile_state(s, pt.st(var) + st_tile, st_lane);
}

}  // namespace l2o
