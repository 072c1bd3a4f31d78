// l2o_confocal.h -- forward + gradient of problems.confocal_microscopy_3d (DM/problems.py:701-956; DM/util.py:215-222):
// per batch row, a sum of P Gaussian point-spread functions, each integrated over the voxels of an Rx x Ry x Rz region of
// interest, plus a background value, fitted to an l2-normalised target volume:
//   loss = mean_b sum_v (pred - target)^2,  pred = sum_p I0 Ex[ix] Ey[iy] Ez[iz] / 8 + bg,
//   E[k] = erf((k + 0.5 - c) / (sqrt2 sigma)) - erf((k - 0.5 - c) / (sqrt2 sigma)),
// with (I0, x0, y0, z0, sigma_xy, sigma_z) affine in the raw trainable values (the quantiles of uniform priors, not
// clipped).  The target is the same sum over the simulation parameters, or a supplied volume (inference) whose flat voxel
// index is (iy Rx + ix) Rz + iz.  The step-granular evaluation l2o_confocal_fg; included by l2o_confocal.hip; written for
// gfx950 only.
//
// The image of a point is separable, so everything is computed from per-point, per-axis tables of at most 32 entries
// (E, dE/dc, dE/dsigma) that live in LDS.  A problem (batch row) is split into slabs of consecutive iy planes, one
// workgroup per (row, slab), so that the default shape (32 rows) fills the device instead of 32 of its 256 CUs; every
// workgroup rebuilds the row's tables (about 1000 erf and 500 exp per workgroup at 5 points).  THE RESIDUAL
// VOLUME IS NEVER STORED: a workgroup holds one iy plane of it (at most 32 x 32 floats) in LDS, takes the plane's two
// contractions T1[ix] = sum_iz r Ez[iz] and T2[iz] = sum_ix r Ex[ix] per point, folds them into running sums, and moves to
// the next plane -- 86 KB per row at 28^3 would cost the LDS that co-resident workgroups need, and a global round trip
// would cost more than recomputing nothing: every voxel is still evaluated exactly once.
//
// Two launches per evaluation (three in inference mode), fp32, every reduction in a fixed order (no atomics: two calls on
// the same inputs are bit-identical; the loss takes the same path with and without gradients):
//   k_cf_norm     inference only, one workgroup per row: 1 / max(|img row|, 1e-6)
//   k_cf_slab     one workgroup per (row, slab): tables; in simulation mode the target's norm in the exact separable Gram
//                 form sum_pq c_p c_q prod_axis <E_p, E_q> + 2 bg sum_p c_p prod_axis <E_p, 1> + V bg^2 (the same
//                 arithmetic in every workgroup of a row); per plane the residual, its square sum and the contractions;
//                 the slab's share of the 6P + 1 gradients (prior scales and the factor 2 applied) and of the loss
//   k_cf_reduce   one thread per (variable, row): the slabs in order, times 1 / batch; workgroup 0 also the mean loss
// erf differences in the tails are taken as erfc differences, so a point far outside the volume keeps full relative
// accuracy in its (tiny) image instead of the rounding noise of 1 - 1.
#pragma once
#include "l2o_params.h"

namespace l2o {

constexpr int kCfThreads = 256;
constexpr int kCfMaxBatch = 1024, kCfMaxPts = 8, kCfMinEdge = 2, kCfMaxEdge = 32;
constexpr int kCfMaxVars = 6 * kCfMaxPts + 1;       // 49: per point I, x, y, z, sigmaxy, sigmaz; then bg
constexpr int kCfPart = 6 * kCfMaxPts + 2;          // a (row, slab)'s partial: the 6P + 1 gradients, then its loss share
constexpr int kCfTargetWgs = 512;                   // slabs are sized so that batch x slabs is about two workgroups per CU

struct CfArgs {
  int batch, P, rx, ry, rz, slab, nslab, inference, want_grad;
  const float* img;                   // inference: [batch][ry][rx][rz]
  float* inv;                         // inference: [batch] 1 / norm of the image row
  float* part;                        // [nslab][kCfPart][batch]
  float* loss;                        // [1]
  const float* th[kCfMaxVars];        // [batch] each
  const float* sim[kCfMaxVars];
  float* g[kCfMaxVars];
};

// sum over the 32 lanes of a wave half (lanes 0-31 / 32-63), in a fixed order; result in all 32
__device__ __forceinline__ float cf_half_sum(float v) { return xor16_add(row_sum16(v)); }

// workgroup sum in a fixed order (wave butterflies, then the four waves in order); red: >= 4 floats; result in every thread
__device__ __forceinline__ float cf_block_sum(float v, float* red) {
  v = wave_sum64(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// E[k] of one axis and its derivatives with respect to the centre c and the width sg (sg > 0 is the caller's business)
__device__ __forceinline__ void cf_axis(float c, float sg, int k, float& E, float& dc, float& ds) {
  const float is = 0.70710678118654752f / sg;
  const float am = ((float)k - 0.5f - c) * is, ap = ((float)k + 0.5f - c) * is;
  if (am > 0.5f) E = erfcf(am) - erfcf(ap);
  else if (ap < -0.5f) E = erfcf(-ap) - erfcf(-am);
  else E = erff(ap) - erff(am);
  const float gm = expf(-am * am), gp = expf(-ap * ap);
  constexpr float kTwoRsqrtPi = 1.12837916709551257f;
  dc = (gm - gp) * (kTwoRsqrtPi * is);
  ds = (am * gm - ap * gp) * (kTwoRsqrtPi / sg);
}

__device__ __forceinline__ int cf_edge(const CfArgs& a, int axis) { return axis == 0 ? a.rx : axis == 1 ? a.ry : a.rz; }

__global__ __launch_bounds__(kCfThreads) void k_cf_norm(CfArgs a) {
  __shared__ float red[4];
  const int b = blockIdx.x, V = a.rx * a.ry * a.rz;
  const float* row = a.img + (size_t)b * V;
  float s = 0.f;
  for (int v = threadIdx.x; v < V; v += kCfThreads) s = fmaf(row[v], row[v], s);
  s = cf_block_sum(s, red);
  if (threadIdx.x == 0) a.inv[b] = 1.0f / sqrtf(fmaxf(s, 1e-12f));
}

__global__ __launch_bounds__(kCfThreads) void k_cf_slab(CfArgs a) {
  __shared__ float sE[3][kCfMaxPts][32], sDc[3][kCfMaxPts][32], sDs[3][kCfMaxPts][32];   // the fitted points' tables
  __shared__ float sT[3][kCfMaxPts][32];                                               // the simulated points' E
  __shared__ float sGram[3][kCfMaxPts][kCfMaxPts + 1];                                 // <E_p, E_q>; [..][p][8] = <E_p, 1>
  __shared__ float sR[32][33];                                                         // one plane of the residual
  __shared__ float sRaw[2][kCfMaxVars + 3];
  __shared__ float sC[2][kCfMaxPts];                                                   // I0 / 8 of the fitted / simulated points
  __shared__ float red[4];
  const int b = blockIdx.x, slab = blockIdx.y, tid = threadIdx.x;
  const int P = a.P, nv = 6 * P + 1, rx = a.rx, ry = a.ry, rz = a.rz;
  const bool sim = !a.inference;

  if (tid < nv) sRaw[0][tid] = a.th[tid][b];
  else if (sim && tid >= 64 && tid < 64 + nv) sRaw[1][tid - 64] = a.sim[tid - 64][b];
  __syncthreads();
  if (tid < 2 * kCfMaxPts) {
    const int w = tid >> 3, p = tid & 7;
    sC[w][p] = (p < P && (w == 0 || sim)) ? 0.125f * (0.5f + 1.5f * sRaw[w][6 * p]) : 0.f;
  }
  for (int i = tid; i < 3 * P * 32; i += kCfThreads) {
    const int axis = i / (P * 32), rem = i - axis * (P * 32), p = rem >> 5, k = rem & 31;
    const int R = cf_edge(a, axis);
    const float span = (float)R - 1.5f;
    float E = 0.f, dc = 0.f, ds = 0.f, Es = 0.f;
    if (k < R) {
      cf_axis(0.5f + span * sRaw[0][6 * p + 1 + axis], 2.f + 2.f * sRaw[0][6 * p + (axis < 2 ? 4 : 5)], k, E, dc, ds);
      if (sim) {
        float d0, d1;
        cf_axis(0.5f + span * sRaw[1][6 * p + 1 + axis], 2.f + 2.f * sRaw[1][6 * p + (axis < 2 ? 4 : 5)], k, Es, d0, d1);
      }
    }
    sE[axis][p][k] = E; sDc[axis][p][k] = dc; sDs[axis][p][k] = ds; sT[axis][p][k] = Es;
  }
  __syncthreads();

  // 1 / norm of the target
  float inv, bgs = 0.f;
  if (sim) {
    for (int i = tid; i < 3 * P * (P + 1); i += kCfThreads) {
      const int axis = i / (P * (P + 1)), rem = i - axis * (P * (P + 1)), p = rem / (P + 1), q = rem - p * (P + 1);
      const int R = cf_edge(a, axis);
      float s = 0.f;
      if (q < P) for (int k = 0; k < R; ++k) s = fmaf(sT[axis][p][k], sT[axis][q][k], s);
      else for (int k = 0; k < R; ++k) s += sT[axis][p][k];
      sGram[axis][p][q < P ? q : kCfMaxPts] = s;
    }
    __syncthreads();
    bgs = sRaw[1][6 * P];
    float n2 = 0.f, lin = 0.f;                       // every thread the same arithmetic: no broadcast needed
    for (int p = 0; p < P; ++p) {
      for (int q = 0; q < P; ++q) n2 = fmaf(sC[1][p] * sC[1][q], sGram[0][p][q] * sGram[1][p][q] * sGram[2][p][q], n2);
      lin = fmaf(sC[1][p], sGram[0][p][kCfMaxPts] * sGram[1][p][kCfMaxPts] * sGram[2][p][kCfMaxPts], lin);
    }
    n2 += 2.f * bgs * lin + (float)(rx * ry * rz) * bgs * bgs;
    inv = 1.0f / sqrtf(fmaxf(n2, 1e-12f));
  } else {
    inv = a.inv[b];
  }

  const float bg = sRaw[0][6 * P];
  const int nvox = rx * rz, pp = tid >> 5, k = tid & 31;
  const bool grad_thread = a.want_grad && pp < P;
  const int y0 = slab * a.slab, y1 = min(ry, y0 + a.slab);
  const float* img = a.inference ? a.img + (size_t)b * ry * nvox : nullptr;
  float acc_l = 0.f, acc_b = 0.f, gx = 0.f, gz = 0.f, ay0 = 0.f, asy = 0.f;
  for (int iy = y0; iy < y1; ++iy) {
    for (int v = tid; v < nvox; v += kCfThreads) {
      const int ix = v / rz, iz = v - ix * rz;
      float pr = bg, tg;
      for (int p = 0; p < P; ++p) pr = fmaf(sC[0][p] * sE[1][p][iy], sE[0][p][ix] * sE[2][p][iz], pr);
      if (sim) {
        tg = bgs;
        for (int p = 0; p < P; ++p) tg = fmaf(sC[1][p] * sT[1][p][iy], sT[0][p][ix] * sT[2][p][iz], tg);
      } else {
        tg = img[iy * nvox + v];
      }
      const float r = fmaf(-tg, inv, pr);
      sR[ix][iz] = r;
      acc_l = fmaf(r, r, acc_l);
      acc_b += r;
    }
    __syncthreads();
    if (grad_thread) {
      float t1 = 0.f, t2 = 0.f;
      if (k < rx) for (int iz = 0; iz < rz; ++iz) t1 = fmaf(sR[k][iz], sE[2][pp][iz], t1);
      if (k < rz) for (int ix = 0; ix < rx; ++ix) t2 = fmaf(sR[ix][k], sE[0][pp][ix], t2);
      const float ey = sE[1][pp][iy], u = sE[0][pp][k] * t1;
      gx = fmaf(ey, t1, gx);
      gz = fmaf(ey, t2, gz);
      ay0 = fmaf(sDc[1][pp][iy], u, ay0);
      asy = fmaf(sDs[1][pp][iy], u, asy);
    }
    __syncthreads();
  }

  float* part = a.part + (size_t)slab * kCfPart * a.batch + b;
  const float loss = cf_block_sum(acc_l, red);
  if (tid == 0) part[(size_t)(6 * P + 1) * a.batch] = loss;
  if (!a.want_grad) return;                          // (uniform)
  const float sum_r = cf_block_sum(acc_b, red);
  if (tid == 0) part[(size_t)(6 * P) * a.batch] = 2.f * sum_r;
  // the six gradients of point pp: sums over k of the table entries times the contracted residual (tables are 0 past
  // the edges, and so are gx / gz there)
  const int p = pp < P ? pp : 0;
  float q[6];
  q[0] = sE[0][p][k] * gx;                           // I0
  q[1] = sDc[0][p][k] * gx;                          // x0
  q[2] = ay0;                                        // y0
  q[3] = sDc[2][p][k] * gz;                          // z0
  q[4] = fmaf(sDs[0][p][k], gx, asy);                // sigma_xy: the x and the y axis
  q[5] = sDs[2][p][k] * gz;                          // sigma_z
#pragma unroll
  for (int j = 0; j < 6; ++j) q[j] = cf_half_sum(q[j]);
  if (pp < P && k == 0) {
    const float c2 = 2.f * sC[0][p];
    part[(size_t)(6 * p + 0) * a.batch] = 0.25f * 1.5f * q[0];
    part[(size_t)(6 * p + 1) * a.batch] = c2 * ((float)rx - 1.5f) * q[1];
    part[(size_t)(6 * p + 2) * a.batch] = c2 * ((float)ry - 1.5f) * q[2];
    part[(size_t)(6 * p + 3) * a.batch] = c2 * ((float)rz - 1.5f) * q[3];
    part[(size_t)(6 * p + 4) * a.batch] = c2 * 2.f * q[4];
    part[(size_t)(6 * p + 5) * a.batch] = c2 * 2.f * q[5];
  }
}

// the slabs' shares of one value, summed in slab order; every load is issued before the first add (the shares were written
// by other CUs: a load-add chain would pay the memory latency once per slab)
__device__ __forceinline__ float cf_slab_sum(const float* src, size_t stride, int nslab) {
  float v[kCfMaxEdge];
#pragma unroll
  for (int sl = 0; sl < kCfMaxEdge; ++sl) v[sl] = sl < nslab ? src[sl * stride] : 0.f;
  float s = 0.f;
#pragma unroll
  for (int sl = 0; sl < kCfMaxEdge; ++sl) s += v[sl];
  return s;
}

__global__ __launch_bounds__(kCfThreads) void k_cf_reduce(CfArgs a) {
  __shared__ float red[4];
  const int nv = 6 * a.P + 1, B = a.batch;
  const float rb = 1.0f / (float)B;
  const size_t stride = (size_t)kCfPart * B;
  if (a.want_grad) {
    const int i = blockIdx.x * kCfThreads + threadIdx.x;
    if (i < nv * B) {
      const int var = i / B, b = i - var * B;
      a.g[var][b] = cf_slab_sum(a.part + (size_t)var * B + b, stride, a.nslab) * rb;
    }
  }
  if (blockIdx.x == 0) {
    float s = 0.f;
    for (int b = threadIdx.x; b < B; b += kCfThreads) {
      s += cf_slab_sum(a.part + (size_t)nv * B + b, stride, a.nslab);
    }
    s = cf_block_sum(s, red);
    if (threadIdx.x == 0) a.loss[0] = s * rb;
  }
}

}  // namespace l2o
