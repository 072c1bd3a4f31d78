// l2o_problem_fg.h -- optimizee forward + gradient at arbitrary sizes, and the separable term of its Hessian-vector product.
#pragma once
#include "l2o_params.h"

// ---------------------------------------------------------------------------
// K2: optimizee forward + gradient for arbitrary sizes (matrix streamed from HBM/L2).
// One 256-thread workgroup per problem.
//   pass 1  r = W xs - y      rows over waves, columns over lanes (coalesced), wave reduce
//   pass 2  g = W^T r         columns over threads (coalesced), rows split over thread groups
// ---------------------------------------------------------------------------
constexpr int kFgThreads = 512;
constexpr int kFgWaves = kFgThreads / 64;

__device__ __forceinline__ float block_sum_fg(float v, float* red /* >= kFgWaves floats */) {
  v = wave_sum64(v);
  const int wv = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[wv] = v;
  __syncthreads();
  float s = red[0];
#pragma unroll
  for (int k = 1; k < kFgWaves; ++k) s += red[k];
  return s;
}

// VEC = true: D % 4 == 0 and 16-byte aligned rows -> dwordx4 loads, 4 rows (r pass) /
// 4 row-strided loads (g pass) in flight per lane; VEC = false: scalar fallback.
template <bool VEC>
__global__ __launch_bounds__(kFgThreads) void k_problem_fg(ProbParams pp, const float* __restrict__ x,
                                                            float* __restrict__ f_part,
                                                            float* __restrict__ gout) {
  extern __shared__ float sm[];
  const int D = pp.D, M = pp.M;
  float* xs = sm;                       // [D4]  scaled x (padded to a multiple of 4)
  const int D4 = (D + 3) & ~3;
  float* rs = xs + D4;                  // [M]   residual
  float* part = rs + ((M + 3) & ~3);    // [4 * kFgThreads] partial column sums
  float* red = part + 4 * kFgThreads;   // [kFgWaves]
  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float* xb = x + (size_t)b * D;
  const float* sb = pp.x_scale ? pp.x_scale + (size_t)b * D : nullptr;

  float facc = 0.0f;   // per-thread contribution to f_b
  for (int j = tid; j < D4; j += kFgThreads) {
    float xv = 0.0f;
    if (j < D) {
      xv = xb[j] * (sb ? sb[j] : 1.0f);
      if (pp.kind == L2O_PROB_SIMPLE) facc += xv * xv;
      if (pp.kind == L2O_PROB_LASSO) facc += pp.l1 * __builtin_fabsf(xv);
      if (pp.kind == L2O_PROB_RASTRIGIN || pp.kind == L2O_PROB_SQUARE_COS)
        facc += pp.alpha - pp.alpha * pp.C[(size_t)b * D + j] * l2o::cos_f(pp.twopi * xv);
    }
    xs[j] = xv;
  }
  __syncthreads();

  if (pp.kind != L2O_PROB_SIMPLE) {
    const float* Wb = pp.W + (pp.w_shared ? (size_t)0 : (size_t)b * M * D);
    const float* yb = pp.y + (size_t)b * M;
    const float coef = (pp.kind == L2O_PROB_QUADRATIC || pp.kind == L2O_PROB_SQUARE_COS) ? 1.0f : 0.5f;
    if (VEC) {
      // ---- pass 1: r = W xs - y ; each wave takes 4 rows at a time -> 4 x (D/256) dwordx4 in flight
      for (int i0 = wv * 4; i0 < M; i0 += kFgWaves * 4) {
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int j = lane * 4; j < D; j += 256) {
          const float4 xv4 = *reinterpret_cast<const float4*>(xs + j);
          float4 w4[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int i = i0 + k < M ? i0 + k : M - 1;       // clamp: result of a clamped row is discarded
            w4[k] = *reinterpret_cast<const float4*>(Wb + (size_t)i * D + j);
          }
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            acc[k] = __builtin_fmaf(w4[k].x, xv4.x, acc[k]);
            acc[k] = __builtin_fmaf(w4[k].y, xv4.y, acc[k]);
            acc[k] = __builtin_fmaf(w4[k].z, xv4.z, acc[k]);
            acc[k] = __builtin_fmaf(w4[k].w, xv4.w, acc[k]);
          }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float a = wave_sum64(acc[k]);
          if (lane == 0 && i0 + k < M) {
            const float r = a - (pp.hvp ? 0.0f : yb[i0 + k]);
            rs[i0 + k] = r;
            facc += coef * r * r;
          }
        }
      }
    } else {
      for (int i = wv; i < M; i += kFgWaves) {
        const float* row = Wb + (size_t)i * D;
        float acc = 0.0f;
        for (int j = lane; j < D; j += 64) acc = __builtin_fmaf(row[j], xs[j], acc);
        acc = wave_sum64(acc);
        if (lane == 0) {
          const float r = acc - (pp.hvp ? 0.0f : yb[i]);
          rs[i] = r;
          facc += coef * r * r;
        }
      }
    }
  }
  const float fb = block_sum_fg(facc, red);   // contains a __syncthreads: rs is visible after it
  if (tid == 0) f_part[b] = fb;
  if (gout == nullptr) return;

  float* gb = gout + (size_t)b * D;
  if (pp.kind == L2O_PROB_SIMPLE) {
    for (int j = tid; j < D; j += kFgThreads) gb[j] = 2.0f * xs[j] * pp.inv_bg * (sb ? sb[j] : 1.0f);
    return;
  }
  const float* Wb = pp.W + (pp.w_shared ? (size_t)0 : (size_t)b * M * D);
  const float cg = (pp.kind == L2O_PROB_QUADRATIC || pp.kind == L2O_PROB_SQUARE_COS) ? 2.0f : 1.0f;
  auto finish = [&](int j, float s) {
    float gj = cg * s;
    const float xv = xs[j];
    if (!pp.hvp) {
      if (pp.kind == L2O_PROB_LASSO) gj += pp.l1 * (xv > 0.f ? 1.f : (xv < 0.f ? -1.f : 0.f));
      if (pp.kind == L2O_PROB_RASTRIGIN || pp.kind == L2O_PROB_SQUARE_COS)
        gj += pp.twopi * pp.alpha * pp.C[(size_t)b * D + j] * l2o::sin_f(pp.twopi * xv);
    }
    gb[j] = gj * pp.inv_bg * (sb ? sb[j] : 1.0f);
  };
  if (VEC) {
    // ---- pass 2: g = W^T r ; a thread owns 4 adjacent columns, row groups are strided over
    // RP thread groups; 4 dwordx4 loads in flight per thread
    const int ncol4 = D >> 2;
    const int CP4 = ncol4 >= kFgThreads ? kFgThreads : ((ncol4 + 63) & ~63);
    const int RP = kFgThreads / CP4;
    const int jc = tid % CP4, rp = tid / CP4;
    for (int j0 = 0; j0 < ncol4; j0 += CP4) {
      const int j4 = j0 + jc;
      float4 a = {0.f, 0.f, 0.f, 0.f};
      if (j4 < ncol4 && rp < RP) {
        const float* col = Wb + 4 * (size_t)j4;
        int i = rp;
        for (; i + 3 * RP < M; i += 4 * RP) {
          const float4 w0 = *reinterpret_cast<const float4*>(col + (size_t)i * D);
          const float4 w1 = *reinterpret_cast<const float4*>(col + (size_t)(i + RP) * D);
          const float4 w2 = *reinterpret_cast<const float4*>(col + (size_t)(i + 2 * RP) * D);
          const float4 w3 = *reinterpret_cast<const float4*>(col + (size_t)(i + 3 * RP) * D);
          const float r0 = rs[i], r1 = rs[i + RP], r2 = rs[i + 2 * RP], r3 = rs[i + 3 * RP];
          a.x += (w0.x * r0 + w1.x * r1) + (w2.x * r2 + w3.x * r3);
          a.y += (w0.y * r0 + w1.y * r1) + (w2.y * r2 + w3.y * r3);
          a.z += (w0.z * r0 + w1.z * r1) + (w2.z * r2 + w3.z * r3);
          a.w += (w0.w * r0 + w1.w * r1) + (w2.w * r2 + w3.w * r3);
        }
        for (; i < M; i += RP) {
          const float4 w0 = *reinterpret_cast<const float4*>(col + (size_t)i * D);
          const float r0 = rs[i];
          a.x = __builtin_fmaf(w0.x, r0, a.x); a.y = __builtin_fmaf(w0.y, r0, a.y);
          a.z = __builtin_fmaf(w0.z, r0, a.z); a.w = __builtin_fmaf(w0.w, r0, a.w);
        }
      }
      __syncthreads();
      *reinterpret_cast<float4*>(part + 4 * tid) = a;
      __syncthreads();
      if (rp == 0 && j4 < ncol4) {
        float4 s4 = *reinterpret_cast<const float4*>(part + 4 * jc);
        for (int p = 1; p < RP; ++p) {
          const float4 t4 = *reinterpret_cast<const float4*>(part + 4 * (p * CP4 + jc));
          s4.x += t4.x; s4.y += t4.y; s4.z += t4.z; s4.w += t4.w;
        }
        finish(4 * j4, s4.x); finish(4 * j4 + 1, s4.y); finish(4 * j4 + 2, s4.z); finish(4 * j4 + 3, s4.w);
      }
    }
  } else {
    const int CP = D >= kFgThreads ? kFgThreads : ((D + 63) & ~63);
    const int RP = kFgThreads / CP;
    const int jc = tid % CP, rp = tid / CP;
    for (int j0 = 0; j0 < D; j0 += CP) {
      const int j = j0 + jc;
      float a0 = 0.f, a1 = 0.f;
      if (j < D && rp < RP) {
        int i = rp;
        for (; i + RP < M; i += 2 * RP) {
          a0 = __builtin_fmaf(Wb[(size_t)i * D + j], rs[i], a0);
          a1 = __builtin_fmaf(Wb[(size_t)(i + RP) * D + j], rs[i + RP], a1);
        }
        for (; i < M; i += RP) a0 = __builtin_fmaf(Wb[(size_t)i * D + j], rs[i], a0);
      }
      __syncthreads();
      part[tid] = a0 + a1;
      __syncthreads();
      if (rp == 0 && j < D) {
        float s = part[jc];
        for (int p = 1; p < RP; ++p) s += part[p * CP + jc];
        finish(j, s);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// K2b: the same forward + gradient with the matrix read ONCE.  A wave keeps the rows it visits in
// registers between their two uses: lane l holds the row's columns 4 (64 v + l) .. + 3 (v < NV: coalesced
// 1 KB pieces), r_i = dot(row, xs) - y_i is a wave sum that every lane receives, and the same registers
// then feed g += r_i * row.  Eight waves walk the rows in groups of four (4 NV dwordx4 loads in flight per
// lane); their partial gradients are added in a fixed order through LDS.  Halves the HBM traffic of the
// step-granular path's matrix-bound optimizees (config 3: 256 x 512 per problem, 128 MiB per batch).
// D % 4 == 0, D <= 256 NV.
// ---------------------------------------------------------------------------
template <int NV>
__global__ __launch_bounds__(kFgThreads) void k_problem_fg1(ProbParams pp, const float* __restrict__ x,
                                                             float* __restrict__ f_part,
                                                             float* __restrict__ gout) {
  extern __shared__ float sm[];
  const int D = pp.D, M = pp.M;
  float* part = sm;                     // [kFgWaves][D] partial gradients
  float* red = part + kFgWaves * D;     // [kFgWaves]
  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const float* xb = x + (size_t)b * D;
  const float* sb = pp.x_scale ? pp.x_scale + (size_t)b * D : nullptr;
  const float* Wb = pp.W + (pp.w_shared ? (size_t)0 : (size_t)b * M * D);
  const l2o_cfp yb = (l2o_cfp)(pp.y + (size_t)b * M);
  const bool want_g = gout != nullptr;
  const float coef = (pp.kind == L2O_PROB_QUADRATIC || pp.kind == L2O_PROB_SQUARE_COS) ? 1.0f : 0.5f;

  float4 xv[NV], sv[NV], ga[NV];
  float facc = 0.0f;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int j = 4 * (64 * v + lane);
    const float4 zero = {0.f, 0.f, 0.f, 0.f}, one = {1.f, 1.f, 1.f, 1.f};
    xv[v] = zero; sv[v] = one; ga[v] = zero;
    if (j < D) {
      xv[v] = *reinterpret_cast<const float4*>(xb + j);
      if (sb) sv[v] = *reinterpret_cast<const float4*>(sb + j);
      xv[v].x *= sv[v].x; xv[v].y *= sv[v].y; xv[v].z *= sv[v].z; xv[v].w *= sv[v].w;
      if (wv == 0) {                                        // the separable terms of f: once per problem
        const float xe[4] = {xv[v].x, xv[v].y, xv[v].z, xv[v].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (pp.kind == L2O_PROB_LASSO) facc += pp.l1 * __builtin_fabsf(xe[e]);
          if (pp.kind == L2O_PROB_RASTRIGIN || pp.kind == L2O_PROB_SQUARE_COS)
            facc += pp.alpha - pp.alpha * pp.C[(size_t)b * D + j + e] * l2o::cos_f(pp.twopi * xe[e]);
        }
      }
    }
  }
  // software pipeline: the next group of four rows is requested before the current one is reduced (one wave
  // has 4 NV dwordx4 per lane in flight while it computes; without it every group pays a full memory latency)
  auto load4 = [&](int i0, float4 (&w4)[4][NV]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = i0 + k < M ? i0 + k : M - 1;             // clamped rows contribute r = 0 below
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        const int j = 4 * (64 * v + lane);
        const float4 zero = {0.f, 0.f, 0.f, 0.f};
        w4[k][v] = j < D ? *reinterpret_cast<const float4*>(Wb + (size_t)i * D + j) : zero;
      }
    }
  };
  auto use4 = [&](int i0, const float4 (&w4)[4][NV]) {
    float acc[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float a = 0.0f;
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        a = __builtin_fmaf(w4[k][v].x, xv[v].x, a);
        a = __builtin_fmaf(w4[k][v].y, xv[v].y, a);
        a = __builtin_fmaf(w4[k][v].z, xv[v].z, a);
        a = __builtin_fmaf(w4[k][v].w, xv[v].w, a);
      }
      acc[k] = a;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool ok = i0 + k < M;
      const float r = ok ? wave_sum64(acc[k]) - (pp.hvp ? 0.0f : yb[ok ? i0 + k : 0]) : 0.0f;
      if (lane == 0) facc += coef * r * r;
      if (want_g) {
#pragma unroll
        for (int v = 0; v < NV; ++v) {
          ga[v].x = __builtin_fmaf(r, w4[k][v].x, ga[v].x);
          ga[v].y = __builtin_fmaf(r, w4[k][v].y, ga[v].y);
          ga[v].z = __builtin_fmaf(r, w4[k][v].z, ga[v].z);
          ga[v].w = __builtin_fmaf(r, w4[k][v].w, ga[v].w);
        }
      }
    }
  };
  {
    constexpr int STEP = kFgWaves * 4;
    float4 wa[4][NV], wb[4][NV];
    int i0 = wv * 4;
    if (i0 < M) load4(i0, wa);
    for (; i0 < M; i0 += 2 * STEP) {
      if (i0 + STEP < M) load4(i0 + STEP, wb);
      use4(i0, wa);
      if (i0 + STEP < M) {
        if (i0 + 2 * STEP < M) load4(i0 + 2 * STEP, wa);
        use4(i0 + STEP, wb);
      }
    }
  }
  if (want_g) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int j = 4 * (64 * v + lane);
      if (j < D) *reinterpret_cast<float4*>(part + wv * D + j) = ga[v];
    }
  }
  const float fb = block_sum_fg(facc, red);   // contains __syncthreads: the partial gradients are visible after it
  if (tid == 0) f_part[b] = fb;
  if (!want_g) return;
  float* gb = gout + (size_t)b * D;
  const float cg = (pp.kind == L2O_PROB_QUADRATIC || pp.kind == L2O_PROB_SQUARE_COS) ? 2.0f : 1.0f;
  for (int j = tid; j < D; j += kFgThreads) {
    float s = part[j];
#pragma unroll
    for (int w = 1; w < kFgWaves; ++w) s += part[w * D + j];
    const float sc = sb ? sb[j] : 1.0f;
    const float xj = xb[j] * sc;
    float gj = cg * s;
    if (!pp.hvp) {
      if (pp.kind == L2O_PROB_LASSO) gj += pp.l1 * (xj > 0.f ? 1.f : (xj < 0.f ? -1.f : 0.f));
      if (pp.kind == L2O_PROB_RASTRIGIN || pp.kind == L2O_PROB_SQUARE_COS)
        gj += pp.twopi * pp.alpha * pp.C[(size_t)b * D + j] * l2o::sin_f(pp.twopi * xj);
    }
    gb[j] = gj * pp.inv_bg * sc;
  }
}

extern "C" {   // (the kernel keeps its unmangled name)
// out += s * inv_bg * f''(x s) * s * u for the separable cosine term (rastrigin / square_cos)
__global__ void k_hvp_sep(ProbParams pp, const float* __restrict__ x, const float* __restrict__ u, float* __restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float sc = pp.x_scale ? pp.x_scale[i] : 1.0f;
  const float xs = x[i] * sc;
  out[i] += sc * pp.inv_bg * (pp.twopi * pp.twopi * pp.alpha * pp.C[i] * l2o::cos_f(pp.twopi * xs)) * sc * u[i];
}
}
