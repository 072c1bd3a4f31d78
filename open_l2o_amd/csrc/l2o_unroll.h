// l2o_unroll.h -- k_unroll, the fused persistent unroll with one workgroup per problem.
#pragma once
#include "l2o_lstm_bx3.h"
#include "l2o_params.h"

// ---------------------------------------------------------------------------
// K3: the fused persistent unroll.  One workgroup per problem, one wave per
// 16-coordinate tile (<= 8 waves), T steps in ONE launch.
//   LDS  : the problem matrix TWICE -- W_b row-major and W_b^T row-major, row stride
//          S = SQ + 16 floats (S/4 == 4 or 12 mod 16 -> ds_read_b128 of a (row, 16-byte
//          column chunk) per lane is bank-conflict free) -- plus y, x*s and the residual r
//   VGPR : optimizer weights (MFMA A fragments), LSTM state, x, m, v
//   HBM  : W_b read once per launch; x/state/m/v read+written once; one float per
//          (step, problem)
// Per step and wave (lane l also plays the GEMV role (row = 16*wave + l/4, chunk = l%4)):
//   xs <- x*s ; barrier
//   r  = W xs - y           || the 25 layer-2 MFMAs fed by the previous h2
//   f_b partial ; barrier
//   g  = W^T r (own 16 coordinates) || the 25 layer-1 MFMAs fed by the previous h1
//   preprocess(g) -> input MFMAs -> gates -> layer-2 MFMAs -> gates -> Linear -> x += delta
// i.e. 50 of the 80 MFMAs of a step depend only on the previous step's state and are
// issued interleaved with the GEMV's LDS reads and FMAs (separate pipes).
// ---------------------------------------------------------------------------
#ifdef L2O_ABLATE_BARRIER
#define L2O_SYNC() ((void)0)
#else
#define L2O_SYNC() __syncthreads()
#endif
template <int PRE, int KIND, int CH, bool HIST, bool EXACT = false>
__global__ __launch_bounds__(CH <= 4 ? 256 : 512) void k_unroll(UnrollArgs a) {
  // CH <= 4 <=> at most 4 waves per workgroup = one wave per SIMD: the bf16x3 gate GEMM with
  // its weights in VGPR + AGPR; CH == 8 (5..8 waves) keeps the fp32 MFMA form (as does EXACT: L2O_OPT_EXACT_GATES)
  using Core = LstmCore<PRE, (CH <= 4) && !EXACT>;
  constexpr int SQ = 16 * CH;      // padded square size of the LDS-resident matrix
  constexpr int S = SQ + 16;       // row stride (floats)
  extern __shared__ float sm[];
  const ProbParams& pp = a.pp;
  const int D = pp.D, M = pp.M;
  float* Ws = sm;                  // [SQ][S]  W   (rows i, columns j)
  float* WTs = Ws + SQ * S;        // [SQ][S]  W^T (rows j, columns i)
  float* xs = WTs + SQ * S;        // [SQ]
  float* rs = xs + SQ;             // [SQ]
  float* ys = rs + SQ;             // [SQ]
  float* fpart = ys + SQ;          // [8]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nw = blockDim.x >> 6;
  const int c = lane & 15, q = lane >> 4;      // LSTM role: coordinate c, unit group q
  const int grow = wv * kTile + (lane >> 2);   // GEMV role: matrix row (r pass) / coordinate (g pass)
  const int gq = lane & 3;                     //            16-byte column chunk inside a 64-byte group
  const int b = blockIdx.x;

  // ---- stage the problem into LDS (zero padded), both orientations ---------
  const float* Wb = pp.W + (pp.w_shared ? (size_t)0 : (size_t)b * M * D);
  for (int i = tid; i < 2 * SQ * S + 3 * SQ; i += blockDim.x) sm[i] = 0.0f;
  __syncthreads();
  for (int e = tid; e < M * D; e += blockDim.x) {
    const int i = e / D, j = e - i * D;
    const float v = Wb[e];
    Ws[i * S + j] = v;
    WTs[j * S + i] = v;
  }
  for (int i = tid; i < M; i += blockDim.x) ys[i] = pp.y[(size_t)b * M + i];

  // ---- per-lane persistent registers -------------------------------------
  Core core;
  core.load(a.np.wpack, lane);
  core.pin();   // (bf16x3 forms: fragments -> AGPRs; without it 125-133 v_accvgpr_read per step)
  __shared__ __attribute__((aligned(16))) float bias_s[Core::kBiasFloats];   // the gate biases = accumulator inits
  core.stage_bias(bias_s, a.np.wpack, tid, blockDim.x, q);
  const int j = wv * kTile + c;             // this lane's coordinate (LSTM role)
  const bool live = j < D;
  const size_t idx = (size_t)b * D + j;
  const int tile = b * nw + wv;
  TileState s;
  float* st_tile = a.st + (size_t)tile * kStateFloatsPerTile;
  if (a.zero_state) {
#pragma unroll
    for (int t5 = 0; t5 < kNT; ++t5) s.h1[t5] = s.c1[t5] = s.h2[t5] = s.c2[t5] = 0.0f;
  } else {
    load_tile_state(s, st_tile, lane);
  }
  float xv = live ? (a.x_in ? a.x_in : a.x)[idx] : 0.0f;
  const float sc = (live && pp.x_scale) ? pp.x_scale[idx] : 1.0f;
  float cj = 0.0f;
  constexpr bool kCos = KIND == L2O_PROB_RASTRIGIN || KIND == L2O_PROB_SQUARE_COS;
  if (kCos) cj = live ? pp.C[idx] : 0.0f;
  float mv = 0.0f, vv = 0.0f;
  if (PRE == L2O_PRE_FC_ELU && !a.zero_state) { mv = live ? a.m[idx] : 0.0f; vv = live ? a.v[idx] : 0.0f; }
  float p1h = a.p1_hi, p1l = a.p1_lo, p2h = a.p2_hi, p2l = a.p2_lo;
  constexpr bool kSq = KIND == L2O_PROB_QUADRATIC || KIND == L2O_PROB_SQUARE_COS;
  const float coef = kSq ? 1.0f : 0.5f;
  const float cg = (KIND == L2O_PROB_QUADRATIC ? 2.0f : 1.0f) * pp.inv_bg;   // x2 folded in (exact)
  const float kTwoPi = pp.twopi;
  const float* wrow = Ws + grow * S + 4 * gq;
  const float* wtrow = WTs + grow * S + 4 * gq;
  const float* xsq = xs + 4 * gq;
  const float* rsq = rs + 4 * gq;
  const int perm_src = (4 * c) << 2;        // byte index of lane 4*c for ds_bpermute

  // software pipeline of the matrix work: acc1 always holds bias + (h1 of the previous step)
  // part of layer 1; it is produced at the END of the previous step (overlapping that step's
  // layer-2 gate math), here for step 0.
  f32x4 acc1[kNT], acc2[kNT];
  core.init(s, q);
  __syncthreads();                                           // the bias table is staged
  core.preload(acc1, acc2);
  core.template issue_l1_prev<0, Core::kTotal>(s, acc1);

  const size_t hist_n = (size_t)pp.B_local * D;
  for (int t = 0;; ++t) {
    const float xsv = xv * sc;
    if (live && q == 0) xs[j] = xsv;
    if (HIST && t < a.T)
      store_tile_state(s, a.hist_st + ((size_t)t * pp.B_local * nw + tile) * kStateFloatsPerTile, lane);
    L2O_SYNC();                                             // B1: xs complete
    // ---- r = W xs - y  ||  first 12 layer-2 MFMAs of the previous h2 -----------
    float4 racc = {0.f, 0.f, 0.f, 0.f};
    static_for<0, CH>([&](auto mc) {
      constexpr int m = decltype(mc)::value;
      const float4 wv4 = *reinterpret_cast<const float4*>(wrow + 16 * m);
      const float4 xv4 = *reinterpret_cast<const float4*>(xsq + 16 * m);
      core.template issue_l2_prev<(Core::kHalf * m) / CH, (Core::kHalf * (m + 1)) / CH>(s, acc2);
      dot4(wv4, xv4, racc);
    });
    const float r = quad_sum(hsum4(racc)) - ys[grow];
    float contrib = 0.0f;
    if (gq == 0) {
      rs[grow] = r;                       // rows >= M: W row and y are zero -> r == 0
      contrib = coef * r * r;
    }
    if (live && q == 0) {
      if (KIND == L2O_PROB_LASSO) contrib += pp.l1 * __builtin_fabsf(xsv);
      if (kCos) contrib += pp.alpha - pp.alpha * cj * l2o::cos_f(kTwoPi * xsv);
    }
    contrib = wave_sum64(contrib);
    if (lane == 0) fpart[wv] = contrib;
    L2O_SYNC();                                             // B2: rs, fpart complete
    if (tid == 0) {
      float f = fpart[0];
      for (int k = 1; k < nw; ++k) f += fpart[k];
      a.fx_part[(size_t)t * pp.B_local + b] = f;
    }
    if (t == a.T && !HIST) break;

    // ---- g = W^T r for this wave's 16 coordinates  ||  the other 13 of those MFMAs ----
    float4 gacc4 = {0.f, 0.f, 0.f, 0.f};
    static_for<0, CH>([&](auto mc) {
      constexpr int m = decltype(mc)::value;
      const float4 wt4 = *reinterpret_cast<const float4*>(wtrow + 16 * m);
      const float4 rv4 = *reinterpret_cast<const float4*>(rsq + 16 * m);
      core.template issue_l2_prev<Core::kHalf + ((Core::kTotal - Core::kHalf) * m) / CH,
                                  Core::kHalf + ((Core::kTotal - Core::kHalf) * (m + 1)) / CH>(s, acc2);
      dot4(wt4, rv4, gacc4);
    });
    const float gacc = quad_sum(hsum4(gacc4));                 // lanes 4k..4k+3 hold g of coordinate 16*wv + k
    float gv = __int_as_float(__builtin_amdgcn_ds_bpermute(perm_src, __float_as_int(gacc)));
    if (KIND == L2O_PROB_SQUARE_COS) gv *= 2.0f;            // only the ||wx-y||^2 part carries the 2
    if (KIND == L2O_PROB_LASSO) gv += pp.l1 * (xsv > 0.f ? 1.f : (xsv < 0.f ? -1.f : 0.f));
    if (kCos) gv += kTwoPi * pp.alpha * cj * l2o::sin_f(kTwoPi * xsv);
    gv = live ? gv * cg * sc : 0.0f;
    if (HIST && live && q == 0) {
      if (t < a.T) a.hist_g[(size_t)t * hist_n + idx] = gv;
      else a.hist_gfinal[idx] = gv;
    }
    if (HIST && t == a.T) break;                            // (history mode: the gradient at x_T was still needed)

    // ---- optimizer network ----------------------------------------------------
    float in0, in1;
    if (PRE == L2O_PRE_FC_ELU) {
      // beta^k as a float-float running product (k = step0 + t)
      rnnprop_inputs(gv, mv, vv, a.np.beta1, a.np.beta2, a.np.omb1, a.np.omb2, 1.0f - p1h, 1.0f - p2h, in0, in1);
      if (HIST && live && q == 0) { a.hist_m[(size_t)t * hist_n + idx] = mv; a.hist_v[(size_t)t * hist_n + idx] = vv; }
      if (!live) { in0 = 0.0f; in1 = 0.0f; }
      {
        float hi = p1h * a.np.beta1, er = __builtin_fmaf(p1h, a.np.beta1, -hi);
        float lo = __builtin_fmaf(p1l, a.np.beta1, er), sum = hi + lo;
        p1l = lo - (sum - hi); p1h = sum;
        hi = p2h * a.np.beta2; er = __builtin_fmaf(p2h, a.np.beta2, -hi);
        lo = __builtin_fmaf(p2l, a.np.beta2, er); sum = hi + lo;
        p2l = lo - (sum - hi); p2h = sum;
      }
    } else {
      preprocess_grad<PRE>(gv, a.np.k_inv_ln2, a.np.exp_k, in0, in1);
    }
    PhaseClock pc;
    float d = core.template finish<true>(s, acc1, acc2, in0, in1, q, pc);
    if (a.np.tanh_output) d = tanhf_(d);
    xv = __builtin_fmaf(d, a.np.scale, xv);
  }

  if (live && q == 0) {
    a.x[idx] = xv;
    if (PRE == L2O_PRE_FC_ELU) { a.m[idx] = mv; a.v[idx] = vv; }
  }
  store_tile_state(s, st_tile, lane);
}
