// l2o_unroll.hip -- the quadratic-family optimizees of the C ABI of include/l2o_abi.h: their loss / gradient / Hessian-vector
// product (l2o_problem_fg, l2o_problem_hvp), the step-granular optimizer step (l2o_cwlstm_step*) and the fused persistent
// unrolls (l2o_unroll*) with their workspace and the co-residency probe.  This unit owns the kernels of l2o_problem_fg.h and
// every k_unroll* / k_cwlstm_step instantiation except the ones l2o_ilp_kernels.h lists.
//
// Reference semantics (file:line under /root/reference/Model_Free_L2O/
// "L2O-DM and L2O-RNNProp"/, shorthand DM/):
//   unroll loop        DM/meta.py:319-389, DM/meta_rnnprop_eval.py (time_step/update)
//   optimizer nets     DM/networks.py:157-300
//   preprocess         DM/preprocess.py:26-70
//   optimizees         DM/problems.py:41-213
// Written for gfx950 only: wave64, v_mfma_f32_16x16x4_f32, 160 KiB LDS per CU.
#include "l2o_host.h"
#include "l2o_step.h"
#include "l2o_problem_fg.h"
#include "l2o_unroll.h"
#include "l2o_unroll_pair.h"
#include "l2o_unroll_lds.h"
#include "l2o_unroll_cu.h"
#include "l2o_unroll_cu8.h"
#include "l2o_ilp_kernels.h"   // the plain two-CU / eight-wave unrolls: code in l2o_kernels_ilp.hip, `extern template` here

// the two kernels of l2o_util_kernels.h that this unit launches: code in l2o_core.hip, the launch binds to its host stub
__global__ void k_combine_halves(const float* __restrict__ fx_half, float* __restrict__ fx_part, int nb, int nparts,
                                 float inv_bg, float* __restrict__ fx, unsigned long long* __restrict__ xbuf, long xwords,
                                 PairWs* ws, int b0, int B_local);
__global__ void k_coresident_probe(unsigned* ctr, unsigned* min_seen);

static int check_problem(const l2o_problem* p) {
  if (!p) return fail(L2O_ERR_ARG, "problem is NULL");
  if (p->B_local <= 0 || p->B_global < p->B_local || p->D <= 0)
    return fail(L2O_ERR_ARG, "bad problem sizes B_local=%d B_global=%d D=%d", p->B_local, p->B_global, p->D);
  switch (p->kind) {
    case L2O_PROB_SIMPLE: return L2O_OK;
    case L2O_PROB_QUADRATIC:
    case L2O_PROB_LASSO:
      if (!p->W || !p->y || p->M <= 0) return fail(L2O_ERR_ARG, "problem needs W, y and M > 0");
      if (p->kind == L2O_PROB_QUADRATIC && p->M != p->D) return fail(L2O_ERR_ARG, "quadratic needs M == D");
      return L2O_OK;
    case L2O_PROB_RASTRIGIN:
    case L2O_PROB_SQUARE_COS:
      if (!p->W || !p->y || !p->C || p->M != p->D)
        return fail(L2O_ERR_ARG, "rastrigin / square_cos need W, y, C and M == D");
      return L2O_OK;
    default: return fail(L2O_ERR_UNSUPPORTED, "problem kind %d has no HIP kernel", p->kind);
  }
}

struct UnrollGeom { int CH, nw; size_t lds; };
static bool unroll_geom(const l2o_problem* p, UnrollGeom* g) {
  const int D = p->D, M = p->M;
  g->nw = tiles_per_problem(D);
  if (g->nw > 8 || M > 16 * g->nw) return false;     // rows are covered by the nw waves, 16 each
  const int need = g->nw;                            // 16-float chunks per matrix row
  g->CH = need <= 1 ? 1 : (need <= 2 ? 2 : (need <= 4 ? 4 : 8));
  const int SQ = 16 * g->CH, S = SQ + 16;
  g->lds = sizeof(float) * (2 * (size_t)SQ * S + 3 * (size_t)SQ + 8);
  return g->lds <= 160 * 1024;
}

// Split every problem over two workgroups when that still leaves all of them co-resident.
// Problems per launch of the two-CU form, 0 = not this form.  Every problem of a launch must be co-resident with its
// partner: at most #CU / 2 per launch.  A larger batch shard runs as consecutive launches of equal chunks (a multiple
// of the 8-problem launch groups) -- normal-matrix kernel only; a chunk launch with every tile on its own SIMD beats
// one round of the one-CU form (config 4, 1024 problems on one GPU: 5.3 -> 6.0 G coordinate-steps/s).
static int pair_chunk(const l2o_problem* p, const UnrollGeom& g, hipStream_t s) {
  if (!opt(L2O_OPT_PAIR) || g.CH < 2) return 0;
  const int cap = coresident_cus(s) / 2;
  if (p->B_local <= cap) return p->B_local;
  if (cap < 8) return 0;
  const int n = (p->B_local + cap - 1) / cap;               // launches
  const int chunk = (((p->B_local + n - 1) / n) + 7) & ~7;  // balanced, whole launch groups
  return chunk <= cap ? chunk : (cap & ~7);
}
struct PairLayout { size_t xbuf_off, xbuf_bytes, fxh_off, total; int npg; size_t lds; };
static PairLayout pair_layout(const l2o_problem* p, const UnrollGeom& g, int T) {
  PairLayout L;
  const int SQ = 16 * g.CH;
  L.npg = SQ;                         // granules per (half, parity): one per residual row
  L.xbuf_off = sizeof(PairWs);
  L.xbuf_bytes = (size_t)p->B_local * 2 * 2 * L.npg * sizeof(unsigned long long);
  L.fxh_off = L.xbuf_off + L.xbuf_bytes;
  L.total = L.fxh_off + sizeof(float) * (size_t)(T + 1) * g.CH * p->B_local;   // one partial per (step, problem, wave)
  L.lds = 0;                          // static LDS only (xs, rs, fpart)
  return L;
}

template <int PRE, int KIND>
static int launch_unroll_ch(const UnrollArgs& a, const UnrollGeom& g, hipStream_t s, const l2o_problem* prob,
                            void* workspace, float* fx, bool* fx_done) {
  const bool hist = a.hist_st != nullptr;
  int chunk = workspace ? pair_chunk(prob, g, s) : 0;
  // Large shards (round 4) -- more problems than the #CU / 2 one launch of the two-CU kernel holds -- run k_unroll_lds: one
  // problem per CU, the gate-GEMM fragments in LDS, two waves of the SAME problem per SIMD, one launch, no cross-CU
  // protocol.  L2O_OPT_ONE_LDS: 0 = consecutive chunk launches of the two-CU kernel instead (rounds 2-3; A/B runs), 1 = the
  // default, 2 = k_unroll_lds for every shard (A/B runs).  5..8 tiles, no exact-gates request.  Also the exchange-free
  // fallback of those shapes when the two-CU form is not available (no workspace, L2O_OPT_PAIR = 0; the host's recovery
  // from a partner timeout): the alternative there is k_unroll's fp32-MFMA form, 11 200 cycles per step against 7 200.
  // (k_unroll_pair2 -- the two-CU kernel with fragments in LDS, two workgroups per CU -- measured the same as k_unroll_lds
  //  in round 4 and was removed in round 5: docs/DESIGN_history_r04.md.)
  {
    const int one_lds = (int)opt(L2O_OPT_ONE_LDS);
#ifdef L2O_LDS_ABL_ANYNW   // (timing ablation: also 1..4 tiles, i.e. ONE wave per SIMD in this kernel; needs M <= 16 nw)
    const bool shape_ok = g.nw >= 1 && a.pp.M <= 16 * g.nw;
#else
    const bool shape_ok = g.CH == 8 && g.nw >= 5;
#endif
    const bool plain = !(opt(L2O_OPT_EXACT_GATES) && !hist);
    if ((one_lds == 2 || (one_lds == 1 && (chunk == 0 || a.pp.B_local > chunk))) && shape_ok && plain) {
      UnrollArgs al = a;
      al.ticks = workspace ? &reinterpret_cast<PairWs*>(workspace)->ticks : nullptr;
      void (*fl)(UnrollArgs) = hist ? k_unroll_lds<PRE, KIND, true> : k_unroll_lds<PRE, KIND, false>;
      const size_t lds = sizeof(float) * ((size_t)LstmCoreLds<PRE>::kFragWords + 2 * 128 + 8);
      const int rc = launch(fl, dim3(a.pp.B_local), dim3(64 * g.nw), lds, s, al);
      if (rc) return rc;
      note_form(L2O_FORM_UNROLL_LDS);
      note_variant(0, hist, false, false, 0, 0);
      return L2O_OK;
    }
  }
  if (chunk > 0) {
    const PairLayout L = pair_layout(prob, g, a.T);
    UnrollPairArgs pa;
    pa.u = a;
    pa.ws = reinterpret_cast<PairWs*>(workspace);
    pa.xbuf = reinterpret_cast<unsigned long long*>(static_cast<char*>(workspace) + L.xbuf_off);
    pa.fx_half = reinterpret_cast<float*>(static_cast<char*>(workspace) + L.fxh_off);
    // (the per-launch salt of the granule tags is the device-side sequence word ws->seq, which
    //  k_combine_halves advances after every launch: no host-side launch state)
    pa.use_salt = a.T + 1 < 0xffff ? 1u : 0u;
    pa.plain_stores = opt(L2O_OPT_PAIR_PLAIN_STORES) ? 1u : 0u;
    pa.b0 = 0;
    pa.nb = a.pp.B_local;
    // (no memset here: the workspace starts zeroed -- l2o_unroll_workspace_init -- and the epilogue kernel of every
    //  launch leaves the granule area zeroed for the next one)
    // grid: groups of 16 blocks = 8 problems x 2 halves (partners are b and b + 8)
    const int B = a.pp.B_local;
    const bool one_launch = chunk >= B;
    const bool exact = opt(L2O_OPT_EXACT_GATES) != 0 && !hist;   // (the recording unroll keeps the bf16x3 core)
    bool fast_launched = false;
    {
      void (*fn)(UnrollPairArgs) = nullptr;
      const size_t dyn_lds = L.lds;
      // full tiles (M = D = padded size) run the FAST prologue, everything else -- and L2O_OPT_PAIR_FAST_LOAD = 0 -- the gather
      const int SQ = 16 * g.CH;
      const bool fast = opt(L2O_OPT_PAIR_FAST_LOAD) != 0 && a.pp.M == SQ && a.pp.D == SQ;
      pa.fast_load = fast ? 1u : 0u;
      fast_launched = fast;
#define L2O_PAIR_FN(C)                                                                                       \
  (fast ? (hist ? k_unroll_pair<PRE, KIND, C, true, false, true>                                             \
                : (exact ? k_unroll_pair<PRE, KIND, C, false, true, true> : k_unroll_pair<PRE, KIND, C, false, false, true>)) \
        : (hist ? k_unroll_pair<PRE, KIND, C, true> : (exact ? k_unroll_pair<PRE, KIND, C, false, true> : k_unroll_pair<PRE, KIND, C, false>)))
      switch (g.CH) {
        case 2: fn = L2O_PAIR_FN(2); break;
        case 4: fn = L2O_PAIR_FN(4); break;
        default: fn = L2O_PAIR_FN(8); break;
      }
#undef L2O_PAIR_FN
      for (int b0 = 0; b0 < B; b0 += chunk) {
        pa.b0 = b0;
        pa.nb = B - b0 < chunk ? B - b0 : chunk;
        hipLaunchKernelGGL(fn, dim3((pa.nb + 7) / 8 * 16), dim3(64 * (g.CH / 2)), dyn_lds, s, pa);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_combine_halves, dim3(a.T + 1), dim3(256), 0, s, pa.fx_half, a.fx_part, pa.nb, g.CH,
                           a.pp.inv_bg, one_launch ? fx : nullptr, pa.xbuf, (long)pa.nb * 2 * 2 * L.npg, pa.ws, b0, B);
        HIP_TRY(hipGetLastError());
      }
    }
    note_form(L2O_FORM_UNROLL_PAIR, (B + chunk - 1) / chunk);
    note_variant(g.CH, hist, exact, fast_launched, 0, 0);
    if (fx_done) *fx_done = fx != nullptr && one_launch;
    return L2O_OK;
  }
  void (*fn)(UnrollArgs) = nullptr;
  const bool exact1 = opt(L2O_OPT_EXACT_GATES) != 0 && !hist;
  switch (g.CH) {
    case 1: fn = hist ? k_unroll<PRE, KIND, 1, true> : (exact1 ? k_unroll<PRE, KIND, 1, false, true> : k_unroll<PRE, KIND, 1, false>); break;
    case 2: fn = hist ? k_unroll<PRE, KIND, 2, true> : (exact1 ? k_unroll<PRE, KIND, 2, false, true> : k_unroll<PRE, KIND, 2, false>); break;
    case 4: fn = hist ? k_unroll<PRE, KIND, 4, true> : (exact1 ? k_unroll<PRE, KIND, 4, false, true> : k_unroll<PRE, KIND, 4, false>); break;
    default: fn = hist ? k_unroll<PRE, KIND, 8, true> : k_unroll<PRE, KIND, 8, false>; break;
  }
  const int rc = launch(fn, dim3(a.pp.B_local), dim3(64 * g.nw), g.lds, s, a);
  if (rc) return rc;
  note_form(L2O_FORM_UNROLL);
  note_variant(g.CH, hist, exact1 && g.CH <= 4, false, 0, 0);     // (CH == 8 has no EXACT instantiation: fp32 MFMA always)
  return L2O_OK;
}

template <int PRE>
static int launch_unroll_kind(const UnrollArgs& a, const UnrollGeom& g, int kind, hipStream_t s,
                              const l2o_problem* prob, void* workspace, float* fx, bool* fx_done) {
  switch (kind) {
    case L2O_PROB_QUADRATIC: return launch_unroll_ch<PRE, L2O_PROB_QUADRATIC>(a, g, s, prob, workspace, fx, fx_done);
    case L2O_PROB_LASSO: return launch_unroll_ch<PRE, L2O_PROB_LASSO>(a, g, s, prob, workspace, fx, fx_done);
    case L2O_PROB_RASTRIGIN: return launch_unroll_ch<PRE, L2O_PROB_RASTRIGIN>(a, g, s, prob, workspace, fx, fx_done);
    case L2O_PROB_SQUARE_COS: return launch_unroll_ch<PRE, L2O_PROB_SQUARE_COS>(a, g, s, prob, workspace, fx, fx_done);
    default: return fail(L2O_ERR_UNSUPPORTED, "no fused kernel for problem kind %d", kind);
  }
}

// The streaming form (csrc/l2o_unroll_cu.h) takes the sizes the LDS-resident kernels cannot: one
// workgroup per problem, matrix streamed once per step, LSTM state in LDS (+ registers).
static bool unroll_cu_eligible(const l2o_problem* p) {
  if (!opt(L2O_OPT_UNROLL_CU)) return false;
  if (p->D < 4 || p->D > 512 || (p->D & 3) || p->M <= 0) return false;   // (D <= 128: only when the rows do not fit the LDS forms)
  return unroll_cu_layout(p->D).lds + sizeof(float) * bx::kBiasWords <= 160 * 1024;   // (+ the static bias table)
}
// L2O_OPT_UNROLL_CU: 0 step-granular path, 1* the eight-wave form (k_unroll_cu8: two waves per SIMD, fragments in LDS, LSTM
// state in registers) for RNNProp's plain unroll and the four-wave form (k_unroll_cu) otherwise, 2 k_unroll_cu always,
// 3 k_unroll_cu8 always, 4 k_unroll_cu8 with three register tiles + one LDS slot per wave (A/B runs)
template <int PRE, int KR>
static int launch_unroll_cu8(const UnrollArgs& a, hipStream_t s) {
  const UnrollCu8Layout L = unroll_cu8_layout(a.pp.D, PRE, KR);
  const bool hist = a.hist_st != nullptr;
  void (*fn)(UnrollArgs) = a.pp.D <= 256 ? (hist ? k_unroll_cu8<PRE, 1, KR, true> : k_unroll_cu8<PRE, 1, KR, false>)
                                         : (hist ? k_unroll_cu8<PRE, 2, KR, true> : k_unroll_cu8<PRE, 2, KR, false>);
  note_form(L2O_FORM_UNROLL_CU8);
  note_variant(0, hist, false, false, KR, a.pp.D <= 256 ? 1 : 2);
  return launch(fn, dim3(a.pp.B_local), dim3(kCu8Threads), L.lds, s, a);
}
template <int PRE>
static int launch_unroll_cu(const UnrollArgs& a_in, hipStream_t s) {
  const int form = (int)opt(L2O_OPT_UNROLL_CU);
  // Default (1): the eight-wave form (k_unroll_cu8) with the number of register-resident state tiles per wave (KR) that the
  // instantiation holds without spilling at 256 registers (scripts/tu_regs.sh; D = 512): RNNProp's plain unroll 4 (config 3:
  // 3 spilled registers, measured best), the DM nets' plain unroll 3 (round 5: their input-weight rows moved to LDS; 0
  // spills -- with 4: 31-37; measured on DM / Lasso 256 x 512, batch 256: 5.25 G four-wave, 5.26 G KR = 4, 6.24 G KR = 3),
  // every recording unroll 2 (0 / 10 spills) where that LDS image fits (two more 5 KB state slots per wave: D <= 256), the
  // DM nets' recording unroll at larger D 3 (8 spills); RNNProp's recording unroll at D > 256 stays on the four-wave kernel
  // (KR = 3: 52 spills).  2: k_unroll_cu always; 3 / 4 / 5: k_unroll_cu8 always with KR = 4 / 3 / 2 where it fits (A/B runs).
  const bool hist0 = a_in.hist_st != nullptr;
  auto fits = [&](int kr) { return unroll_cu8_layout(a_in.pp.D, PRE, kr).lds + sizeof(float) * bx::kBiasWords <= 160 * 1024; };
  int KR = 0;
  if (form == 1) {
    KR = hist0 ? 2 : (PRE == L2O_PRE_FC_ELU ? 4 : 3);
    if (hist0 && !fits(2) && PRE != L2O_PRE_FC_ELU) KR = 3;
  } else if (form >= 3 && form <= 5) KR = 7 - form;
  if (KR && fits(KR))
    return KR == 4 ? launch_unroll_cu8<PRE, 4>(a_in, s) : (KR == 3 ? launch_unroll_cu8<PRE, 3>(a_in, s) : launch_unroll_cu8<PRE, 2>(a_in, s));
  const UnrollCuLayout L = unroll_cu_layout(a_in.pp.D);
  const UnrollArgs& a = a_in;
  const bool hist = a.hist_st != nullptr;
  void (*fn)(UnrollArgs) = a.pp.D <= 256 ? (hist ? k_unroll_cu<PRE, 1, true> : k_unroll_cu<PRE, 1, false>)
                                         : (hist ? k_unroll_cu<PRE, 2, true> : k_unroll_cu<PRE, 2, false>);
  note_form(L2O_FORM_UNROLL_CU);
  note_variant(0, hist, false, false, 0, a.pp.D <= 256 ? 1 : 2);
  return launch(fn, dim3(a.pp.B_local), dim3(kCuThreads), L.lds, s, a);
}

extern "C" {

static int launch_problem_fg(const ProbParams& pp, const float* x, float* f_part, float* g, void* stream) {
  const size_t lds = sizeof(float) * ((size_t)((pp.D + 3) & ~3) + ((pp.M + 3) & ~3) + 4 * kFgThreads + kFgWaves);
  if (lds > 160 * 1024) return fail(L2O_ERR_UNSUPPORTED, "problem too large for k_problem_fg (D=%d M=%d)", pp.D, pp.M);
  const bool vec = pp.kind != L2O_PROB_SIMPLE && (pp.D & 3) == 0 && ((uintptr_t)pp.W & 15) == 0;
  if (vec && pp.D >= 64 && pp.D <= 2048 && ((uintptr_t)x & 15) == 0 && (!pp.x_scale || ((uintptr_t)pp.x_scale & 15) == 0) &&
      !pp.w_shared && !opt(L2O_OPT_FG_TWO_PASS)) {         // single pass over the matrix (a shared, L2-resident
                                                            // matrix is faster in two passes: 20 vs 28 us for config 3)
    const size_t lds1 = sizeof(float) * ((size_t)kFgWaves * pp.D + kFgWaves);
    void (*f1)(ProbParams, const float*, float*, float*) =
        pp.D <= 256 ? k_problem_fg1<1> : pp.D <= 512 ? k_problem_fg1<2> : pp.D <= 1024 ? k_problem_fg1<4> : k_problem_fg1<8>;
    return launch(f1, dim3(pp.B_local), dim3(kFgThreads), lds1, (hipStream_t)stream, pp, x, f_part, g);
  }
  void (*fn)(ProbParams, const float*, float*, float*) = vec ? k_problem_fg<true> : k_problem_fg<false>;
  return launch(fn, dim3(pp.B_local), dim3(kFgThreads), lds, (hipStream_t)stream, pp, x, f_part, g);
}

int l2o_problem_fg(const l2o_problem* prob, const float* x, float* f_part, float* g, void* stream) {
  OptScope opt_scope((prob && (prob->flags & L2O_PROB_FG_TWO_PASS)) ? L2O_OPTW(L2O_OPT_FG_TWO_PASS, 1) : 0);
  int rc = check_problem(prob);
  if (rc) return rc;
  if (!x || !f_part) return fail(L2O_ERR_ARG, "l2o_problem_fg: NULL x / f_part");
  return launch_problem_fg(make_prob_params(prob), x, f_part, g, stream);
}

int l2o_problem_hvp(const l2o_problem* prob, const float* x, const float* u, float* out, float* scratch, void* stream) {
  OptScope opt_scope((prob && (prob->flags & L2O_PROB_FG_TWO_PASS)) ? L2O_OPTW(L2O_OPT_FG_TWO_PASS, 1) : 0);
  int rc = check_problem(prob);
  if (rc) return rc;
  if (!x || !u || !out || !scratch) return fail(L2O_ERR_ARG, "l2o_problem_hvp: NULL argument");
  ProbParams pp = make_prob_params(prob);
  pp.hvp = 1;
  rc = launch_problem_fg(pp, u, scratch, out, stream);     // cg s inv_bg W^T (W (s u))  (simple: 2 s^2 u)
  if (rc) return rc;
  if (pp.kind == L2O_PROB_RASTRIGIN || pp.kind == L2O_PROB_SQUARE_COS) {
    const size_t n = (size_t)pp.B_local * pp.D;
    hipLaunchKernelGGL(k_hvp_sep, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, pp, x, u, out, n);
    HIP_TRY(hipGetLastError());
  }
  return L2O_OK;
}

int l2o_cwlstm_step_multi(const l2o_net_cfg* cfg, const float* wpack, const l2o_step_seg* segs, int32_t nseg,
                          double pow1, double pow2, void* stream) {
  OptScope opt_scope(cfg_optw(cfg));
  if (!cfg || !wpack || !segs || nseg < 1) return fail(L2O_ERR_ARG, "l2o_cwlstm_step: bad argument");
  if (nseg > kMaxStepSegs) return fail(L2O_ERR_UNSUPPORTED, "l2o_cwlstm_step_multi: at most %d segments", kMaxStepSegs);
  for (int i = 0; i < nseg; ++i)
    if (!segs[i].g || !segs[i].x || segs[i].B <= 0 || segs[i].D <= 0)
      return fail(L2O_ERR_ARG, "l2o_cwlstm_step: bad argument (segment %d)", i);
  const NetParams np = make_net_params(cfg, wpack);
  hipStream_t s = (hipStream_t)stream;
  if (cfg->n_layers == 0) {
    if (cfg->kind != L2O_NET_CW || cfg->preprocess == L2O_PRE_FC_ELU)
      return fail(L2O_ERR_UNSUPPORTED, "layers=() is implemented for CoordinateWiseDeepLSTM only");
    for (int i = 0; i < nseg; ++i) {
      const size_t n = (size_t)segs[i].B * segs[i].D;
      const dim3 grid((unsigned)((n + 255) / 256));
      if (cfg->preprocess == L2O_PRE_LOGSIGN)
        hipLaunchKernelGGL(k_linear_step<L2O_PRE_LOGSIGN>, grid, dim3(256), 0, s, np, segs[i].g, segs[i].x, n);
      else
        hipLaunchKernelGGL(k_linear_step<L2O_PRE_IDENTITY>, grid, dim3(256), 0, s, np, segs[i].g, segs[i].x, n);
    }
    HIP_TRY(hipGetLastError());
    return L2O_OK;
  }
  if (!net_ok_for_mfma(cfg)) return fail(L2O_ERR_UNSUPPORTED, "l2o_cwlstm_step: only layers=(20,20) / () nets");
  StepSegs sg;
  std::memset(&sg, 0, sizeof(sg));
  sg.n = nseg;
  int64_t ntiles = 0;
  for (int i = 0; i < nseg; ++i) {
    if (!segs[i].st) return fail(L2O_ERR_ARG, "l2o_cwlstm_step: NULL state");
    if (cfg->preprocess == L2O_PRE_FC_ELU && (!segs[i].m || !segs[i].v))
      return fail(L2O_ERR_ARG, "l2o_cwlstm_step: RNNProp needs m and v");
    sg.tpp[i] = tiles_per_problem(segs[i].D);
    sg.D[i] = (int)segs[i].D;
    ntiles += segs[i].B * sg.tpp[i];
    if (ntiles > INT32_MAX) return fail(L2O_ERR_UNSUPPORTED, "l2o_cwlstm_step: too many coordinates");
    sg.tile_end[i] = (int)ntiles;
    sg.g[i] = segs[i].g; sg.m[i] = segs[i].m; sg.v[i] = segs[i].v; sg.st[i] = segs[i].st; sg.x[i] = segs[i].x;
    sg.st_out[i] = segs[i].st_out ? segs[i].st_out : segs[i].st;
    sg.m_out[i] = segs[i].m_out ? segs[i].m_out : segs[i].m;
    sg.v_out[i] = segs[i].v_out ? segs[i].v_out : segs[i].v;
  }
  int blocks = (int)((ntiles + 3) / 4);
  if (blocks > 256) blocks = 256;            // one 4-wave block per CU (one wave per SIMD), grid-stride beyond
  const dim3 grid(blocks), block(256);
  const float om1 = (float)(1.0 - pow1), om2 = (float)(1.0 - pow2);
  with_pre(cfg->preprocess, [&](auto pre) { hipLaunchKernelGGL(k_cwlstm_step<decltype(pre)::value>, grid, block, 0, s, np, sg, om1, om2); });
  HIP_TRY(hipGetLastError());
  return L2O_OK;
}

int l2o_cwlstm_step(const l2o_net_cfg* cfg, const float* wpack, const float* g, float* m, float* v, double pow1,
                    double pow2, float* st, float* x, int64_t B, int64_t D, void* stream) {
  OptScope opt_scope(cfg_optw(cfg));
  l2o_step_seg seg;
  std::memset(&seg, 0, sizeof(seg));
  seg.g = g; seg.m = m; seg.v = v; seg.st = st; seg.x = x; seg.B = B; seg.D = D;
  return l2o_cwlstm_step_multi(cfg, wpack, &seg, 1, pow1, pow2, stream);
}

int l2o_unroll_supported(const l2o_net_cfg* cfg, const l2o_problem* prob) {
  OptScope opt_scope(cfg_optw(cfg));
  if (!cfg || !prob || !net_ok_for_mfma(cfg)) return 0;
  if (prob->kind != L2O_PROB_QUADRATIC && prob->kind != L2O_PROB_LASSO && prob->kind != L2O_PROB_RASTRIGIN &&
      prob->kind != L2O_PROB_SQUARE_COS)
    return 0;
  if (prob->D <= 0 || prob->M <= 0) return 0;
  UnrollGeom g;
  return (unroll_geom(prob, &g) || unroll_cu_eligible(prob)) ? 1 : 0;
}

int l2o_unroll_record_supported(const l2o_net_cfg* cfg, const l2o_problem* prob) {
  OptScope opt_scope(cfg_optw(cfg));
  return l2o_unroll_supported(cfg, prob);                   // every fused form records (ABI v6: the streaming form too)
}

size_t l2o_unroll_workspace_bytes(const l2o_net_cfg* cfg, const l2o_problem* prob, int32_t T) {
  OptScope opt_scope(cfg_optw(cfg));
  if (!l2o_unroll_supported(cfg, prob) || T < 0) return 0;
  UnrollGeom g;
  if (!unroll_geom(prob, &g) || g.CH < 2) return 0;       // (the streaming form needs no workspace)
  return pair_layout(prob, g, T).total;
}

int l2o_unroll_status(const void* workspace_header_host) {
  if (!workspace_header_host) return L2O_OK;
  const unsigned st = *static_cast<const unsigned*>(workspace_header_host);
  if (st == 0) return L2O_OK;
  if (st == 2)
    return fail(L2O_ERR_TIMEOUT, "l2o_mlp_unroll: a workgroup's all-reduce inputs never arrived (status 2): the persistent "
                             "launch was not fully co-resident (a shared / masked device?); the iterate and LSTM state "
                             "of that launch are invalid.  Run l2o_coresident_workgroups once so that the library "
                             "sizes against what is really available, or switch the fused form off "
                             "(L2O_OPT_MLP_UNROLL = 0 / L2O_NO_MLP_UNROLL=1)");
  return fail(L2O_ERR_TIMEOUT, "l2o_unroll: partner workgroup timed out (status %u): the two halves of a problem were not "
                           "co-resident (a shared / masked device?); the iterate and LSTM state of that launch are "
                           "invalid.  Run l2o_coresident_workgroups once so that the library sizes against what is "
                           "really available, or use one CU per problem (L2O_OPT_PAIR = 0 / L2O_NO_PAIR=1)", st);
}

static int unroll_impl(const l2o_net_cfg* cfg, const float* wpack, const l2o_problem* prob, float* x, float* st,
                       float* m, float* v, int32_t T, int32_t step0, float* fx_part, void* workspace,
                       const l2o_unroll_hist* hist, float* fx, void* stream, const float* x0 = nullptr, int flags = 0);

int l2o_unroll(const l2o_net_cfg* cfg, const float* wpack, const l2o_problem* prob, float* x, float* st, float* m,
               float* v, int32_t T, int32_t step0, float* fx_part, void* workspace, void* stream) {
  OptScope opt_scope(cfg_optw(cfg));
  return unroll_impl(cfg, wpack, prob, x, st, m, v, T, step0, fx_part, workspace, nullptr, nullptr, stream);
}

int l2o_unroll_record(const l2o_net_cfg* cfg, const float* wpack, const l2o_problem* prob, float* x, float* st,
                      float* m, float* v, int32_t T, int32_t step0, float* fx_part, void* workspace,
                      const l2o_unroll_hist* hist, void* stream) {
  OptScope opt_scope(cfg_optw(cfg));
  return unroll_impl(cfg, wpack, prob, x, st, m, v, T, step0, fx_part, workspace, hist, nullptr, stream);
}

int l2o_unroll_reduce(const l2o_net_cfg* cfg, const float* wpack, const l2o_problem* prob, const float* x0, float* x,
                      float* st, float* m, float* v, int32_t T, int32_t step0, int32_t flags, float* fx_part, float* fx,
                      void* workspace, const l2o_unroll_hist* hist, void* stream) {
  OptScope opt_scope(cfg_optw(cfg));
  if (!fx) return fail(L2O_ERR_ARG, "l2o_unroll_reduce: NULL fx");
  if (flags & ~L2O_UNROLL_ZERO_STATE)
    return fail(L2O_ERR_ARG, "l2o_unroll_reduce: unknown flags %d", flags);
  return unroll_impl(cfg, wpack, prob, x, st, m, v, T, step0, fx_part, workspace, hist, fx, stream, x0, flags);
}

int32_t l2o_coresident_workgroups(void* scratch, void* stream) {
  if (!scratch) return fail(L2O_ERR_ARG, "l2o_coresident_workgroups: NULL scratch");
  hipStream_t s = (hipStream_t)stream;
  const int dev = device_ordinal(s);
  if (dev >= 0 && dev < 64) {
    const int m = g_measured_cus[dev].load(std::memory_order_relaxed);
    if (m > 0) return m;
  }
  const int n = device_cu_count(s);
  if (n <= 0) return fail(L2O_ERR_HIP, "l2o_coresident_workgroups: no device");
  unsigned* d = static_cast<unsigned*>(scratch);
  constexpr int kLds = 100 * 1024;                           // more than half a CU's LDS: one workgroup per CU
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_coresident_probe), hipFuncAttributeMaxDynamicSharedMemorySize, kLds));
  // A pass can only UNDER-count (a slow dispatch lets the earliest workgroup sample before the others arrived), never
  // over-count (at most `capacity` workgroups exist until the first one leaves): the maximum of a few passes.
  int got = 0;
  for (int pass = 0; pass < 3; ++pass) {
    const unsigned init[2] = {0u, 0xffffffffu};
    HIP_TRY(hipMemcpyAsync(d, init, sizeof(init), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_coresident_probe, dim3(n), dim3(256), kLds, s, d, d + 1);
    HIP_TRY(hipGetLastError());
    unsigned out[2] = {0u, 0u};
    HIP_TRY(hipMemcpyAsync(out, d, sizeof(out), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const int seen = (int)out[1];
    if (seen > got && seen <= n) got = seen;
    if (got == n) break;
  }
  if (got <= 0) got = n;
  if (dev >= 0 && dev < 64) g_measured_cus[dev].store(got, std::memory_order_relaxed);
  return got;
}

int l2o_unroll_workspace_init(void* workspace, size_t bytes, void* stream) {
  if (!workspace && bytes) return fail(L2O_ERR_ARG, "l2o_unroll_workspace_init: NULL workspace");
  if (bytes) HIP_TRY(hipMemsetAsync(workspace, 0, bytes, (hipStream_t)stream));
  return L2O_OK;
}

int64_t l2o_unroll_workspace_layout(const l2o_net_cfg* cfg, const l2o_problem* prob) {
  OptScope opt_scope(cfg_optw(cfg));
  UnrollGeom g;
  if (!cfg || !prob || !l2o_unroll_supported(cfg, prob) || !unroll_geom(prob, &g) || g.CH < 2) return 0;
  return ((int64_t)prob->B_local << 8) | g.CH;            // changes whenever the granule area's layout does
}

static int unroll_impl(const l2o_net_cfg* cfg, const float* wpack, const l2o_problem* prob, float* x, float* st,
                       float* m, float* v, int32_t T, int32_t step0, float* fx_part, void* workspace,
                       const l2o_unroll_hist* hist, float* fx, void* stream, const float* x0, int flags) {
  int rc = check_problem(prob);
  if (rc) return rc;
  if (!cfg || !wpack || !x || !st || !fx_part || T < 0) return fail(L2O_ERR_ARG, "l2o_unroll: bad argument");
  if (hist && (!hist->st || !hist->g || !hist->g_final ||
               (cfg->preprocess == L2O_PRE_FC_ELU && (!hist->m || !hist->v))))
    return fail(L2O_ERR_ARG, "l2o_unroll_record: incomplete history buffers");
  if (!l2o_unroll_supported(cfg, prob))
    return fail(L2O_ERR_UNSUPPORTED, "l2o_unroll: no fused kernel for kind=%d D=%d M=%d net(kind=%d,layers=%d)",
                prob->kind, prob->D, prob->M, cfg->kind, cfg->n_layers);
  UnrollGeom g;
  const bool lds_form = unroll_geom(prob, &g);
  UnrollArgs a;
  a.np = make_net_params(cfg, wpack);
  a.pp = make_prob_params(prob);
  a.x = x; a.st = st; a.m = m; a.v = v; a.fx_part = fx_part;
  a.x_in = x0; a.zero_state = (flags & L2O_UNROLL_ZERO_STATE) ? 1 : 0;
  a.ticks = nullptr;
  a.T = T;
  a.hist_st = hist ? hist->st : nullptr;
  a.hist_g = hist ? hist->g : nullptr;
  a.hist_m = hist ? hist->m : nullptr;
  a.hist_v = hist ? hist->v : nullptr;
  a.hist_gfinal = hist ? hist->g_final : nullptr;
  pow_ff(cfg->beta1, step0, &a.p1_hi, &a.p1_lo);
  pow_ff(cfg->beta2, step0, &a.p2_hi, &a.p2_lo);
  hipStream_t s = (hipStream_t)stream;
  bool fx_done = false;
  rc = L2O_OK;
  if (cfg->preprocess == L2O_PRE_FC_ELU && (!m || !v)) return fail(L2O_ERR_ARG, "l2o_unroll: RNNProp needs m and v");
  if (!lds_form) {
    rc = with_pre(cfg->preprocess, [&](auto pre) { return launch_unroll_cu<decltype(pre)::value>(a, s); });
  } else {
    rc = with_pre(cfg->preprocess, [&](auto pre) {
      return launch_unroll_kind<decltype(pre)::value>(a, g, prob->kind, s, prob, workspace, fx, &fx_done);
    });
  }
  if (rc) return rc;
  if (fx && !fx_done)                                       // forms without the fused epilogue: the separate reduction
    return l2o_reduce_fx(fx_part, T + 1, prob->B_local, prob->B_global, fx, stream);
  return L2O_OK;
}

}  // extern "C"
