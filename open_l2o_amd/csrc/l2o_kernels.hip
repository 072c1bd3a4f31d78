// l2o_kernels.hip -- gfx950 (MI355X / CDNA4) kernels + the C ABI of include/l2o_abi.h.
//
// Reference semantics (file:line under /root/reference/Model_Free_L2O/
// "L2O-DM and L2O-RNNProp"/, shorthand DM/):
//   unroll loop        DM/meta.py:319-389, DM/meta_rnnprop_eval.py (time_step/update)
//   optimizer nets     DM/networks.py:157-300
//   preprocess         DM/preprocess.py:26-70
//   optimizees         DM/problems.py:41-213
// Written for gfx950 only: wave64, v_mfma_f32_16x16x4_f32, 160 KiB LDS per CU.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "l2o_common.h"
#include "l2o_lstm_bx3.h"
#include "l2o_params.h"
#include "l2o_step.h"
#include "l2o_problem_fg.h"
#include "l2o_unroll.h"
#include "l2o_unroll_pair.h"
#include "l2o_unroll_lds.h"
#include "l2o_unroll_cu.h"
#include "l2o_unroll_cu8.h"
#include "l2o_ilp_kernels.h"   // the plain two-CU / eight-wave unrolls: code in l2o_kernels_ilp.hip, `extern template` here
#include "l2o_mlp.h"
#include "l2o_mlp_unroll.h"
#include "l2o_mlp_xcd.h"
#include "l2o_mlp_deep.h"
#include "l2o_mlp_hvp.h"
#include "l2o_mnist_conv.h"
#include "l2o_cifar_conv.h"
#include "l2o_lenet.h"
#include "l2o_vgg16.h"
#include "l2o_nas.h"
#include "l2o_confocal.h"
#include "l2o_confocal_unroll.h"
#include "l2o_generic.h"
#include "l2o_klstm.h"
#include "../../include/l2o_klstm_abi.h"
#include "l2o_atb.h"
#include "l2o_bwd.h"
#include "l2o_bwd_mfma.h"
#include "l2o_vecops.h"
#include "l2o_util_kernels.h"

using namespace l2o;

// ---------------------------------------------------------------------------
// error plumbing
// ---------------------------------------------------------------------------
static thread_local char g_err[512] = "";
// which kernel form the last l2o_unroll* / l2o_mlp_unroll* call of this thread launched (l2o_last_unroll_form, ABI v12):
// L2O_FORM_* | dispatches << 8.  Diagnostic only, like g_err -- no launch depends on it.
static thread_local int g_last_form = 0;
// ... and which instantiation of that template (l2o_last_unroll_variant: the L2O_VARIANT_* fields of include/l2o_abi.h; the
// five unroll launchers set it right after note_form, every other form leaves the 0 note_form stores)
static thread_local int g_last_variant = 0;
static inline void note_form(int form, int dispatches = 1) { g_last_form = form | (dispatches << 8); g_last_variant = 0; }
static inline void note_variant(int ch, bool hist, bool exact, bool fast, int kr, int nv) {
  g_last_variant = L2O_VARIANT(ch, hist ? 1 : 0, exact ? 1 : 0, fast ? 1 : 0, kr, nv);
}

static int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}
#define HIP_TRY(expr)                                                              \
  do {                                                                             \
    hipError_t e_ = (expr);                                                        \
    if (e_ != hipSuccess) return fail(L2O_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

// the run-time preprocess kind as a template argument: f(std::integral_constant<int, L2O_PRE_...>{}), FC_ELU for every other value
template <class F>
static auto with_pre(int pre, F&& f) {
  switch (pre) {
    case L2O_PRE_IDENTITY: return f(std::integral_constant<int, L2O_PRE_IDENTITY>{});
    case L2O_PRE_LOGSIGN: return f(std::integral_constant<int, L2O_PRE_LOGSIGN>{});
    default: return f(std::integral_constant<int, L2O_PRE_FC_ELU>{});
  }
}
// a launch with `lds` bytes of dynamic LDS: raise the kernel's limit (every time: no host-side state), launch, check
template <class K, class... A>
static int launch(K fn, dim3 grid, dim3 block, size_t lds, hipStream_t s, const A&... args) {
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(fn, grid, block, lds, s, args...);
  HIP_TRY(hipGetLastError());
  return L2O_OK;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
static bool net_ok_for_mfma(const l2o_net_cfg* c) {
  if (c->n_layers != 2 || c->hidden != kH) return false;
  if (c->kind == L2O_NET_CW) return c->preprocess == L2O_PRE_IDENTITY || c->preprocess == L2O_PRE_LOGSIGN;
  if (c->kind == L2O_NET_RNNPROP) return c->preprocess == L2O_PRE_FC_ELU;
  return false;
}

static NetParams make_net_params(const l2o_net_cfg* c, const float* wpack) {
  NetParams np;
  np.wpack = wpack;
  np.scale = (float)c->scale;
  np.k_inv_ln2 = c->logsign_k != 0.0 ? (float)(0.6931471805599453 / c->logsign_k) : 0.0f;
  np.exp_k = (float)std::exp(c->logsign_k);
  np.beta1 = (float)c->beta1;
  np.beta2 = (float)c->beta2;
  np.omb1 = (float)(1.0 - c->beta1);
  np.omb2 = (float)(1.0 - c->beta2);
  np.tanh_output = c->tanh_output;
  return np;
}

static ProbParams make_prob_params(const l2o_problem* p) {
  ProbParams pp;
  pp.kind = p->kind;
  pp.B_local = p->B_local;
  pp.D = p->D;
  pp.M = p->kind == L2O_PROB_SIMPLE ? 0 : p->M;
  pp.w_shared = (p->flags & L2O_PROB_W_SHARED) ? 1 : 0;
  pp.hvp = 0;
  pp.inv_bg = 1.0f / (float)p->B_global;
  pp.l1 = (float)p->l1;
  pp.alpha = p->kind == L2O_PROB_SQUARE_COS ? 10.0f : (float)p->alpha;
  pp.twopi = p->kind == L2O_PROB_SQUARE_COS ? (float)(2 * 3.1415926) : 6.2831853071795864769f;
  pp.W = p->W;
  pp.y = p->y;
  pp.C = p->C;
  pp.x_scale = p->x_scale;
  return pp;
}

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

// float-float split of base^k computed in double
static void pow_ff(double base, int k, float* hi, float* lo) {
  const double p = std::pow((double)(float)base, (double)k);
  *hi = (float)p;
  *lo = (float)(p - (double)*hi);
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

// ---------------------------------------------------------------------------
// options: A/B switches between kernels that compute the same thing.  The library keeps NO option state: every call
// carries its switches in the caller's own structs -- l2o_net_cfg.options (L2O_OPTW(option, value) words OR-ed
// together; 0 = every default), l2o_problem.flags (L2O_PROB_FG_TWO_PASS) and l2o_mlp.flags (L2O_MLP_GENERIC).  An entry
// point copies the word into a call-scoped thread-local (OptScope) that the launch helpers below read through opt().
// ---------------------------------------------------------------------------
static const int64_t kOptDefault[L2O_OPT_COUNT_] = {
    /* L2O_OPT_PAIR */ 1, /* L2O_OPT_PAIR_PLAIN_STORES */ 1, /* L2O_OPT_UNROLL_CU */ 1,
    /* L2O_OPT_FG_TWO_PASS */ 0, /* L2O_OPT_MLP_GENERIC */ 0, /* L2O_OPT_BWD_BLOCKS */ 0,
    /* L2O_OPT_BWD_KERNEL */ 0, /* L2O_OPT_MLP_UNROLL */ 1, /* L2O_OPT_MLP_XCD_WAVES */ 0, /* L2O_OPT_EXACT_GATES */ 0,
    /* L2O_OPT_WPACK_NO_CLEAR */ 0, /* L2O_OPT_MLP_HIER */ 1, /* L2O_OPT_ONE_LDS */ 1, /* L2O_OPT_PAIR_FAST_LOAD */ 1};
static thread_local uint64_t t_optw = 0;
struct OptScope {
  uint64_t saved;
  explicit OptScope(uint64_t w) : saved(t_optw) { t_optw = w; }
  ~OptScope() { t_optw = saved; }
};
static inline uint64_t cfg_optw(const l2o_net_cfg* cfg) { return cfg ? cfg->options : 0; }
static inline int64_t opt(int o) {
  if (o == L2O_OPT_BWD_BLOCKS) return (int64_t)((t_optw >> 48) & 0xfffu);      // a count: its own 12-bit field
  const unsigned nib = (unsigned)(t_optw >> (4 * L2O_OPT_FIELD_(o))) & 0xfu;
  return (nib & 8u) ? (int64_t)(nib & 7u) : kOptDefault[o];
}

// CUs of the device the call runs on (the stream's device; the current device for the null stream).
// Immutable hardware facts cached per device ordinal -- not launch state.
static int device_cu_count(hipStream_t s) {
  constexpr int kMaxDev = 64;
  static std::atomic<int> cache[kMaxDev];
  int dev = -1;
  if (s == nullptr || hipStreamGetDevice(s, &dev) != hipSuccess || dev < 0) {
    if (hipGetDevice(&dev) != hipSuccess) return 0;
  }
  if (dev < kMaxDev) {
    const int c = cache[dev].load(std::memory_order_relaxed);
    if (c > 0) return c;
  }
  int n = 0;
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
  if (dev < kMaxDev) cache[dev].store(n, std::memory_order_relaxed);
  return n;
}

static int device_ordinal(hipStream_t s) {
  int dev = -1;
  if (s == nullptr || hipStreamGetDevice(s, &dev) != hipSuccess || dev < 0) {
    if (hipGetDevice(&dev) != hipSuccess) return -1;
  }
  return dev;
}
// measured co-resident one-per-CU workgroups per device (l2o_coresident_workgroups); 0 = never probed
static std::atomic<int> g_measured_cus[64];

// CUs on which workgroups of a launch on stream `s` can be resident AT THE SAME TIME -- what the kernels with
// inter-workgroup exchanges (two-CU unroll, l2o_mlp_unroll) size their grids against:
//   the device's CU count (reflects ROC_GLOBAL_CU_MASK and the partition mode), the stream's own CU mask
//   (hipExtStreamCreateWithCUMask; 0.3 us per query), and the MEASURED capacity where the caller ran the probe
//   (restrictions below HIP, e.g. HSA_CU_MASK: the device still reports every CU).
static int coresident_cus(hipStream_t s) {
  int n = device_cu_count(s);
  uint32_t mask[16] = {0};
  if (hipExtStreamGetCUMask(s, 16, mask) == hipSuccess) {
    int pop = 0;
    for (uint32_t w : mask) pop += __builtin_popcount(w);
    if (pop > 0 && pop < n) n = pop;
  } else {
    (void)hipGetLastError();
  }
  const int dev = device_ordinal(s);
  if (dev >= 0 && dev < 64) {
    const int m = g_measured_cus[dev].load(std::memory_order_relaxed);
    if (m > 0 && m < n) n = m;
  }
  return n;
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

// the fused unroll of the confocal optimizee (csrc/l2o_confocal_unroll.h): one workgroup per batch row
template <int PRE>
static int launch_confocal_unroll(const CfUnrollArgs& a, bool hist, size_t lds, hipStream_t s) {
  void (*fn)(CfUnrollArgs) = hist ? k_cf_unroll<PRE, true> : k_cf_unroll<PRE, false>;
  return launch(fn, dim3(a.batch), dim3(kCfThreads), lds, s, a);
}

// ... and several instances per launch: n_inst x batch workgroups, the pointers out of the tables in device scratch
template <int PRE>
static int launch_confocal_unroll_multi(const CfUnrollMultiArgs& a, int n_inst, bool hist, size_t lds, hipStream_t s) {
  void (*fn)(CfUnrollMultiArgs) = hist ? k_cf_unroll<PRE, true, true> : k_cf_unroll<PRE, false, true>;
  return launch(fn, dim3(n_inst * a.batch), dim3(kCfThreads), lds, s, a);
}

extern "C" {

int l2o_abi_version(void) { return L2O_ABI_VERSION; }
const char* l2o_last_error(void) { return g_err; }
#ifndef L2O_BUILD_ID
#define L2O_BUILD_ID "unknown"
#endif
const char* l2o_build_id(void) { return L2O_BUILD_ID; }
int l2o_last_unroll_form(void) { return g_last_form; }
int l2o_last_unroll_variant(void) { return g_last_variant; }

size_t l2o_wpack_floats(const l2o_net_cfg* cfg) {
  if (!cfg) return 0;
  if (cfg->n_layers == 0) return 4;
  if (!net_ok_for_mfma(cfg)) return 0;
  return (size_t)wp_rows(cfg->preprocess) * 64 + (size_t)bx::words(cfg->preprocess) + (size_t)bxb::words(cfg->preprocess);
}

int l2o_wpack_host(const l2o_net_cfg* cfg, const float* wg1, const float* bg1, const float* wg2,
                   const float* bg2, const float* wl, const float* bl, const float* wfc, const float* bfc,
                   float* out) {
  if (!cfg || !out || !wl || !bl) return fail(L2O_ERR_ARG, "l2o_wpack_host: NULL argument");
  if (cfg->n_layers == 0) {
    // Linear(P -> 1) on the preprocessed gradient, P = 1 (identity) or 2 (LogAndSign)
    if (cfg->kind != L2O_NET_CW || cfg->preprocess == L2O_PRE_FC_ELU)
      return fail(L2O_ERR_UNSUPPORTED, "layers=() is implemented for CoordinateWiseDeepLSTM only");
    out[0] = wl[0];
    out[1] = cfg->preprocess == L2O_PRE_LOGSIGN ? wl[1] : 0.0f;
    out[2] = bl[0];
    out[3] = 0.0f;
    return L2O_OK;
  }
  if (!net_ok_for_mfma(cfg))
    return fail(L2O_ERR_UNSUPPORTED, "MFMA kernels implement layers=(20,20) (got n_layers=%d hidden=%d kind=%d pre=%d)",
                cfg->n_layers, cfg->hidden, cfg->kind, cfg->preprocess);
  if (!wg1 || !bg1 || !wg2 || !bg2) return fail(L2O_ERR_ARG, "l2o_wpack_host: NULL LSTM weights");
  const int pre = cfg->preprocess;
  const bool fc = pre == L2O_PRE_FC_ELU;
  if (fc && (!wfc || !bfc)) return fail(L2O_ERR_ARG, "l2o_wpack_host: fc preprocess needs input_projection");
  std::memset(out, 0, sizeof(float) * l2o_wpack_floats(cfg));
  for (int l = 0; l < 64; ++l) wpack_lane(pre, l, 0, kNT, 0, bxb::ntiles(pre), wg1, bg1, wg2, bg2, wl, bl, wfc, bfc, out);
  return L2O_OK;
}

int l2o_wpack_device(const l2o_net_cfg* cfg, const l2o_net_weights* w, float* wpack, void* stream) {
  OptScope opt_scope(cfg_optw(cfg));
  if (!cfg || !w || !wpack) return fail(L2O_ERR_ARG, "l2o_wpack_device: NULL argument");
  if (!net_ok_for_mfma(cfg) || cfg->n_layers == 0)
    return fail(L2O_ERR_UNSUPPORTED, "l2o_wpack_device: layers=(20,20) nets only");
  const bool fc = cfg->preprocess == L2O_PRE_FC_ELU;
  if (!w->w_gates1 || !w->b_gates1 || !w->w_gates2 || !w->b_gates2 || !w->w_lin || !w->b_lin ||
      (fc && (!w->w_fc || !w->b_fc)))
    return fail(L2O_ERR_ARG, "l2o_wpack_device: NULL weight pointer");
  hipStream_t s = (hipStream_t)stream;
  if (!opt(L2O_OPT_WPACK_NO_CLEAR)) HIP_TRY(hipMemsetAsync(wpack, 0, sizeof(float) * l2o_wpack_floats(cfg), s));
  hipLaunchKernelGGL(k_wpack, dim3(kNT * bx::nchunks(cfg->preprocess) + 4 * bxb::ntiles(cfg->preprocess)), dim3(64), 0, s, (int)cfg->preprocess, w->w_gates1, w->b_gates1, w->w_gates2,
                     w->b_gates2, w->w_lin, w->b_lin, w->w_fc, w->b_fc, wpack);
  HIP_TRY(hipGetLastError());
  return L2O_OK;
}

static int adam_launch(float* w, float* m, float* v, const float* g, int64_t n, float lr_t, double beta1, double beta2,
                       double epsilon, const unsigned* guard, void* stream, const int* map = nullptr) {
  if (!w || !m || !v || !g || n < 0) return fail(L2O_ERR_ARG, "l2o_adam_step: bad argument");
  if (n == 0) return L2O_OK;
  hipLaunchKernelGGL(k_adam, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, m, v, g, (long)n,
                     lr_t, (float)beta1, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)epsilon, guard, map);
  HIP_TRY(hipGetLastError());
  return L2O_OK;
}
int l2o_adam_step(float* w, float* m, float* v, const float* g, int64_t n, float lr_t, double beta1, double beta2,
                  double epsilon, void* stream) {
  return adam_launch(w, m, v, g, n, lr_t, beta1, beta2, epsilon, nullptr, stream);
}
int l2o_adam_step_gather(float* w, float* m, float* v, const float* G, const int32_t* map, int64_t n, float lr_t,
                         double beta1, double beta2, double epsilon, const void* unroll_workspace, void* stream) {
  if (!map) return fail(L2O_ERR_ARG, "l2o_adam_step_gather: NULL map");
  return adam_launch(w, m, v, G, n, lr_t, beta1, beta2, epsilon, static_cast<const unsigned*>(unroll_workspace), stream, map);
}
int l2o_adam_step_guarded(float* w, float* m, float* v, const float* g, int64_t n, float lr_t, double beta1,
                          double beta2, double epsilon, const void* unroll_workspace, void* stream) {
  // (the status word is the first member of the workspace header: l2o_unroll_status reads the same 4 bytes)
  return adam_launch(w, m, v, g, n, lr_t, beta1, beta2, epsilon, static_cast<const unsigned*>(unroll_workspace), stream);
}

size_t l2o_state_floats(int64_t B, int64_t D) {
  if (B <= 0 || D <= 0) return 0;
  return (size_t)B * tiles_per_problem(D) * kStateFloatsPerTile;
}

static int state_repack(float* h1, float* c1, float* h2, float* c2, float* st, int64_t B, int64_t D,
                        void* stream, int to_packed) {
  if (!h1 || !c1 || !h2 || !c2 || !st || B <= 0 || D <= 0) return fail(L2O_ERR_ARG, "state repack: bad argument");
  const int tpp = tiles_per_problem(D);
  const size_t total = (size_t)B * tpp * 64 * 20;
  hipLaunchKernelGGL(k_state_repack, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, h1,
                     c1, h2, c2, st, (int)B, (int)D, tpp, to_packed);
  HIP_TRY(hipGetLastError());
  return L2O_OK;
}
int l2o_state_pack(const float* h1, const float* c1, const float* h2, const float* c2, float* st, int64_t B,
                   int64_t D, void* stream) {
  return state_repack(const_cast<float*>(h1), const_cast<float*>(c1), const_cast<float*>(h2),
                      const_cast<float*>(c2), st, B, D, stream, 1);
}
int l2o_state_unpack(const float* st, float* h1, float* c1, float* h2, float* c2, int64_t B, int64_t D,
                     void* stream) {
  return state_repack(h1, c1, h2, c2, const_cast<float*>(st), B, D, stream, 0);
}

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

int l2o_mlp_fg(const l2o_mlp* mlp, const int32_t* indices, const float* w1, const float* b1, const float* w2,
               const float* b2, float* loss, float* gw1, float* gb1, float* gw2, float* gb2, float* scratch,
               void* stream) {
  OptScope opt_scope((mlp && (mlp->flags & L2O_MLP_GENERIC)) ? L2O_OPTW(L2O_OPT_MLP_GENERIC, 1) : 0);
  if (!mlp || !indices || !w1 || !b1 || !w2 || !b2 || !loss || !mlp->images || !mlp->labels)
    return fail(L2O_ERR_ARG, "l2o_mlp_fg: NULL argument");
  const bool want_g = gw1 || gb1 || gw2 || gb2;
  if (want_g && !(gw1 && gb1 && gw2 && gb2)) return fail(L2O_ERR_ARG, "l2o_mlp_fg: pass all four gradients or none");
  if (mlp->n_hidden < 1 || mlp->n_hidden > kMlpMaxH || mlp->n_out < 1 || mlp->n_out > kMlpMaxO ||
      mlp->batch < 1 || mlp->batch > 256 || mlp->n_in < 1 || mlp->n_in > kMlpTPS * kMlpKPT)
    return fail(L2O_ERR_UNSUPPORTED, "l2o_mlp_fg: sizes n_in=%d hidden=%d out=%d batch=%d not implemented",
                mlp->n_in, mlp->n_hidden, mlp->n_out, mlp->batch);
  if (!scratch) return fail(L2O_ERR_ARG, "l2o_mlp_fg: NULL scratch (l2o_mlp_scratch_floats)");
  MlpParams p;
  p.n_in = mlp->n_in; p.H = mlp->n_hidden; p.O = mlp->n_out; p.batch = mlp->batch; p.act = mlp->activation;
  p.images = mlp->images; p.labels = mlp->labels; p.idx = indices;
  p.w1 = w1; p.b1 = b1; p.w2 = w2; p.b2 = b2; p.loss = loss;
  p.gw1 = gw1; p.gb1 = gb1; p.gw2 = gw2; p.gb2 = gb2;
  p.scratch = scratch;
  hipStream_t s = (hipStream_t)stream;
  const int HP = p.H == 20 ? 20 : kMlpMaxH;             // padded hidden width of the kernels' hot loops
  const int HS = HP | 1;
  const size_t lds_f = sizeof(float) * ((HP == 20 ? 0 : (size_t)p.n_in * HS) + (size_t)kMlpSPB * kMlpTPS * HP + (size_t)kMlpSPB * p.H +
                                        (size_t)kMlpSPB * p.O + (size_t)p.H * p.O + p.H + p.O);
  size_t lds_b = sizeof(float) * ((size_t)p.batch * HP + (size_t)p.batch + 4 * (size_t)kMlpKPB * HP);
  const size_t lds_small = sizeof(float) * (size_t)p.batch * (2 * p.H + p.O + 1);   // the small-tensor workgroup's copy of scratch
  if (lds_small > lds_b) lds_b = lds_small;
  if (lds_f > 160 * 1024 || lds_b > 160 * 1024)
    return fail(L2O_ERR_UNSUPPORTED, "l2o_mlp_fg: needs %zu / %zu bytes of LDS", lds_f, lds_b);
  if (p.H == kMlp20 && !opt(L2O_OPT_MLP_GENERIC)) {       // the reference's width: barrier-free forward, scalar-operand backward
    hipLaunchKernelGGL(k_mlp_fwd20, dim3(p.batch), dim3(64), 0, s, p);
    HIP_TRY(hipGetLastError());
    const int nkb20 = (p.n_in + 63) / 64;
    size_t lds20 = sizeof(float) * (size_t)kMlpBwdWaves * 64 * (kMlp20 + 1);
    if (lds_small > lds20) lds20 = lds_small;
    return launch(k_mlp_bwd20, dim3(nkb20 + 1), dim3(64 * kMlpBwdWaves), lds20, s, p);
  }
  void (*ffwd)(MlpParams) = HP == 20 ? k_mlp_fwd<20> : k_mlp_fwd<kMlpMaxH>;
  void (*fbwd)(MlpParams) = HP == 20 ? k_mlp_bwd<20> : k_mlp_bwd<kMlpMaxH>;
  const int rc = launch(ffwd, dim3((p.batch + kMlpSPB - 1) / kMlpSPB), dim3(256), lds_f, s, p);
  if (rc) return rc;
  const int nkb = (p.n_in + kMlpKPB - 1) / kMlpKPB;
  return launch(fbwd, dim3(nkb + 1), dim3(256), lds_b, s, p);
}

size_t l2o_mlp_scratch_floats(const l2o_mlp* mlp) {
  if (!mlp || mlp->batch < 1) return 0;
  return (size_t)mlp->batch * (2 * (size_t)mlp->n_hidden + mlp->n_out + 1);
}

// ---- G = A^T B, the weight-gradient contraction of the meta-gradient (csrc/l2o_atb.h) ----------------------
static int atb_groups(int64_t R, int wgs_per_cu, hipStream_t s) {
  const int64_t nblk = (R + kAtbRows - 1) / kAtbRows;
  int g = wgs_per_cu * device_cu_count(s);                // persistent workgroups (k_atb: 72 KB of LDS each, k_atb_bx3: 52 | 58)
  if (g <= 0 || g > kAtbMaxGroups) g = kAtbMaxGroups;
  return (int)(nblk < g ? nblk : g);
}
size_t l2o_atb_workspace_bytes(int64_t R, int32_t KA, int32_t KB) {
  if (R <= 0 || KA <= 0 || KB <= 0) return 0;
  return sizeof(float) * (size_t)kAtbMaxGroups * KA * KB;
}
// mask 0: the dense product (fp32 matrix pipe, exact products).  mask 1 | 2: the weight-gradient blocks -- on the
// bf16 pipe (k_atb_bx3) unless the call asks for exact gates (L2O_OPT_EXACT_GATES: the fp32 pipe, bit-equal to the
// dense product on those blocks)
// compact_rows > 0 (mask 1 | 2, bf16 pipe only): A is the COMPACT operand of l2o_cwlstm_bwd_unroll_compact -- T + 1 blocks of
// compact_rows rows of KA - 40 floats -- and R = T * compact_rows rows of B (csrc/l2o_atb.h: atb_compact_off)
static int atb_launch(const float* A, const float* B, int64_t R, int KA, int KB, int mask, float* out, void* workspace,
                      hipStream_t s, int64_t compact_rows = 0, int P = 0) {
  float* part = static_cast<float*>(workspace);
  const int MT = (KA + 15) / 16, NT = (KB + 15) / 16;
  void (*fn)(const float*, const float*, long, int, int, float*) = nullptr;
  void (*fx)(const float*, const float*, long, int, int, float*, int, unsigned, int) = nullptr;
  int wgs = L2O_ATB_WGS_PER_CU;
  const bool bx3 = mask != 0 && !opt(L2O_OPT_EXACT_GATES);
  if (compact_rows > 0 && !bx3) return fail(L2O_ERR_UNSUPPORTED, "the compact A operand is read by the bf16x3 contraction only");
  if (mask == 1) {
    if (bx3) { fx = k_atb_bx3<6, 11, 1>; wgs = atb_bx3_wgs_per_cu<6, 11>(); } else fn = k_atb<6, 11, 1>;
  } else if (mask == 2) {
    if (bx3) { fx = k_atb_bx3<7, 12, 2>; wgs = atb_bx3_wgs_per_cu<7, 12>(); } else fn = k_atb<7, 12, 2>;
  } else if (MT <= 1 && NT <= 1) fn = k_atb<1, 1>;
  else if (MT <= 6 && NT <= 11) fn = k_atb<6, 11>;
  else fn = k_atb<7, 12>;
  const int groups = atb_groups(R, wgs, s);
  if (fx) {
    const int KAs = compact_rows > 0 ? KA - 2 * kH : KA;
    const uint64_t slice = compact_rows > 0 ? (uint64_t)compact_rows * KAs * sizeof(float) : 0;
    if (slice > 0xf0000000ull) return fail(L2O_ERR_UNSUPPORTED, "l2o_cwlstm_wgrad_compact: %lld rows per step is too many", (long long)compact_rows);
    hipLaunchKernelGGL(fx, dim3(groups), dim3(256), 0, s, A, B, (long)R, KA, KB, part, KAs, (unsigned)slice, P);
  } else {
    hipLaunchKernelGGL(fn, dim3(groups), dim3(256), 0, s, A, B, (long)R, KA, KB, part);
  }
  HIP_TRY(hipGetLastError());
  const int n = KA * KB;
  hipLaunchKernelGGL(k_atb_reduce, dim3((n + 31) / 32), dim3(256), 0, s, part, groups, n, out, mask,
                     mask == 2 ? 12 : 11, KB);
  HIP_TRY(hipGetLastError());
  return L2O_OK;
}

int l2o_atb(const float* A, const float* B, int64_t R, int32_t KA, int32_t KB, float* out, void* workspace, void* stream) {
  if (!A || !B || !out || !workspace || R <= 0 || KA <= 0 || KB <= 0) return fail(L2O_ERR_ARG, "l2o_atb: bad argument");
  if (KA > 112 || KB > 192) return fail(L2O_ERR_UNSUPPORTED, "l2o_atb: KA <= 112 and KB <= 192 (got %d x %d)", KA, KB);
  return atb_launch(A, B, R, KA, KB, 0, out, workspace, (hipStream_t)stream);
}

int32_t l2o_cwlstm_wgrad_dims(const l2o_net_cfg* cfg, int32_t* KA, int32_t* KB) {
  if (!cfg || !net_ok_for_mfma(cfg) || cfg->n_layers == 0) return fail(L2O_ERR_UNSUPPORTED, "l2o_cwlstm_wgrad: layers=(20,20) nets only");
  const bool fc = cfg->preprocess == L2O_PRE_FC_ELU;
  const int P = fc ? kH : (cfg->preprocess == L2O_PRE_LOGSIGN ? 2 : 1);
  if (KA) *KA = P + kH + 3 * kH + (fc ? 2 : 0) + 1;         // act1 | act2 | h2 | feats | 1   (BwdTileGeom::KA)
  if (KB) *KB = 8 * kH + 1 + (fc ? kH : 0);                 // dz1 | dz2 | dd | du             (BwdTileGeom::KB)
  return L2O_OK;
}

int l2o_cwlstm_wgrad(const l2o_net_cfg* cfg, const float* A, const float* Bm, int64_t R, float* G, void* workspace,
                     void* stream) {
  OptScope opt_scope(cfg_optw(cfg));
  int32_t KA = 0, KB = 0;
  const int rc = l2o_cwlstm_wgrad_dims(cfg, &KA, &KB);
  if (rc) return rc;
  if (!A || !Bm || !G || !workspace || R <= 0) return fail(L2O_ERR_ARG, "l2o_cwlstm_wgrad: bad argument");
  return atb_launch(A, Bm, R, KA, KB, cfg->preprocess == L2O_PRE_FC_ELU ? 2 : 1, G, workspace, (hipStream_t)stream);
}

int l2o_cwlstm_wgrad_compact(const l2o_net_cfg* cfg, const float* Ac, const float* Bm, int32_t T, int64_t rows, float* G,
                             void* workspace, void* stream) {
  OptScope opt_scope(cfg_optw(cfg));
  int32_t KA = 0, KB = 0;
  const int rc = l2o_cwlstm_wgrad_dims(cfg, &KA, &KB);
  if (rc) return rc;
  if (!Ac || !Bm || !G || !workspace || T <= 0 || rows <= 0) return fail(L2O_ERR_ARG, "l2o_cwlstm_wgrad_compact: bad argument");
  const bool fc = cfg->preprocess == L2O_PRE_FC_ELU;
  const int P = fc ? kH : (cfg->preprocess == L2O_PRE_LOGSIGN ? 2 : 1);
  return atb_launch(Ac, Bm, (int64_t)T * rows, KA, KB, fc ? 2 : 1, G, workspace, (hipStream_t)stream, rows, P);
}

// ---- generic-`layers` optimizer step (csrc/l2o_generic.h) --------------------------------------------------
static int check_gen_net(const l2o_net_cfg* cfg, const l2o_gen_net* net) {
  if (!cfg || !net) return fail(L2O_ERR_ARG, "generic net: NULL argument");
  if (net->n_layers < 1 || net->n_layers > kGenMaxL)
    return fail(L2O_ERR_UNSUPPORTED, "generic net: 1..%d LSTM layers (got %d)", kGenMaxL, net->n_layers);
  for (int l = 0; l < net->n_layers; ++l) {
    if (net->hidden[l] < 1 || net->hidden[l] > kGenMaxH)
      return fail(L2O_ERR_UNSUPPORTED, "generic net: hidden sizes 1..%d (layer %d has %d)", kGenMaxH, l, net->hidden[l]);
    if (!net->w_gates[l] || !net->b_gates[l]) return fail(L2O_ERR_ARG, "generic net: NULL weights of layer %d", l);
  }
  if (!net->w_lin || !net->b_lin) return fail(L2O_ERR_ARG, "generic net: NULL output Linear");
  const int want = cfg->preprocess == L2O_PRE_FC_ELU ? net->in_dim : (cfg->preprocess == L2O_PRE_LOGSIGN ? 2 : 1);
  if (net->in_dim != want || net->in_dim < 1 || net->in_dim > kGenMaxH)
    return fail(L2O_ERR_ARG, "generic net: in_dim %d does not match the preprocessing (%d)", net->in_dim, want);
  if (cfg->preprocess == L2O_PRE_FC_ELU && (!net->w_fc || !net->b_fc)) return fail(L2O_ERR_ARG, "generic net: fc weights");
  return L2O_OK;
}

size_t l2o_gen_state_floats(const l2o_gen_net* net, int64_t N) {
  if (!net || N <= 0 || net->n_layers < 1 || net->n_layers > kGenMaxL) return 0;
  size_t n = 0;
  for (int l = 0; l < net->n_layers; ++l) n += 2 * (size_t)N * (size_t)net->hidden[l];
  return n;
}

int l2o_cwlstm_step_generic(const l2o_net_cfg* cfg, const l2o_gen_net* net, const float* g, const float* m_tilde, float* m,
                            float* v, double pow1, double pow2, float* state, float* x, int64_t N, void* stream) {
  OptScope opt_scope(cfg_optw(cfg));
  int rc = check_gen_net(cfg, net);
  if (rc) return rc;
  if (!g || !state || !x || N <= 0) return fail(L2O_ERR_ARG, "l2o_cwlstm_step_generic: bad argument");
  const bool fc = cfg->preprocess == L2O_PRE_FC_ELU;
  if (fc && net->direct_inputs && !m_tilde) return fail(L2O_ERR_ARG, "l2o_cwlstm_step_generic: direct inputs need m_tilde");
  if (fc && !net->direct_inputs && (!m || !v)) return fail(L2O_ERR_ARG, "l2o_cwlstm_step_generic: RNNProp needs m and v");
  GenParams p;
  std::memset(&p, 0, sizeof(p));
  p.n_layers = net->n_layers;
  for (int l = 0; l < net->n_layers; ++l) { p.H[l] = net->hidden[l]; p.wg[l] = net->w_gates[l]; p.bg[l] = net->b_gates[l]; }
  p.in_dim = net->in_dim; p.pre = cfg->preprocess; p.direct = net->direct_inputs; p.tanh_output = cfg->tanh_output;
  p.scale = (float)cfg->scale;
  p.k_inv = cfg->logsign_k != 0.0 ? (float)(1.0 / cfg->logsign_k) : 0.0f;
  p.exp_k = (float)std::exp(cfg->logsign_k);
  p.beta1 = (float)cfg->beta1; p.beta2 = (float)cfg->beta2;
  p.omb1 = (float)(1.0 - cfg->beta1); p.omb2 = (float)(1.0 - cfg->beta2);
  p.om1 = (float)(1.0 - pow1); p.om2 = (float)(1.0 - pow2);
  p.wl = net->w_lin; p.bl = net->b_lin; p.wfc = net->w_fc; p.bfc = net->b_fc;
  p.g = g; p.m_in = m_tilde; p.m = m; p.v = v; p.state = state; p.x = x; p.N = (long)N;
  hipLaunchKernelGGL(k_cwlstm_generic, dim3((unsigned)((N + kGenThreads - 1) / kGenThreads)), dim3(kGenThreads), 0,
                     (hipStream_t)stream, p);
  HIP_TRY(hipGetLastError());
  return L2O_OK;
}

int l2o_cwlstm_bwd_step_generic(const l2o_net_cfg* cfg, const l2o_gen_net* net, const l2o_gen_bwd_io* io, double pow1,
                                double pow2, int64_t N, void* stream) {
  OptScope opt_scope(cfg_optw(cfg));
  int rc = check_gen_net(cfg, net);
  if (rc) return rc;
  if (!io || N <= 0 || !io->g || !io->st_prev || !io->dx_next || !io->carry_in || !io->carry_out || !io->tc ||
      !io->h_last || !io->dd)
    return fail(L2O_ERR_ARG, "l2o_cwlstm_bwd_step_generic: bad argument");
  if (net->direct_inputs) return fail(L2O_ERR_UNSUPPORTED, "l2o_cwlstm_bwd_step_generic: direct inputs have no moments to chain through");
  const bool fc = cfg->preprocess == L2O_PRE_FC_ELU;
  if (fc && (!io->m || !io->v || !io->feats || !io->du))
    return fail(L2O_ERR_ARG, "l2o_cwlstm_bwd_step_generic: RNNProp needs m, v, feats and du");
  if (fc && io->dg) return fail(L2O_ERR_UNSUPPORTED, "l2o_cwlstm_bwd_step_generic: the input adjoint of RNNProp is formed by the host from du");
  GenBwdParams p;
  std::memset(&p, 0, sizeof(p));
  p.n_layers = net->n_layers;
  for (int l = 0; l < net->n_layers; ++l) {
    if (!io->act[l] || !io->dz[l]) return fail(L2O_ERR_ARG, "l2o_cwlstm_bwd_step_generic: NULL act / dz of layer %d", l);
    p.H[l] = net->hidden[l]; p.wg[l] = net->w_gates[l]; p.bg[l] = net->b_gates[l];
    p.act[l] = io->act[l]; p.dz[l] = io->dz[l];
  }
  p.in_dim = net->in_dim; p.pre = cfg->preprocess; p.tanh_output = cfg->tanh_output;
  p.scale = (float)cfg->scale;
  p.k_inv = cfg->logsign_k != 0.0 ? (float)(1.0 / cfg->logsign_k) : 0.0f;
  p.exp_k = (float)std::exp(cfg->logsign_k);
  p.om1 = (float)(1.0 - pow1); p.om2 = (float)(1.0 - pow2);
  p.wl = net->w_lin; p.bl = net->b_lin; p.wfc = net->w_fc; p.bfc = net->b_fc;
  p.g = io->g; p.m = io->m; p.v = io->v; p.st_prev = io->st_prev; p.dx_next = io->dx_next;
  p.carry_in = io->carry_in; p.carry_out = io->carry_out; p.tc = io->tc; p.h_last = io->h_last; p.dd = io->dd;
  p.feats = io->feats; p.du = io->du; p.dg = io->dg; p.N = (long)N;
  hipLaunchKernelGGL(k_cwlstm_generic_bwd, dim3((unsigned)((N + kGenThreads - 1) / kGenThreads)), dim3(kGenThreads), 0,
                     (hipStream_t)stream, p);
  HIP_TRY(hipGetLastError());
  return L2O_OK;
}

// ---- the fused persistent unroll of the MLP optimizee (csrc/l2o_mlp_unroll.h) ---------------------------
struct MlpUnrollLayout { int n[4], tile_begin[5], nwg, nw1, R, hier_R1; bool fast; size_t NO, NSM, p_off, s_off, sm_off, hs_off, x_off, s1_off, total; };
static bool mlp_unroll_layout(const l2o_mlp* mlp, MlpUnrollLayout* L) {
  if (!mlp) return false;
  const int H = mlp->n_hidden, O = mlp->n_out;
  if (H < kMuMinH || H > kMuMaxH || O < 1 || O > kMuMaxO || mlp->batch < 1 || mlp->batch > kMuMaxBatch || mlp->n_in < 1)
    return false;
  L->n[0] = mlp->n_in * H; L->n[1] = H; L->n[2] = H * O; L->n[3] = O;
  if (L->n[0] % 64) return false;                        // the w1 coordinates fill whole workgroups
  L->tile_begin[0] = 0;
  for (int v = 0; v < 4; ++v) L->tile_begin[v + 1] = L->tile_begin[v] + tiles_per_problem(L->n[v]);
  L->nwg = (L->tile_begin[4] + 3) / 4;
  L->nw1 = L->n[0] / 64;
  L->NO = (size_t)mlp->batch * H;
  L->NSM = (size_t)H + (size_t)H * O + O;
  L->R = (int)((L->NO + L->nwg - 1) / L->nwg);
  L->R = (L->R + 1) & ~1;                                // even: the fast path moves granules in pairs
  // one 64-byte line per (source, reducer): R = 8 measured best (profiles/archive_r01_r03/r02l: R = 6 / 8 / 12 / 16 -> 1.32 / 1.35 /
  // 1.28 / 1.24 G on config 5)
  if (L->R < 8 && L->NO >= 8 * 32) L->R = 8;
  if (L->R > kMuMaxR) return false;
  L->fast = H == 20 && O == 10 && mlp->batch == 64;
  L->p_off = sizeof(MlpWs);
  // XCD-hierarchical all-reduce (fast path; l2o_mlp_unroll.h): group g = wg % 8, every group needs enough w1 owners to
  // reduce all NO outputs in slices of R1 (even) <= kMuHierR1Max
  L->hier_R1 = 0;
  if (L->fast && opt(L2O_OPT_MLP_HIER) && L->nwg <= 256 && L->nw1 >= 2 * kMuHierG && (L->nwg + kMuHierG - 1) / kMuHierG <= kMuHierM) {
    const int min_cnt = L->nw1 / kMuHierG;                 // the smallest group
    int r1 = (int)((L->NO + min_cnt - 1) / min_cnt);
    r1 = (r1 + 1) & ~1;
    if (r1 <= kMuHierR1Max) L->hier_R1 = r1;
  }
  // P: generic [nw1][NO]; fast path: one inbox per reducing workgroup, [nwg][nw1][R]; hierarchical: [8][M][M][R1]
  const size_t pg = (size_t)L->nw1 * L->NO, pf = (size_t)L->nwg * L->nw1 * L->R;
  const size_t ph = L->hier_R1 ? (size_t)kMuHierG * kMuHierM * kMuHierM * L->hier_R1 : 0;
  size_t pmax = pg > pf ? pg : pf;
  if (ph > pmax) pmax = ph;
  L->s_off = L->p_off + sizeof(unsigned long long) * pmax;
  L->sm_off = L->s_off + sizeof(unsigned long long) * 2 * L->NO;
  L->hs_off = L->sm_off + sizeof(unsigned long long) * 2 * ((L->NSM + 1) & ~(size_t)1);
  L->x_off = L->hs_off + sizeof(unsigned long long) * 256;
  L->s1_off = L->x_off + sizeof(unsigned long long) * 2 * kMuHierG * kMuHierM * kMuHierR1Max;
  L->total = L->s1_off + sizeof(unsigned long long) * 2 * kMuHierG * kMuHierS;
  return true;
}

int l2o_mlp_unroll_supported(const l2o_net_cfg* cfg, const l2o_mlp* mlp, void* stream) {
  OptScope opt_scope(cfg_optw(cfg));
  MlpUnrollLayout L;
  if (!cfg || !net_ok_for_mfma(cfg) || !opt(L2O_OPT_MLP_UNROLL) || !mlp_unroll_layout(mlp, &L)) return 0;
  if (L.nwg > coresident_cus((hipStream_t)stream)) return 0;     // one workgroup per CU, all co-resident
  return L.fast ? 2 : 1;                                           // 2: the reference's shape (static loop bounds, paired granules)
}

size_t l2o_mlp_unroll_workspace_bytes(const l2o_mlp* mlp) {
  MlpUnrollLayout L;
  return mlp_unroll_layout(mlp, &L) ? L.total : 0;
}

static int mlp_unroll_launch(const l2o_net_cfg* cfg, const float* wpack, const l2o_mlp* mlp, const int32_t* indices,
                             float* const* x, float* const* st, float* const* m, float* const* v,
                             const float* const* x_scale, int32_t T, int32_t step0, float* fx, const l2o_mlp_hist* hist,
                             void* workspace, void* stream) {
  OptScope opt_scope(cfg_optw(cfg));
  if (!cfg || !wpack || !mlp || !indices || !x || !st || !fx || !workspace || T < 0 || !mlp->images || !mlp->labels)
    return fail(L2O_ERR_ARG, "l2o_mlp_unroll: bad argument");
  hipStream_t s = (hipStream_t)stream;
  MlpUnrollLayout L;
  if (!net_ok_for_mfma(cfg) || !mlp_unroll_layout(mlp, &L) || L.nwg > coresident_cus(s))
    return fail(L2O_ERR_UNSUPPORTED, "l2o_mlp_unroll: no fused kernel for n_in=%d hidden=%d out=%d batch=%d net(layers=%d)",
                mlp->n_in, mlp->n_hidden, mlp->n_out, mlp->batch, cfg->n_layers);
  const bool rn = cfg->preprocess == L2O_PRE_FC_ELU;
  MlpUnrollArgs a;
  std::memset(&a, 0, sizeof(a));
  a.np = make_net_params(cfg, wpack);
  a.n_in = mlp->n_in; a.H = mlp->n_hidden; a.O = mlp->n_out; a.batch = mlp->batch; a.act = mlp->activation;
  a.images = mlp->images; a.labels = mlp->labels; a.idx = indices;
  for (int k = 0; k < 4; ++k) {
    if (!x[k] || !st[k] || (rn && (!m || !v || !m[k] || !v[k]))) return fail(L2O_ERR_ARG, "l2o_mlp_unroll: NULL buffer of variable %d", k);
    a.x[k] = x[k]; a.st[k] = st[k]; a.m[k] = rn ? m[k] : nullptr; a.v[k] = rn ? v[k] : nullptr;
    a.xscale[k] = x_scale ? x_scale[k] : nullptr;
    a.n[k] = L.n[k];
  }
  for (int k = 0; k < 5; ++k) a.tile_begin[k] = L.tile_begin[k];
  a.T = T;
  pow_ff(cfg->beta1, step0, &a.p1_hi, &a.p1_lo);
  pow_ff(cfg->beta2, step0, &a.p2_hi, &a.p2_lo);
  a.fx = fx;
  char* wsb = static_cast<char*>(workspace);
  a.ws = reinterpret_cast<MlpWs*>(wsb);
  a.P = reinterpret_cast<unsigned long long*>(wsb + L.p_off);
  a.S = reinterpret_cast<unsigned long long*>(wsb + L.s_off);
  a.Sm = reinterpret_cast<unsigned long long*>(wsb + L.sm_off);
  a.nwg = L.nwg; a.nw1 = L.nw1; a.R = L.R;
  a.hier_R1 = L.hier_R1;
  a.HS = reinterpret_cast<unsigned long long*>(wsb + L.hs_off);
  a.X = reinterpret_cast<unsigned long long*>(wsb + L.x_off);
  a.S1 = reinterpret_cast<unsigned long long*>(wsb + L.s1_off);
  a.use_salt = T + 1 < 0xffff ? 1u : 0u;
  if (hist) {
    for (int k = 0; k < 4; ++k) {
      if (!hist->st[k] || !hist->g[k] || (rn && (!hist->m[k] || !hist->v[k])))
        return fail(L2O_ERR_ARG, "l2o_mlp_unroll_record: NULL history buffer of variable %d", k);
      a.hist_st[k] = hist->st[k]; a.hist_g[k] = hist->g[k];
      a.hist_m[k] = rn ? hist->m[k] : nullptr; a.hist_v[k] = rn ? hist->v[k] : nullptr;
    }
  }
  HIP_TRY(hipMemsetAsync(wsb + L.p_off, 0, L.total - L.p_off, s));   // the granules only: the header survives
  const dim3 grid(L.nwg), block(256);
  void (*fn)(MlpUnrollArgs) = with_pre(cfg->preprocess, [&](auto pre) -> void (*)(MlpUnrollArgs) {
    constexpr int PRE = decltype(pre)::value;
    if (hist) return L.fast ? k_mlp_unroll<PRE, true, true> : k_mlp_unroll<PRE, false, true>;
    return L.fast ? k_mlp_unroll<PRE, true> : k_mlp_unroll<PRE, false>;
  });
  hipLaunchKernelGGL(fn, grid, block, 0, s, a);
  HIP_TRY(hipGetLastError());
  note_form(!L.fast ? L2O_FORM_MLP_UNROLL_GENERIC : (a.hier_R1 ? L2O_FORM_MLP_UNROLL_HIER : L2O_FORM_MLP_UNROLL));
  return L2O_OK;
}

int l2o_mlp_unroll(const l2o_net_cfg* cfg, const float* wpack, const l2o_mlp* mlp, const int32_t* indices,
                   float* const* x, float* const* st, float* const* m, float* const* v, const float* const* x_scale,
                   int32_t T, int32_t step0, float* fx, void* workspace, void* stream) {
  return mlp_unroll_launch(cfg, wpack, mlp, indices, x, st, m, v, x_scale, T, step0, fx, nullptr, workspace, stream);
}
int l2o_mlp_unroll_record(const l2o_net_cfg* cfg, const float* wpack, const l2o_mlp* mlp, const int32_t* indices,
                          float* const* x, float* const* st, float* const* m, float* const* v,
                          const float* const* x_scale, int32_t T, int32_t step0, float* fx, const l2o_mlp_hist* hist,
                          void* workspace, void* stream) {
  if (!hist) return fail(L2O_ERR_ARG, "l2o_mlp_unroll_record: NULL hist");
  return mlp_unroll_launch(cfg, wpack, mlp, indices, x, st, m, v, x_scale, T, step0, fx, hist, workspace, stream);
}

// ---- problems.mnist with several hidden layers (csrc/l2o_mlp_deep.h) ---------------------------------------------------
static bool mlp_deep_ok(const l2o_mlp_deep* m) {
  if (!m || m->n_hidden_layers < 1 || m->n_hidden_layers > kMdMaxHidden || m->n_in < 1 || m->n_in > kMdMaxIn) return false;
  if (m->n_out < 1 || m->n_out > kMdMaxOut || m->batch < 1 || m->batch > 4096) return false;
  for (int l = 0; l < m->n_hidden_layers; ++l)
    if (m->hidden[l] < 1 || m->hidden[l] > kMdMaxWidth) return false;
  return true;
}
size_t l2o_mlp_deep_scratch_floats(const l2o_mlp_deep* m) {
  if (!mlp_deep_ok(m)) return 0;
  return (size_t)m->batch * kMdMaxWidth * (2 * m->n_hidden_layers + 1) + m->batch;
}
int l2o_mlp_deep_fg(const l2o_mlp_deep* m, const int32_t* indices, const float* const* w, float* loss, float* const* g,
                    float* scratch, void* stream) {
  if (!mlp_deep_ok(m))
    return fail(L2O_ERR_UNSUPPORTED, "l2o_mlp_deep_fg: 1-3 hidden layers of <= 32 units, n_in <= 1024, n_out <= 16, batch <= 4096");
  if (!indices || !w || !loss || !scratch || !m->images || !m->labels) return fail(L2O_ERR_ARG, "l2o_mlp_deep_fg: NULL argument");
  MlpDeepArgs a;
  std::memset(&a, 0, sizeof(a));
  a.n_in = m->n_in; a.n_out = m->n_out; a.batch = m->batch; a.act = m->activation; a.nh = m->n_hidden_layers;
  for (int l = 0; l < a.nh; ++l) a.width[l] = m->hidden[l];
  a.width[a.nh] = m->n_out;
  a.images = m->images; a.labels = m->labels; a.idx = indices;
  long ncoord = 0;
  for (int l = 0; l <= a.nh; ++l) {
    if (!w[2 * l] || !w[2 * l + 1] || (g && (!g[2 * l] || !g[2 * l + 1]))) return fail(L2O_ERR_ARG, "l2o_mlp_deep_fg: NULL buffer of layer %d", l);
    a.w[l] = w[2 * l]; a.b[l] = w[2 * l + 1];
    if (g) { a.gw[l] = g[2 * l]; a.gb[l] = g[2 * l + 1]; }
    ncoord += (long)(l == 0 ? a.n_in : a.width[l - 1]) * a.width[l] + a.width[l];
  }
  a.acts = scratch;
  a.deltas = a.acts + (size_t)a.nh * a.batch * kMdMaxWidth;
  a.loss_s = a.deltas + (size_t)(a.nh + 1) * a.batch * kMdMaxWidth;
  a.loss = loss;
  a.want_grad = g ? 1 : 0;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_mlp_deep_sample, dim3(a.batch), dim3(kMdThreads), 0, s, a);
  const long nthreads = g ? ncoord : 1;
  hipLaunchKernelGGL(k_mlp_deep_grad, dim3((unsigned)((nthreads + kMdThreads - 1) / kMdThreads)), dim3(kMdThreads), 0, s, a);
  HIP_TRY(hipGetLastError());
  return L2O_OK;
}

// ---- second derivatives of problems.mnist: the Hessian-vector product (csrc/l2o_mlp_hvp.h, include/l2o_mlp_hvp_abi.h) ------
size_t l2o_mlp_hvp_scratch_floats(const l2o_mlp_deep* m) {
  if (!mlp_deep_ok(m)) return 0;
  return (size_t)m->batch * kMdMaxWidth * (4 * m->n_hidden_layers + 2);
}
int l2o_mlp_hvp(const l2o_mlp_deep* m, const int32_t* indices, const float* const* w, const float* const* u, float* const* out,
                float* scratch, void* stream) {
  if (!mlp_deep_ok(m))
    return fail(L2O_ERR_UNSUPPORTED, "l2o_mlp_hvp: 1-3 hidden layers of <= 32 units, n_in <= 1024, n_out <= 16, batch <= 4096");
  if (m->activation != 0 && m->activation != 1) return fail(L2O_ERR_UNSUPPORTED, "l2o_mlp_hvp: activation 0 (sigmoid) or 1 (relu)");
  if (!indices || !w || !u || !out || !scratch || !m->images || !m->labels) return fail(L2O_ERR_ARG, "l2o_mlp_hvp: NULL argument");
  MlpHvpArgs a;
  std::memset(&a, 0, sizeof(a));
  a.n_in = m->n_in; a.n_out = m->n_out; a.batch = m->batch; a.act = m->activation; a.nh = m->n_hidden_layers;
  for (int l = 0; l < a.nh; ++l) a.width[l] = m->hidden[l];
  a.width[a.nh] = m->n_out;
  a.images = m->images; a.labels = m->labels; a.idx = indices;
  long ncoord = 0;
  for (int l = 0; l <= a.nh; ++l) {
    for (int q = 2 * l; q < 2 * l + 2; ++q)
      if (!w[q] || !u[q] || !out[q]) return fail(L2O_ERR_ARG, "l2o_mlp_hvp: NULL buffer of layer %d", l);
    a.w[l] = w[2 * l]; a.b[l] = w[2 * l + 1];
    a.vw[l] = u[2 * l]; a.vb[l] = u[2 * l + 1];
    a.ow[l] = out[2 * l]; a.ob[l] = out[2 * l + 1];
    ncoord += (long)(l == 0 ? a.n_in : a.width[l - 1]) * a.width[l] + a.width[l];
  }
  const size_t per = (size_t)a.batch * kMdMaxWidth;
  a.acts = scratch;
  a.racts = a.acts + (size_t)a.nh * per;
  a.deltas = a.racts + (size_t)a.nh * per;
  a.rdeltas = a.deltas + (size_t)(a.nh + 1) * per;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_mlp_hvp_sample, dim3(a.batch), dim3(kMdThreads), 0, s, a);
  hipLaunchKernelGGL(k_mlp_hvp_reduce, dim3((unsigned)((ncoord + kMdThreads - 1) / kMdThreads)), dim3(kMdThreads), 0, s, a);
  HIP_TRY(hipGetLastError());
  return L2O_OK;
}

// ---- problems.mnist_conv (csrc/l2o_mnist_conv.h) ----------------------------------------------------------------------
static bool mnist_conv_ok(const l2o_mnist_conv* m) {
  return m && m->batch >= 2 && m->batch <= kCvMaxBatch && m->n_data >= 1 && (m->batch_norm == 0 || m->batch_norm == 1);
}
static size_t mnist_conv_per_sample() {
  return (size_t)2 * kCvZ1 + 2 * kCvA1 + 2 * kCvZ2 + kCvNF + 16 + 1 + 2 * kCvC1 * 2 + 2 * kCvC2 * 2 + kCvPW2 + kCvPW1;
}
size_t l2o_mnist_conv_scratch_floats(const l2o_mnist_conv* m) {
  if (!mnist_conv_ok(m)) return 0;
  return (size_t)m->batch * mnist_conv_per_sample() + 2 * (kCvC1 + kCvC2);
}
int l2o_mnist_conv_fg(const l2o_mnist_conv* m, const int32_t* indices, const float* const* w, float* loss, float* const* g,
                      float* scratch, void* stream) {
  if (!mnist_conv_ok(m))
    return fail(L2O_ERR_UNSUPPORTED, "l2o_mnist_conv_fg: batch in [2, %d], batch_norm 0 or 1, n_data >= 1", kCvMaxBatch);
  if (!indices || !w || !loss || !scratch || !m->images || !m->labels) return fail(L2O_ERR_ARG, "l2o_mnist_conv_fg: NULL argument");
  const int bn = m->batch_norm, nv = bn ? 10 : 6;
  for (int k = 0; k < nv; ++k)
    if (!w[k] || (g && !g[k])) return fail(L2O_ERR_ARG, "l2o_mnist_conv_fg: NULL buffer of variable %d", k);
  MnistConvArgs a;
  std::memset(&a, 0, sizeof(a));
  a.batch = m->batch; a.bn = bn; a.want_grad = g ? 1 : 0;
  a.images = m->images; a.labels = m->labels; a.idx = indices;
  // variable order of the reference's graph: conv_layer1/{weights1, biases1}, [batch_normalization/{gamma, beta}],
  // conv_layer2/{weights1, biases1}, [batch_normalization_1/{gamma, beta}], fc_weights, fc_bias
  const int k2 = bn ? 4 : 2, kf = bn ? 8 : 4;
  a.w1 = w[0]; a.b1 = w[1]; a.w2 = w[k2]; a.b2 = w[k2 + 1]; a.wf = w[kf]; a.bf = w[kf + 1];
  if (bn) { a.g1 = w[2]; a.be1 = w[3]; a.g2 = w[6]; a.be2 = w[7]; }
  if (g) {
    a.gw1 = g[0]; a.gb1 = g[1]; a.gw2 = g[k2]; a.gb2 = g[k2 + 1]; a.gwf = g[kf]; a.gbf = g[kf + 1];
    if (bn) { a.gg1 = g[2]; a.gbe1 = g[3]; a.gg2 = g[6]; a.gbe2 = g[7]; }
  }
  const size_t B = (size_t)a.batch;
  float* p = scratch;
  a.z1 = p; p += B * kCvZ1;
  a.d1 = p; p += B * kCvZ1;
  a.p1 = p; p += B * kCvA1;
  a.am1 = reinterpret_cast<int*>(p); p += B * kCvA1;
  a.z2 = p; p += B * kCvZ2;
  a.d2 = p; p += B * kCvZ2;
  a.f = p; p += B * kCvNF;
  a.dlog = p; p += B * 16;
  a.loss_s = p; p += B;
  a.st1 = p; p += B * kCvC1 * 2;
  a.bw1 = p; p += B * kCvC1 * 2;
  a.st2 = p; p += B * kCvC2 * 2;
  a.bw2 = p; p += B * kCvC2 * 2;
  a.pw2 = p; p += B * kCvPW2;
  a.pw1 = p; p += B * kCvPW1;
  a.stat = p;
  a.loss = loss;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(a.batch), blk(kCvThreads);
  hipLaunchKernelGGL(k_cv_conv1, grid, blk, 0, s, a);
  hipLaunchKernelGGL(k_cv_conv2, grid, blk, 0, s, a);
  hipLaunchKernelGGL(k_cv_head, grid, blk, 0, s, a);
  if (g) {
    hipLaunchKernelGGL(k_cv_mid, grid, blk, 0, s, a);
    hipLaunchKernelGGL(k_cv_first, grid, blk, 0, s, a);
  }
  const long nthreads = g ? kCvGradThreads : 1;
  hipLaunchKernelGGL(k_cv_grad, dim3((unsigned)((nthreads + kCvThreads - 1) / kCvThreads)), blk, 0, s, a);
  HIP_TRY(hipGetLastError());
  return L2O_OK;
}

// ---- problems.cifar10 (csrc/l2o_cifar_conv.h) -------------------------------------------------------------------------
static bool cifar_conv_ok(const l2o_cifar_conv* m) {
  return m && m->batch >= 2 && m->batch <= kCcMaxBatch && m->n_data >= 1 && (m->batch_norm == 0 || m->batch_norm == 1);
}
static size_t cifar_conv_per_sample() {
  return (size_t)2 * kCcZ1 + 2 * kCcA1 + 3 * kCcZ2 + kCcNF + 16 + 1 + 2 * kCcC1 * 2 + 2 * kCcC2 * 2 + kCcPW1;
}
size_t l2o_cifar_conv_scratch_floats(const l2o_cifar_conv* m) {
  if (!cifar_conv_ok(m)) return 0;
  return (size_t)m->batch * cifar_conv_per_sample() + 2 * (kCcC1 + kCcC2);
}
int l2o_cifar_conv_fg(const l2o_cifar_conv* m, const int32_t* indices, const float* const* w, float* loss, float* const* g,
                      float* scratch, void* stream) {
  if (!cifar_conv_ok(m))
    return fail(L2O_ERR_UNSUPPORTED, "l2o_cifar_conv_fg: batch in [2, %d], batch_norm 0 or 1, n_data >= 1", kCcMaxBatch);
  if (!indices || !w || !loss || !scratch || !m->images || !m->labels) return fail(L2O_ERR_ARG, "l2o_cifar_conv_fg: NULL argument");
  const int bn = m->batch_norm, nv = bn ? 10 : 6;
  for (int k = 0; k < nv; ++k)
    if (!w[k] || (g && !g[k])) return fail(L2O_ERR_ARG, "l2o_cifar_conv_fg: NULL buffer of variable %d", k);
  CifarConvArgs a;
  std::memset(&a, 0, sizeof(a));
  a.batch = m->batch; a.bn = bn; a.want_grad = g ? 1 : 0;
  a.images = m->images; a.labels = m->labels; a.idx = indices;
  // variable order of the reference's graph: conv_layer1/{weights1, biases1}, [batch_normalization/{gamma, beta}],
  // conv_layer2/{weights1, biases1}, [batch_normalization_1/{gamma, beta}], fc_weights, fc_bias
  const int k2 = bn ? 4 : 2, kf = bn ? 8 : 4;
  a.w1 = w[0]; a.b1 = w[1]; a.w2 = w[k2]; a.b2 = w[k2 + 1]; a.wf = w[kf]; a.bf = w[kf + 1];
  if (bn) { a.g1 = w[2]; a.be1 = w[3]; a.g2 = w[6]; a.be2 = w[7]; }
  if (g) {
    a.gw1 = g[0]; a.gb1 = g[1]; a.gw2 = g[k2]; a.gb2 = g[k2 + 1]; a.gwf = g[kf]; a.gbf = g[kf + 1];
    if (bn) { a.gg1 = g[2]; a.gbe1 = g[3]; a.gg2 = g[6]; a.gbe2 = g[7]; }
  }
  const size_t B = (size_t)a.batch;
  float* p = scratch;
  a.z1 = p; p += B * kCcZ1;
  a.d1 = p; p += B * kCcZ1;
  a.p1 = p; p += B * kCcA1;
  a.am1 = reinterpret_cast<int*>(p); p += B * kCcA1;
  a.z2 = p; p += B * kCcZ2;
  a.d2 = p; p += B * kCcZ2;
  a.dz2 = p; p += B * kCcZ2;
  a.f = p; p += B * kCcNF;
  a.dlog = p; p += B * 16;
  a.loss_s = p; p += B;
  a.st1 = p; p += B * kCcC1 * 2;
  a.bw1 = p; p += B * kCcC1 * 2;
  a.st2 = p; p += B * kCcC2 * 2;
  a.bw2 = p; p += B * kCcC2 * 2;
  a.pw1 = p; p += B * kCcPW1;
  a.stat = p;
  a.loss = loss;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(a.batch), blk(kCcThreads);
  hipLaunchKernelGGL(k_cc_conv1, grid, blk, 0, s, a);
  hipLaunchKernelGGL(k_cc_conv2, grid, blk, 0, s, a);
  hipLaunchKernelGGL(k_cc_head, dim3((a.batch + kCcHeadSamples - 1) / kCcHeadSamples), blk, 0, s, a);
  if (g) {
    hipLaunchKernelGGL(k_cc_mid, grid, blk, 0, s, a);
    hipLaunchKernelGGL(k_cc_first, grid, blk, 0, s, a);
  }
  const long nthreads = g ? kCcGradThreads : 1;
  const unsigned nblocks = (unsigned)((nthreads + kCcThreads - 1) / kCcThreads) + (g ? kCcW2Blocks : 0);
  hipLaunchKernelGGL(k_cc_grad, dim3(nblocks), blk, 0, s, a);
  HIP_TRY(hipGetLastError());
  return L2O_OK;
}

// ---- problems.LeNet (csrc/l2o_lenet.h) --------------------------------------------------------------------------------
static bool lenet_ok(const l2o_lenet* m) {
  return m && m->batch >= 2 && m->batch <= kLnMaxBatch && m->n_data >= 1 && (m->batch_norm == 0 || m->batch_norm == 1);
}
// every per-sample region is a multiple of 4 floats (the kernels read some of them as float4); loss_s and stat come last
static size_t lenet_per_sample() {
  return (size_t)2 * kLnZ1 + 2 * kLnA1 + 2 * kLnZ2 + 2 * kLnF + 3 * kLnN1 + 3 * kLnN2 + 16 + 2 * kLnC1 * 2 + 2 * kLnC2 * 2 +
         kLnPW1 + kLnPW2 + 1;
}
size_t l2o_lenet_scratch_floats(const l2o_lenet* m) {
  if (!lenet_ok(m)) return 0;
  return (size_t)m->batch * lenet_per_sample() + kLnStat;
}
int l2o_lenet_fg(const l2o_lenet* m, const int32_t* indices, const float* const* w, float* loss, float* const* g,
                 float* scratch, void* stream) {
  if (!lenet_ok(m))
    return fail(L2O_ERR_UNSUPPORTED, "l2o_lenet_fg: batch in [2, %d], batch_norm 0 or 1, n_data >= 1", kLnMaxBatch);
  if (!indices || !w || !loss || !scratch || !m->images || !m->labels) return fail(L2O_ERR_ARG, "l2o_lenet_fg: NULL argument");
  if ((uintptr_t)scratch & 15) return fail(L2O_ERR_ARG, "l2o_lenet_fg: scratch must be 16-byte aligned");
  const int bn = m->batch_norm, nv = bn ? 14 : 10;
  for (int k = 0; k < nv; ++k)
    if (!w[k] || (g && !g[k])) return fail(L2O_ERR_ARG, "l2o_lenet_fg: NULL buffer of variable %d", k);
  LenetArgs a;
  std::memset(&a, 0, sizeof(a));
  a.batch = m->batch; a.bn = bn; a.want_grad = g ? 1 : 0;
  a.images = m->images; a.labels = m->labels; a.idx = indices;
  // variable order of the reference's graph: conv_2d_0/{w, b}, [batch_norm_0/beta], conv_2d_1/{w, b}, [batch_norm_1/beta],
  // linear_0/{w, b}, [mlp/batch_norm/beta], linear_1/{w, b}, [mlp/batch_norm_1/beta], linear_2/{w, b}
  const int st = bn ? 3 : 2, k2 = st, k3 = 2 * st, k4 = 3 * st, k5 = 4 * st;
  a.w1 = w[0]; a.b1 = w[1]; a.w2 = w[k2]; a.b2 = w[k2 + 1]; a.wl0 = w[k3]; a.bl0 = w[k3 + 1]; a.wl1 = w[k4]; a.bl1 = w[k4 + 1];
  a.wl2 = w[k5]; a.bl2 = w[k5 + 1];
  if (bn) { a.be1 = w[2]; a.be2 = w[5]; a.bel0 = w[8]; a.bel1 = w[11]; }
  if (g) {
    a.gw1 = g[0]; a.gb1 = g[1]; a.gw2 = g[k2]; a.gb2 = g[k2 + 1]; a.gwl0 = g[k3]; a.gbl0 = g[k3 + 1]; a.gwl1 = g[k4];
    a.gbl1 = g[k4 + 1]; a.gwl2 = g[k5]; a.gbl2 = g[k5 + 1];
    if (bn) { a.gbe1 = g[2]; a.gbe2 = g[5]; a.gbel0 = g[8]; a.gbel1 = g[11]; }
  }
  const size_t B = (size_t)a.batch;
  float* p = scratch;
  a.z1 = p; p += B * kLnZ1;
  a.d1 = p; p += B * kLnZ1;
  a.p1 = p; p += B * kLnA1;
  a.am1 = reinterpret_cast<int*>(p); p += B * kLnA1;
  a.z2 = p; p += B * kLnZ2;
  a.d2 = p; p += B * kLnZ2;
  a.f = p; p += B * kLnF;
  a.am2 = reinterpret_cast<int*>(p); p += B * kLnF;
  a.h1 = p; p += B * kLnN1;
  a.a1 = p; p += B * kLnN1;
  a.dh1 = p; p += B * kLnN1;
  a.h2 = p; p += B * kLnN2;
  a.a2 = p; p += B * kLnN2;
  a.dh2 = p; p += B * kLnN2;
  a.dlog = p; p += B * 16;
  a.st1 = p; p += B * kLnC1 * 2;
  a.bw1 = p; p += B * kLnC1 * 2;
  a.st2 = p; p += B * kLnC2 * 2;
  a.bw2 = p; p += B * kLnC2 * 2;
  a.pw1 = p; p += B * kLnPW1;
  a.pw2 = p; p += B * kLnPW2;
  a.loss_s = p; p += B;
  a.stat = p;
  a.loss = loss;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(a.batch), blk(kLnThreads);
  hipLaunchKernelGGL(k_ln_conv1, grid, blk, 0, s, a);
  hipLaunchKernelGGL(k_ln_conv2, grid, blk, 0, s, a);
  hipLaunchKernelGGL(k_ln_pool2, grid, blk, 0, s, a);
  hipLaunchKernelGGL(k_ln_fc<0>, dim3(kLnN1 / kLnU), blk, 0, s, a);
  hipLaunchKernelGGL(k_ln_fc<1>, dim3(kLnN2 / kLnU), blk, 0, s, a);
  hipLaunchKernelGGL(k_ln_out, dim3((a.batch + kLnOutSamples - 1) / kLnOutSamples), blk, 0, s, a);
  if (g) {
    hipLaunchKernelGGL(k_ln_fcb<1>, dim3(kLnN2 / kLnU), blk, 0, s, a);
    hipLaunchKernelGGL(k_ln_fcb<0>, dim3(kLnN1 / kLnU), blk, 0, s, a);
    hipLaunchKernelGGL(k_ln_mid, grid, blk, 0, s, a);
    hipLaunchKernelGGL(k_ln_mid2, grid, blk, 0, s, a);
    hipLaunchKernelGGL(k_ln_first, grid, blk, 0, s, a);
  }
  const long nthreads = g ? kLnGradThreads : 1;
  hipLaunchKernelGGL(k_ln_grad, dim3((unsigned)((nthreads + kLnThreads - 1) / kLnThreads)), blk, 0, s, a);
  HIP_TRY(hipGetLastError());
  return L2O_OK;
}

// ---- problems.vgg16_cifar10 (csrc/l2o_vgg16.h, include/l2o_vgg16_abi.h) -------------------------------------------------
static bool vgg16_ok(const l2o_vgg16* m) {
  if (!m || m->batch < 2 || m->batch > kVgMaxBatch || m->n_data < 1) return false;
  for (int b = 0; b < 5; ++b)
    if (m->channels[b] < 8 || m->channels[b] > 512 || m->channels[b] % 8) return false;
  return true;
}
// The scratch of one call, in floats from its start: the gathered images, the output of every conv layer and of pools 1-4,
// pool 5's output, dz, the per-sample losses, two gradient buffers of the largest activation and the weight-gradient
// partials.  Every size is a multiple of 4 floats.
struct VgScratch {
  size_t x0, act[kVgLayers], pool[4], pooled, dz, loss_s, grad[2], part, total;
};
static VgScratch vgg16_scratch(const l2o_vgg16* m, const VgLayer* L) {
  VgScratch s;
  const size_t B = (size_t)m->batch;
  size_t p = 0, gmax = 0, pmax = 0;
  auto take = [&](size_t n) { const size_t at = p; p += (n + 3) & ~(size_t)3; return at; };
  s.x0 = take(B * 3072);
  int np = 0;
  for (int l = 0; l < kVgLayers; ++l) {
    const size_t n = (B << (2 * L[l].lw)) * L[l].cout;
    s.act[l] = take(n);
    if (L[l].pool && l != kVgLayers - 1) s.pool[np++] = take(n / 4);
    if (n > gmax) gmax = n;
    int per;
    const size_t pn = (size_t)vg_wgrad_splits(m->batch, L[l], &per) * (9 * L[l].cin + 1) * L[l].cout;
    if (pn > pmax) pmax = pn;
  }
  s.pooled = take(B * m->channels[4]);
  s.dz = take(B * 16);
  s.loss_s = take(B);
  s.grad[0] = take(gmax);
  s.grad[1] = take(gmax);
  s.part = take(pmax);
  s.total = p;
  return s;
}
size_t l2o_vgg16_scratch_floats(const l2o_vgg16* m) {
  if (!vgg16_ok(m)) return 0;
  VgLayer L[kVgLayers];
  vg_plan(m->channels, L);
  return vgg16_scratch(m, L).total;
}
int l2o_vgg16_fg(const l2o_vgg16* m, const int32_t* indices, const float* const* w, float* loss, float* const* g,
                 float* scratch, void* stream) {
  if (!vgg16_ok(m))
    return fail(L2O_ERR_UNSUPPORTED, "l2o_vgg16_fg: batch in [2, %d], channels multiples of 8 in [8, 512], n_data >= 1",
                kVgMaxBatch);
  if (!indices || !w || !loss || !scratch || !m->images || !m->labels) return fail(L2O_ERR_ARG, "l2o_vgg16_fg: NULL argument");
  if ((uintptr_t)scratch & 15) return fail(L2O_ERR_ARG, "l2o_vgg16_fg: scratch must be 16-byte aligned");
  for (int k = 0; k < L2O_VGG16_VARS; ++k)
    if (!w[k] || (g && !g[k])) return fail(L2O_ERR_ARG, "l2o_vgg16_fg: NULL buffer of variable %d", k);
  VgLayer L[kVgLayers];
  vg_plan(m->channels, L);
  const VgScratch sc = vgg16_scratch(m, L);
  hipStream_t s = (hipStream_t)stream;
  const int B = m->batch;
  const dim3 blk(kVgThreads);
  auto blocks = [](size_t n) { return dim3((unsigned)((n + kVgThreads - 1) / kVgThreads)); };
  auto tiles = [](int n, int t) { return (unsigned)((n + t - 1) / t); };
  // ---- forward
  hipLaunchKernelGGL(k_vg_gather, dim3(B), blk, 0, s, m->images, indices, m->n_data, scratch + sc.x0);
  const float* in[kVgLayers];                  // the input of every conv layer
  const float* x = scratch + sc.x0;
  int np = 0;
  for (int l = 0; l < kVgLayers; ++l) {
    const int M = B << (2 * L[l].lw);
    in[l] = x;
    VgGemm a{x, w[2 * l], w[2 * l + 1], scratch + sc.act[l], M, L[l].lw, L[l].cin, L[l].cout, 0};
    hipLaunchKernelGGL(k_vg_gemm<VG_FWD>, dim3(tiles(M, kVgBM), tiles(L[l].cout, kVgBN)), blk, 0, s, a);
    x = scratch + sc.act[l];
    if (L[l].pool && l != kVgLayers - 1) {
      const size_t total = (size_t)(M / 4) * L[l].cout;
      hipLaunchKernelGGL(k_vg_pool, blocks(total), blk, 0, s, x, scratch + sc.pool[np], L[l].lw, L[l].cout, total);
      x = scratch + sc.pool[np++];
    }
  }
  float* dy = scratch + sc.grad[0];            // gradient w.r.t. the pre-activation of the layer in hand
  float* other = scratch + sc.grad[1];
  VgHead h;
  std::memset(&h, 0, sizeof(h));
  h.a13 = scratch + sc.act[kVgLayers - 1]; h.wfc = w[26]; h.bfc = w[27]; h.labels = m->labels; h.idx = indices;
  h.pooled = scratch + sc.pooled; h.dz = scratch + sc.dz; h.loss_s = scratch + sc.loss_s; h.dy13 = g ? dy : nullptr;
  h.loss = loss; h.gwfc = g ? g[26] : nullptr; h.gbfc = g ? g[27] : nullptr;
  h.B = B; h.C = m->channels[4]; h.n_data = m->n_data;
  hipLaunchKernelGGL(k_vg_head, dim3(B), dim3(64), 0, s, h);
  hipLaunchKernelGGL(k_vg_head_sum, dim3(g ? 1 + tiles(h.C * kVgClasses + kVgClasses, kVgThreads) : 1), blk, 0, s, h);
  // ---- backward: per layer the weight (and bias) gradient, then the gradient w.r.t. its input, masked by the ReLU of the
  // layer below -- directly, or on the way back through the pool between them
  for (int l = kVgLayers - 1; g && l >= 0; --l) {
    const int M = B << (2 * L[l].lw), K9 = 9 * L[l].cin;
    int per;
    const int splits = vg_wgrad_splits(B, L[l], &per);
    VgGemm a{in[l], dy, nullptr, scratch + sc.part, M, L[l].lw, L[l].cin, L[l].cout, per};
    hipLaunchKernelGGL(k_vg_gemm<VG_WGRAD>, dim3(tiles(K9, kVgBM), tiles(L[l].cout, kVgBN), splits), blk, 0, s, a);
    hipLaunchKernelGGL(k_vg_wsum, blocks((size_t)(K9 + 1) * L[l].cout), blk, 0, s, scratch + sc.part, splits,
                       K9 * L[l].cout, L[l].cout, g[2 * l], g[2 * l + 1]);
    if (l == 0) break;
    const bool pooled_input = L[l - 1].pool != 0;
    VgGemm d{dy, w[2 * l], pooled_input ? nullptr : in[l], other, M, L[l].lw, L[l].cin, L[l].cout, 0};
    hipLaunchKernelGGL(k_vg_gemm<VG_DGRAD>, dim3(tiles(M, kVgBM), tiles(L[l].cin, kVgBN)), blk, 0, s, d);
    if (pooled_input) {
      const size_t total = (size_t)M * L[l].cin;
      hipLaunchKernelGGL(k_vg_pool_bwd, blocks(total), blk, 0, s, scratch + sc.act[l - 1], other, dy, L[l - 1].lw, L[l].cin,
                         total);
    } else {
      std::swap(dy, other);
    }
  }
  HIP_TRY(hipGetLastError());
  return L2O_OK;
}

// ---- KernelDeepLSTM: one LSTM per convolution filter (csrc/l2o_klstm.h, include/l2o_klstm_abi.h) ----------------------------
static bool klstm_ok(const l2o_klstm_net* n) {
  if (!n || n->flags != 0) return false;
  if (n->kw < 1 || n->kw > L2O_KLSTM_MAX_SIDE || n->kh < 1 || n->kh > L2O_KLSTM_MAX_SIDE) return false;
  if (n->n_layers < 1 || n->n_layers > L2O_KLSTM_MAX_LAYERS) return false;
  for (int l = 0; l < n->n_layers; ++l)
    if (n->hidden[l] < 4 || n->hidden[l] > L2O_KLSTM_MAX_HIDDEN || n->hidden[l] % 4) return false;
  return n->preprocess == L2O_PRE_IDENTITY || n->preprocess == L2O_PRE_LOGSIGN;
}
static int klstm_check(const char* who, const l2o_klstm_net* n, int64_t N) {
  if (!klstm_ok(n) || N < 1)
    return fail(L2O_ERR_UNSUPPORTED, "%s: kw, kh in [1, %d], 1 or 2 layers of a width that is a multiple of 4 in [4, %d], "
                "preprocess identity or LogAndSign, flags 0, N >= 1", who, L2O_KLSTM_MAX_SIDE, L2O_KLSTM_MAX_HIDDEN);
  for (int l = 0; l < n->n_layers; ++l)
    if (!n->w_gates[l] || !n->b_gates[l]) return fail(L2O_ERR_ARG, "%s: NULL weights of layer %d", who, l);
  if (!n->w_lin || !n->b_lin) return fail(L2O_ERR_ARG, "%s: NULL output Linear", who);
  return L2O_OK;
}
int l2o_klstm_supported(const l2o_klstm_net* net) { return klstm_ok(net) ? 1 : 0; }
size_t l2o_klstm_state_floats(const l2o_klstm_net* net, int64_t N) {
  if (!klstm_ok(net) || N < 1) return 0;
  size_t n = 0;
  for (int l = 0; l < net->n_layers; ++l) n += 2 * (size_t)N * (size_t)net->hidden[l];
  return n;
}
int l2o_klstm_step(const l2o_klstm_net* net, const float* g, const float* state_in, float* state_out, float* x, int64_t N,
                   void* stream) {
  int rc = klstm_check("l2o_klstm_step", net, N);
  if (rc) return rc;
  if (!g || !state_in || !state_out || !x) return fail(L2O_ERR_ARG, "l2o_klstm_step: NULL argument");
  KlParams p;
  std::memset(&p, 0, sizeof(p));
  p.K = net->kw * net->kh;
  p.pre = net->preprocess;
  p.in = p.pre == L2O_PRE_LOGSIGN ? 2 * p.K : p.K;
  p.in_pad = (p.in + 3) / 4 * 4;
  p.n_layers = net->n_layers;
  for (int l = 0; l < net->n_layers; ++l) { p.H[l] = net->hidden[l]; p.wg[l] = net->w_gates[l]; p.bg[l] = net->b_gates[l]; }
  p.tanh_output = net->tanh_output;
  p.scale = (float)net->scale;
  p.k_inv = net->logsign_k != 0.0 ? (float)(1.0 / net->logsign_k) : 0.0f;
  p.exp_k = (float)std::exp(net->logsign_k);
  p.wl = net->w_lin; p.bl = net->b_lin;
  p.g = g; p.st_in = state_in; p.st_out = state_out; p.x = x; p.N = (long)N;
  const int64_t ntiles = (N + 15) / 16;
  if (ntiles > 0x7fffffff / 16) return fail(L2O_ERR_UNSUPPORTED, "l2o_klstm_step: N %lld is too large", (long long)N);
  p.ntiles = (int)ntiles;
  const int64_t wgs = (ntiles + kKlWaves - 1) / kKlWaves;
  return launch(k_klstm_step, dim3((unsigned)(wgs < kKlMaxBlocks ? wgs : kKlMaxBlocks)), dim3(kKlThreads),
                sizeof(float) * (size_t)kl_lds_floats(p), (hipStream_t)stream, p);
}
int l2o_klstm_bwd_step(const l2o_klstm_net* net, const l2o_klstm_bwd_io* io, int64_t N, void* stream) {
  int rc = klstm_check("l2o_klstm_bwd_step", net, N);
  if (rc) return rc;
  if (!io || !io->g || !io->st_prev || !io->dx_next || !io->carry_in || !io->carry_out || !io->tc || !io->h_last || !io->dd ||
      io->carry_in == io->carry_out)
    return fail(L2O_ERR_ARG, "l2o_klstm_bwd_step: bad argument");
  KlBwdParams p;
  std::memset(&p, 0, sizeof(p));
  p.K = net->kw * net->kh;
  p.pre = net->preprocess;
  p.in = p.pre == L2O_PRE_LOGSIGN ? 2 * p.K : p.K;
  p.n_layers = net->n_layers;
  for (int l = 0; l < net->n_layers; ++l) {
    if (!io->act[l] || !io->dz[l]) return fail(L2O_ERR_ARG, "l2o_klstm_bwd_step: NULL act / dz of layer %d", l);
    p.H[l] = net->hidden[l]; p.wg[l] = net->w_gates[l]; p.bg[l] = net->b_gates[l];
    p.act[l] = io->act[l]; p.dz[l] = io->dz[l];
  }
  p.tanh_output = net->tanh_output;
  p.scale = (float)net->scale;
  p.k_inv = net->logsign_k != 0.0 ? (float)(1.0 / net->logsign_k) : 0.0f;
  p.exp_k = (float)std::exp(net->logsign_k);
  p.wl = net->w_lin; p.bl = net->b_lin;
  p.g = io->g; p.st_prev = io->st_prev; p.dx_next = io->dx_next; p.carry_in = io->carry_in; p.carry_out = io->carry_out;
  p.tc = io->tc; p.h_last = io->h_last; p.dd = io->dd; p.N = (long)N;
  hipLaunchKernelGGL(k_klstm_bwd_step, dim3((unsigned)((N + kKlBwdThreads - 1) / kKlBwdThreads)), dim3(kKlBwdThreads), 0,
                     (hipStream_t)stream, p);
  HIP_TRY(hipGetLastError());
  return L2O_OK;
}

// ---- problems.NAS (csrc/l2o_nas.h, include/l2o_nas_abi.h) ----------------------------------------------------------------
static bool nas_ok(const l2o_nas* m) {
  return m && m->batch >= 2 && m->batch <= kNsMaxBatch && m->n_data >= 1 && m->flags == 0 &&
         (m->batch_norm == 0 || m->batch_norm == 1);
}
// The scratch of one call, in floats from its start (include/l2o_nas_abi.h has the formula).  Every size is a multiple of
// 4 floats.
struct NsScratch {
  size_t x0, z0, zz, z13, dy1, dy0, P, stat, bsum, nf, dlog, v, loss_s, part, total;
};
static NsScratch nas_scratch(int batch) {
  NsScratch s;
  const size_t B = (size_t)batch, M = B * kNsPix;
  size_t p = 0;
  auto take = [&](size_t n) { const size_t at = p; p += (n + 3) & ~(size_t)3; return at; };
  s.x0 = take(B * 3072);
  s.z0 = take(M * 16);
  s.zz = take(M * 32);
  s.z13 = take(M * 16);
  s.dy1 = take(M * 16);
  s.dy0 = take(M * 16);
  s.P = take(kNsLayers * kNsP);
  s.stat = take(B * 64);
  s.bsum = take(B * 64);
  s.nf = take(B * 16);
  s.dlog = take(B * 16);
  s.v = take(B * 16);
  s.loss_s = take(B);
  s.part = take((size_t)ns_wgrad_groups(batch) * kNsWPart);
  s.total = p;
  return s;
}
size_t l2o_nas_scratch_floats(const l2o_nas* m) { return nas_ok(m) ? nas_scratch(m->batch).total : 0; }
int l2o_nas_fg(const l2o_nas* m, const int32_t* indices, const float* const* w, float* loss, float* const* g, float* scratch,
               void* stream) {
  if (!nas_ok(m))
    return fail(L2O_ERR_UNSUPPORTED, "l2o_nas_fg: batch in [2, %d], batch_norm 0 or 1, flags 0, n_data >= 1", kNsMaxBatch);
  if (!indices || !w || !loss || !scratch || !m->images || !m->labels) return fail(L2O_ERR_ARG, "l2o_nas_fg: NULL argument");
  if ((uintptr_t)scratch & 15) return fail(L2O_ERR_ARG, "l2o_nas_fg: scratch must be 16-byte aligned");
  const int bn = m->batch_norm, per = bn ? 4 : 2, nvars = kNsLayers * per + 2;
  for (int k = 0; k < nvars; ++k)
    if (!w[k] || (g && !g[k])) return fail(L2O_ERR_ARG, "l2o_nas_fg: NULL buffer of variable %d", k);
  const NsScratch sc = nas_scratch(m->batch);
  hipStream_t s = (hipStream_t)stream;
  const int B = m->batch;
  const dim3 blk(kNsThreads), strips(4 * B), samples(B), one(1);
  float* x0 = scratch + sc.x0;
  float* z0 = scratch + sc.z0;
  float* zz = scratch + sc.zz;           // [M][32]: n02 in columns 0-15, node1 in 16-31
  float* z13 = scratch + sc.z13;
  float* dy1 = scratch + sc.dy1;
  float* dy0 = scratch + sc.dy0;
  float* P = scratch + sc.P;
  float* v = scratch + sc.v;
  // layer l (node0, n02, node1, n13): its variables
  auto W = [&](int l) { return w[l * per]; };
  auto Bi = [&](int l) { return w[l * per + 1]; };
  auto src = [](const float* z, int ldz, const float* dy, const float* Pl) { NsSrc r{z, dy, Pl, ldz}; return r; };
  const NsSrc none = src(nullptr, 0, nullptr, nullptr);
  // batch norm of layers l .. l + C / 16 - 1 whose z is the [M][C] array `z`
  auto norm = [&](const float* z, int l, int C) {
    if (!bn) return;
    NsBn a{scratch + sc.stat, {w[l * per + 2], C == 32 ? w[(l + 1) * per + 2] : nullptr},
           {w[l * per + 3], C == 32 ? w[(l + 1) * per + 3] : nullptr}, P + l * kNsP, B};
    if (C == 32) {
      hipLaunchKernelGGL(k_ns_stats<32>, samples, blk, 0, s, z, scratch + sc.stat);
      hipLaunchKernelGGL(k_ns_bn<32>, one, blk, 0, s, a);
    } else {
      hipLaunchKernelGGL(k_ns_stats<16>, samples, blk, 0, s, z, scratch + sc.stat);
      hipLaunchKernelGGL(k_ns_bn<16>, one, blk, 0, s, a);
    }
  };
  // ---- forward
  hipLaunchKernelGGL(k_vg_gather, samples, dim3(kVgThreads), 0, s, m->images, indices, m->n_data, x0);
  if (!bn) hipLaunchKernelGGL(k_ns_identity, one, blk, 0, s, P);
  {
    NsConv a{{src(x0, 3, nullptr, nullptr), none}, v, {W(0), nullptr}, {Bi(0), nullptr}, z0, nullptr, nullptr, 0, 0};
    hipLaunchKernelGGL((k_ns_conv<3, 16, NS_RAW>), strips, blk, 0, s, a);
    norm(z0, 0, 16);
  }
  {
    NsConv a{{src(z0, 16, nullptr, P), none}, v, {W(1), W(2)}, {Bi(1), Bi(2)}, zz, nullptr, nullptr, 0, 0};
    hipLaunchKernelGGL((k_ns_conv<16, 32, NS_ACT>), strips, blk, 0, s, a);
    norm(zz, 1, 32);
  }
  {
    NsConv a{{src(zz + 16, 32, nullptr, P + 2 * kNsP), none}, v, {W(3), nullptr}, {Bi(3), nullptr}, z13, nullptr, nullptr, 0, 0};
    hipLaunchKernelGGL((k_ns_conv<16, 16, NS_ACT>), strips, blk, 0, s, a);
    norm(z13, 3, 16);
  }
  NsHead h;
  std::memset(&h, 0, sizeof(h));
  h.z0 = z0; h.zz = zz; h.z13 = z13; h.P = P; h.wfc = w[nvars - 2]; h.bfc = w[nvars - 1]; h.labels = m->labels; h.idx = indices;
  h.nf = scratch + sc.nf; h.dlog = scratch + sc.dlog; h.v = v; h.loss_s = scratch + sc.loss_s; h.loss = loss;
  h.gwfc = g ? g[nvars - 2] : nullptr; h.gbfc = g ? g[nvars - 1] : nullptr; h.B = B; h.n_data = m->n_data;
  hipLaunchKernelGGL(k_ns_head, samples, blk, 0, s, h);
  hipLaunchKernelGGL(k_ns_head_sum, one, blk, 0, s, h);
  if (g) {
    // ---- backward.  The sums of a layer (or of n02 and node1 together): the two means of its NsP block(s) and the
    // gradients of gamma, beta and the bias
    auto sums = [&](const NsSrc& s0, const NsSrc& s1, int l, int C) {
      NsBwd a;
      std::memset(&a, 0, sizeof(a));
      a.src[0] = s0; a.src[1] = s1; a.v = v; a.part = scratch + sc.bsum; a.P = P + l * kNsP; a.B = B; a.bn = bn;
      for (int i = 0; i < C / 16; ++i) {
        a.gbias[i] = g[(l + i) * per + 1];
        if (bn) { a.ggamma[i] = g[(l + i) * per + 2]; a.gbeta[i] = g[(l + i) * per + 3]; }
      }
      if (C == 32) {
        hipLaunchKernelGGL(k_ns_bwd_sums<32>, samples, blk, 0, s, a);
        hipLaunchKernelGGL(k_ns_bwd_fin<32>, one, blk, 0, s, a);
      } else {
        hipLaunchKernelGGL(k_ns_bwd_sums<16>, samples, blk, 0, s, a);
        hipLaunchKernelGGL(k_ns_bwd_fin<16>, one, blk, 0, s, a);
      }
    };
    const int groups = ns_wgrad_groups(B);
    float* part = scratch + sc.part;
    auto wsum = [&](int K, int NOUT, float* g0, float* g1) {
      hipLaunchKernelGGL(k_ns_wsum, dim3((K * NOUT + kNsWsE - 1) / kNsWsE), blk, 0, s, part, groups, K, NOUT, g0, g1);
    };
    const NsSrc d13 = src(z13, 16, nullptr, P + 3 * kNsP);           // dy = u / 1024 under n13's mask
    const NsSrc d02 = src(zz, 32, nullptr, P + 1 * kNsP);
    const NsSrc d1 = src(zz + 16, 32, dy1, P + 2 * kNsP);
    const NsSrc d0 = src(z0, 16, dy0, P);
    // n13
    sums(d13, none, 3, 16);
    {
      NsWgrad a{src(zz + 16, 32, nullptr, P + 2 * kNsP), {d13, none}, v, part, 4 * B};
      hipLaunchKernelGGL((k_ns_wgrad<16, 16>), dim3(groups), blk, 0, s, a);
      wsum(144, 16, g[3 * per], g[3 * per]);
      NsConv c{{d13, none}, v, {W(3), nullptr}, {nullptr, nullptr}, dy1, zz + 16, P + 2 * kNsP, 32, 1};
      hipLaunchKernelGGL((k_ns_conv<16, 16, NS_DZ>), strips, blk, 0, s, c);
    }
    // n02 and node1
    sums(d02, d1, 1, 32);
    {
      NsWgrad a{src(z0, 16, nullptr, P), {d02, d1}, v, part, 4 * B};
      hipLaunchKernelGGL((k_ns_wgrad<16, 32>), dim3(groups), blk, 0, s, a);
      wsum(144, 32, g[1 * per], g[2 * per]);
      NsConv c{{d02, d1}, v, {W(1), W(2)}, {nullptr, nullptr}, dy0, z0, P, 16, 0};
      hipLaunchKernelGGL((k_ns_conv<32, 16, NS_DZ>), strips, blk, 0, s, c);
    }
    // node0
    sums(d0, none, 0, 16);
    {
      NsWgrad a{src(x0, 3, nullptr, nullptr), {d0, none}, v, part, 4 * B};
      hipLaunchKernelGGL((k_ns_wgrad<3, 16>), dim3(groups), blk, 0, s, a);
      wsum(27, 16, g[0], g[0]);
    }
  }
  HIP_TRY(hipGetLastError());
  return L2O_OK;
}

// ---- problems.confocal_microscopy_3d (csrc/l2o_confocal.h) ------------------------------------------------------------
static bool confocal_ok(const l2o_confocal* m) {
  if (!m || m->batch < 1 || m->batch > kCfMaxBatch || m->num_points < 1 || m->num_points > kCfMaxPts) return false;
  for (int k = 0; k < 3; ++k)
    if (m->roi[k] < kCfMinEdge || m->roi[k] > kCfMaxEdge) return false;
  return m->inference == 0 || m->inference == 1;
}
// planes of iy per workgroup: about kCfTargetWgs workgroups in all, a row never split further than one plane per slab
static void confocal_slabs(const l2o_confocal* m, int* slab, int* nslab) {
  int want = (kCfTargetWgs + m->batch - 1) / m->batch;
  if (want > m->roi[1]) want = m->roi[1];
  *slab = (m->roi[1] + want - 1) / want;
  *nslab = (m->roi[1] + *slab - 1) / *slab;
}
size_t l2o_confocal_scratch_floats(const l2o_confocal* m) {
  if (!confocal_ok(m)) return 0;
  int slab, nslab;
  confocal_slabs(m, &slab, &nslab);
  return (size_t)nslab * kCfPart * m->batch + m->batch;
}
int l2o_confocal_fg(const l2o_confocal* m, const float* const* theta, const float* const* sim, float* loss, float* const* g,
                    float* scratch, void* stream) {
  if (!confocal_ok(m))
    return fail(L2O_ERR_UNSUPPORTED, "l2o_confocal_fg: batch in [1, %d], num_points in [1, %d], roi edges in [%d, %d], "
                "inference 0 or 1", kCfMaxBatch, kCfMaxPts, kCfMinEdge, kCfMaxEdge);
  if (!theta || !loss || !scratch) return fail(L2O_ERR_ARG, "l2o_confocal_fg: NULL argument");
  if (m->inference ? !m->img : !sim) return fail(L2O_ERR_ARG, "l2o_confocal_fg: inference needs img, simulation needs sim");
  const int nv = 6 * m->num_points + 1;
  for (int k = 0; k < nv; ++k)
    if (!theta[k] || (g && !g[k]) || (!m->inference && !sim[k]))
      return fail(L2O_ERR_ARG, "l2o_confocal_fg: NULL buffer of variable %d", k);
  CfArgs a;
  std::memset(&a, 0, sizeof(a));
  a.batch = m->batch; a.P = m->num_points; a.rx = m->roi[0]; a.ry = m->roi[1]; a.rz = m->roi[2];
  a.inference = m->inference; a.want_grad = g ? 1 : 0;
  confocal_slabs(m, &a.slab, &a.nslab);
  a.img = m->inference ? m->img : nullptr;
  a.part = scratch;
  a.inv = scratch + (size_t)a.nslab * kCfPart * a.batch;
  a.loss = loss;
  for (int k = 0; k < nv; ++k) {
    a.th[k] = theta[k];
    a.sim[k] = m->inference ? nullptr : sim[k];
    a.g[k] = g ? g[k] : nullptr;
  }
  hipStream_t s = (hipStream_t)stream;
  const dim3 blk(kCfThreads);
  if (a.inference) hipLaunchKernelGGL(k_cf_norm, dim3(a.batch), blk, 0, s, a);
  hipLaunchKernelGGL(k_cf_slab, dim3(a.batch, a.nslab), blk, 0, s, a);
  const int nred = g ? (nv * a.batch + kCfThreads - 1) / kCfThreads : 1;
  hipLaunchKernelGGL(k_cf_reduce, dim3(nred), blk, 0, s, a);
  HIP_TRY(hipGetLastError());
  return L2O_OK;
}

// ---- the fused unroll of the confocal optimizee (csrc/l2o_confocal_unroll.h) ----------------------------------------------
static bool confocal_unroll_ok(const l2o_net_cfg* cfg, const l2o_confocal* m) {
  return cfg && net_ok_for_mfma(cfg) && confocal_ok(m);
}
int l2o_confocal_unroll_supported(const l2o_net_cfg* cfg, const l2o_confocal* m, void* /*stream*/) {
  return confocal_unroll_ok(cfg, m) ? 1 : 0;
}
// fx_part [T + 1][batch] (rounded up to whole pointers), then the history pointer table of a recording launch
static size_t confocal_unroll_fx_floats(const l2o_confocal* m, int T) { return (((size_t)T + 1) * m->batch + 1) & ~(size_t)1; }
size_t l2o_confocal_unroll_scratch_floats(const l2o_confocal* m, int32_t T) {
  if (!confocal_ok(m) || T < 0) return 0;
  return confocal_unroll_fx_floats(m, T) + 2 * 4 * (size_t)kCfMaxVars;
}
static int confocal_unroll_launch(const char* who, const l2o_net_cfg* cfg, const float* wpack, const l2o_confocal* m,
                                  float* const* x, float* const* st, float* const* mm, float* const* vv,
                                  const float* const* x_scale, const float* const* sim, int32_t T, int32_t step0, float* fx,
                                  const l2o_confocal_hist* hist, float* scratch, void* stream) {
  if (!confocal_unroll_ok(cfg, m))
    return fail(L2O_ERR_UNSUPPORTED, "%s: the (20, 20) LSTM nets; batch in [1, %d], num_points in [1, %d], roi edges in "
                "[%d, %d], inference 0 or 1", who, kCfMaxBatch, kCfMaxPts, kCfMinEdge, kCfMaxEdge);
  if (!wpack || !x || !st || !fx || !scratch || T < 0) return fail(L2O_ERR_ARG, "%s: NULL argument or T < 0", who);
  if (m->inference ? !m->img : !sim) return fail(L2O_ERR_ARG, "%s: inference needs img, simulation needs sim", who);
  const bool rn = cfg->preprocess == L2O_PRE_FC_ELU;
  if (rn && (!mm || !vv)) return fail(L2O_ERR_ARG, "%s: RNNProp needs m and v", who);
  const int nv = 6 * m->num_points + 1;
  CfUnrollArgs a;
  std::memset(&a, 0, sizeof(a));
  CfHistPtrs hp;
  std::memset(&hp, 0, sizeof(hp));
  for (int k = 0; k < nv; ++k) {
    if (!x[k] || !st[k] || (rn && (!mm[k] || !vv[k])) || (!m->inference && !sim[k]))
      return fail(L2O_ERR_ARG, "%s: NULL buffer of variable %d", who, k);
    a.x[k] = x[k]; a.st[k] = st[k];
    a.m[k] = rn ? mm[k] : nullptr; a.v[k] = rn ? vv[k] : nullptr;
    a.xs[k] = x_scale ? x_scale[k] : nullptr;
    a.sim[k] = m->inference ? nullptr : sim[k];
    if (hist) {
      if (!hist->st[k] || !hist->g[k] || (rn && (!hist->m[k] || !hist->v[k])))
        return fail(L2O_ERR_ARG, "%s: NULL history buffer of variable %d", who, k);
      hp.p[0][k] = hist->st[k]; hp.p[1][k] = hist->g[k];
      hp.p[2][k] = rn ? hist->m[k] : nullptr; hp.p[3][k] = rn ? hist->v[k] : nullptr;
    }
  }
  a.np = make_net_params(cfg, wpack);
  a.batch = m->batch; a.P = m->num_points; a.rx = m->roi[0]; a.ry = m->roi[1]; a.rz = m->roi[2];
  a.inference = m->inference; a.T = T;
  a.rb = 1.0f / (float)m->batch;
  pow_ff(cfg->beta1, step0, &a.p1_hi, &a.p1_lo);
  pow_ff(cfg->beta2, step0, &a.p2_hi, &a.p2_lo);
  a.img = m->inference ? m->img : nullptr;
  a.fx_part = scratch;
  float** tab = reinterpret_cast<float**>(scratch + confocal_unroll_fx_floats(m, T));
  a.htab = hist ? tab : nullptr;
  hipStream_t s = (hipStream_t)stream;
  if (hist) hipLaunchKernelGGL(k_cf_hist_table, dim3(1), dim3(256), 0, s, hp, tab);
  const size_t lds = sizeof(float) * (size_t)a.rx * a.ry * a.rz;
  const int rc = with_pre(cfg->preprocess, [&](auto pre) { return launch_confocal_unroll<decltype(pre)::value>(a, hist != nullptr, lds, s); });
  if (rc != L2O_OK) return rc;
  hipLaunchKernelGGL(k_reduce_fx, dim3(T + 1), dim3(64), 0, s, a.fx_part, (int)(T + 1), (int)a.batch, a.rb, fx);
  HIP_TRY(hipGetLastError());
  note_form(L2O_FORM_CONFOCAL_UNROLL);
  return L2O_OK;
}
int l2o_confocal_unroll(const l2o_net_cfg* cfg, const float* wpack, const l2o_confocal* m, float* const* x, float* const* st,
                        float* const* mm, float* const* vv, const float* const* x_scale, const float* const* sim, int32_t T,
                        int32_t step0, float* fx, float* scratch, void* stream) {
  return confocal_unroll_launch("l2o_confocal_unroll", cfg, wpack, m, x, st, mm, vv, x_scale, sim, T, step0, fx, nullptr,
                                scratch, stream);
}
int l2o_confocal_unroll_record(const l2o_net_cfg* cfg, const float* wpack, const l2o_confocal* m, float* const* x,
                               float* const* st, float* const* mm, float* const* vv, const float* const* x_scale,
                               const float* const* sim, int32_t T, int32_t step0, float* fx, const l2o_confocal_hist* hist,
                               float* scratch, void* stream) {
  if (!hist) return fail(L2O_ERR_ARG, "l2o_confocal_unroll_record: NULL hist");
  return confocal_unroll_launch("l2o_confocal_unroll_record", cfg, wpack, m, x, st, mm, vv, x_scale, sim, T, step0, fx, hist,
                                scratch, stream);
}

// ---- several confocal instances per fused launch (include/l2o_confocal_multi_abi.h) ------------------------------------------
static bool confocal_unroll_multi_ok(const l2o_net_cfg* cfg, const l2o_confocal* m, int32_t n_inst) {
  return confocal_unroll_ok(cfg, m) && n_inst >= 1 && n_inst <= L2O_CONFOCAL_MAX_INSTANCES;
}
int l2o_confocal_unroll_multi_supported(const l2o_net_cfg* cfg, const l2o_confocal* m, int32_t n_inst, void* /*stream*/) {
  return confocal_unroll_multi_ok(cfg, m, n_inst) ? 1 : 0;
}
// n_inst x fx_part [T + 1][batch] (each rounded up to whole pointers), then the n_inst pointer tables
size_t l2o_confocal_unroll_multi_scratch_floats(const l2o_confocal* m, int32_t n_inst, int32_t T) {
  if (!confocal_ok(m) || T < 0 || n_inst < 1 || n_inst > L2O_CONFOCAL_MAX_INSTANCES) return 0;
  return (size_t)n_inst * (confocal_unroll_fx_floats(m, T) + 2 * (size_t)kCfInstPtrs);
}
static int confocal_unroll_multi_launch(const char* who, const l2o_net_cfg* cfg, const float* wpack, const l2o_confocal* m,
                                        const l2o_confocal_instance* inst, int32_t n_inst, int32_t T, int32_t step0,
                                        const l2o_confocal_hist* hist, float* scratch, void* stream) {
  if (!confocal_unroll_multi_ok(cfg, m, n_inst))
    return fail(L2O_ERR_UNSUPPORTED, "%s: the (20, 20) LSTM nets; batch in [1, %d], num_points in [1, %d], roi edges in "
                "[%d, %d], inference 0 or 1; 1 to %d instances", who, kCfMaxBatch, kCfMaxPts, kCfMinEdge, kCfMaxEdge,
                L2O_CONFOCAL_MAX_INSTANCES);
  if (!wpack || !inst || !scratch || T < 0) return fail(L2O_ERR_ARG, "%s: NULL argument or T < 0", who);
  const bool rn = cfg->preprocess == L2O_PRE_FC_ELU;
  const int nv = 6 * m->num_points + 1;
  // every instance is checked before anything is launched
  for (int i = 0; i < n_inst; ++i) {
    const l2o_confocal_instance& in = inst[i];
    if (!in.fx || (m->inference && !in.img)) return fail(L2O_ERR_ARG, "%s: instance %d: NULL fx, or inference without img", who, i);
    for (int k = 0; k < nv; ++k) {
      if (!in.x[k] || !in.st[k] || (rn && (!in.m[k] || !in.v[k])) || (!m->inference && !in.sim[k]))
        return fail(L2O_ERR_ARG, "%s: instance %d: NULL buffer of variable %d", who, i, k);
      if (hist && (!hist[i].st[k] || !hist[i].g[k] || (rn && (!hist[i].m[k] || !hist[i].v[k]))))
        return fail(L2O_ERR_ARG, "%s: instance %d: NULL history buffer of variable %d", who, i, k);
    }
  }
  const size_t fx_floats = confocal_unroll_fx_floats(m, T);
  float** tab = reinterpret_cast<float**>(scratch + (size_t)n_inst * fx_floats);
  hipStream_t s = (hipStream_t)stream;
  for (int i = 0; i < n_inst; ++i) {
    const l2o_confocal_instance& in = inst[i];
    CfInstPtrs ip;
    std::memset(&ip, 0, sizeof(ip));
    CfHistPtrs hp;
    std::memset(&hp, 0, sizeof(hp));
    for (int k = 0; k < nv; ++k) {
      ip.p[0][k] = in.x[k]; ip.p[1][k] = in.st[k];
      ip.p[2][k] = rn ? in.m[k] : nullptr; ip.p[3][k] = rn ? in.v[k] : nullptr;
      ip.p[4][k] = const_cast<float*>(in.x_scale[k]);
      ip.p[5][k] = m->inference ? nullptr : const_cast<float*>(in.sim[k]);
      if (hist) {
        hp.p[0][k] = hist[i].st[k]; hp.p[1][k] = hist[i].g[k];
        hp.p[2][k] = rn ? hist[i].m[k] : nullptr; hp.p[3][k] = rn ? hist[i].v[k] : nullptr;
      }
    }
    ip.img = m->inference ? const_cast<float*>(in.img) : nullptr;
    ip.fx_part = scratch + (size_t)i * fx_floats;
    ip.fx = in.fx;
    float** it = tab + (size_t)i * kCfInstPtrs;
    hipLaunchKernelGGL(k_cf_inst_table, dim3(1), dim3(320), 0, s, ip, it);
    if (hist) hipLaunchKernelGGL(k_cf_hist_table, dim3(1), dim3(256), 0, s, hp, it + kCfTabHist);
  }
  HIP_TRY(hipGetLastError());
  CfUnrollMultiArgs a;
  std::memset(&a, 0, sizeof(a));
  a.np = make_net_params(cfg, wpack);
  a.batch = m->batch; a.P = m->num_points; a.rx = m->roi[0]; a.ry = m->roi[1]; a.rz = m->roi[2];
  a.inference = m->inference; a.T = T;
  a.rb = 1.0f / (float)m->batch;
  pow_ff(cfg->beta1, step0, &a.p1_hi, &a.p1_lo);
  pow_ff(cfg->beta2, step0, &a.p2_hi, &a.p2_lo);
  a.tab = tab;
  const size_t lds = sizeof(float) * (size_t)a.rx * a.ry * a.rz;
  const int rc = with_pre(cfg->preprocess, [&](auto pre) { return launch_confocal_unroll_multi<decltype(pre)::value>(a, n_inst, hist != nullptr, lds, s); });
  if (rc != L2O_OK) return rc;
  hipLaunchKernelGGL(k_cf_reduce_fx_multi, dim3(T + 1, n_inst), dim3(64), 0, s, tab, (int)a.batch, a.rb);
  HIP_TRY(hipGetLastError());
  note_form(L2O_FORM_CONFOCAL_MULTI);
  return L2O_OK;
}
int l2o_confocal_unroll_multi(const l2o_net_cfg* cfg, const float* wpack, const l2o_confocal* m,
                              const l2o_confocal_instance* inst, int32_t n_inst, int32_t T, int32_t step0, float* scratch,
                              void* stream) {
  return confocal_unroll_multi_launch("l2o_confocal_unroll_multi", cfg, wpack, m, inst, n_inst, T, step0, nullptr, scratch,
                                      stream);
}
int l2o_confocal_unroll_multi_record(const l2o_net_cfg* cfg, const float* wpack, const l2o_confocal* m,
                                     const l2o_confocal_instance* inst, int32_t n_inst, int32_t T, int32_t step0,
                                     const l2o_confocal_hist* hist, float* scratch, void* stream) {
  if (!hist) return fail(L2O_ERR_ARG, "l2o_confocal_unroll_multi_record: NULL hist");
  return confocal_unroll_multi_launch("l2o_confocal_unroll_multi_record", cfg, wpack, m, inst, n_inst, T, step0, hist,
                                      scratch, stream);
}

#ifndef L2O_MLP_XCD_DEFAULT_FOUR
#define L2O_MLP_XCD_DEFAULT_FOUR 0     // (set from the A/B measurement: profiles/r06_c5_xcd_forms_ab.txt)
#endif
// ---- one optimizee instance per XCD (csrc/l2o_mlp_xcd.h) ------------------------------------------------------------
struct MlpXcdLayout { int n[4], tile_begin[5], nw1; size_t team_off, inst_off, p_bytes, s_bytes, sm_bytes, inst_bytes, total; };
static bool mlp_xcd_layout(const l2o_mlp* mlp, int n_inst, MlpXcdLayout* L) {
  if (!mlp || n_inst < 1 || n_inst > kMxMaxInst) return false;
  if (mlp->n_hidden != kMxH || mlp->n_out != kMxO || (mlp->batch != 64 && mlp->batch != 128) || mlp->n_in < 1) return false;
  const int NO = mlp->batch * kMxH;                   // MxShape<batch>::kNO
  L->n[0] = mlp->n_in * kMxH; L->n[1] = kMxH; L->n[2] = kMxH * kMxO; L->n[3] = kMxO;
  L->tile_begin[0] = 0;
  for (int v = 0; v < 4; ++v) L->tile_begin[v + 1] = L->tile_begin[v] + tiles_per_problem(L->n[v]);
  // members 0 .. 30: the w1 tiles (32 each); member 31: b1 | w2 | b2
  if (L->tile_begin[1] > (kMxMembers - 1) * kMxSlots || L->tile_begin[4] - L->tile_begin[1] > kMxSlots) return false;
  L->nw1 = (L->n[0] + kMxCoords - 1) / kMxCoords;
  L->team_off = sizeof(MlpWs);
  L->inst_off = L->team_off + 64;
  L->p_bytes = sizeof(unsigned long long) * kMxMembers * kMxMembers * (NO / kMxMembers);
  L->s_bytes = sizeof(unsigned long long) * 2 * NO;
  L->sm_bytes = sizeof(unsigned long long) * 2 * kMxNSMp;
  L->inst_bytes = (L->p_bytes + L->s_bytes + L->sm_bytes + 255) & ~(size_t)255;
  L->total = L->inst_off + (size_t)n_inst * L->inst_bytes;
  return true;
}

// the four-wave form (k_mlp_xcd<PRE, 4>): L2O_OPT_MLP_XCD_WAVES = 2, or the build's default for RNNProp
static bool mlp_xcd_four(const l2o_net_cfg* cfg) {
  const int wopt = (int)opt(L2O_OPT_MLP_XCD_WAVES);
  return wopt == 2 || (wopt == 0 && cfg->preprocess == L2O_PRE_FC_ELU && L2O_MLP_XCD_DEFAULT_FOUR);
}

int l2o_mlp_unroll_multi_supported(const l2o_net_cfg* cfg, const l2o_mlp* mlp, int32_t n_inst, void* stream) {
  OptScope opt_scope(cfg_optw(cfg));
  MlpXcdLayout L;
  if (!cfg || !net_ok_for_mfma(cfg) || !opt(L2O_OPT_MLP_UNROLL) || !mlp_xcd_layout(mlp, n_inst, &L)) return 0;
  if (mlp->batch != 64 && mlp_xcd_four(cfg)) return 0;      // (the four-wave form has no batch-128 instantiation)
  // every XCD's 32 CUs must be able to host one workgroup each at the same time
  return coresident_cus((hipStream_t)stream) >= kMxMaxInst * kMxMembers ? 1 : 0;
}

size_t l2o_mlp_unroll_multi_workspace_bytes(const l2o_mlp* mlp, int32_t n_inst) {
  MlpXcdLayout L;
  return mlp_xcd_layout(mlp, n_inst, &L) ? L.total : 0;
}

static int mlp_unroll_multi_launch(const l2o_net_cfg* cfg, const float* wpack, const l2o_mlp* mlp, const l2o_mlp_instance* inst,
                                   int32_t n_inst, int32_t T, int32_t step0, const l2o_mlp_hist* hist, void* workspace, void* stream) {
  OptScope opt_scope(cfg_optw(cfg));
  if (!cfg || !wpack || !mlp || !inst || !workspace || T < 0 || !mlp->images || !mlp->labels)
    return fail(L2O_ERR_ARG, "l2o_mlp_unroll_multi: bad argument");
  hipStream_t s = (hipStream_t)stream;
  MlpXcdLayout L;
  if (!net_ok_for_mfma(cfg) || !mlp_xcd_layout(mlp, n_inst, &L) || coresident_cus(s) < kMxMaxInst * kMxMembers)
    return fail(L2O_ERR_UNSUPPORTED, "l2o_mlp_unroll_multi: no one-XCD kernel for n_in=%d hidden=%d out=%d batch=%d x %d instances "
                "(needs the reference's shape and all 8 x 32 CUs)", mlp->n_in, mlp->n_hidden, mlp->n_out, mlp->batch, (int)n_inst);
  // which form: four waves per member stepping tile PAIRS (a lone wave per SIMD with two independent chains; RNNProp: no
  // spills at 438 registers) or eight waves stepping single tiles (two waves per SIMD; the DM nets' pair form spills)
  const bool four = mlp_xcd_four(cfg);
  if (four && mlp->batch != 64)
    return fail(L2O_ERR_UNSUPPORTED, "l2o_mlp_unroll_multi: the four-wave one-XCD form serves batch 64 only (batch %d)", mlp->batch);
  const bool rn = cfg->preprocess == L2O_PRE_FC_ELU;
  MlpXcdHistArgs a;                                   // (the plain form is launched with its MlpXcdArgs part)
  std::memset(&a, 0, sizeof(a));
  a.np = make_net_params(cfg, wpack);
  a.n_in = mlp->n_in; a.act = mlp->activation; a.T = T; a.ninst = n_inst;
  a.images = mlp->images; a.labels = mlp->labels;
  for (int k = 0; k < 4; ++k) a.n[k] = L.n[k];
  for (int k = 0; k < 5; ++k) a.tile_begin[k] = L.tile_begin[k];
  a.nw1 = L.nw1;
  pow_ff(cfg->beta1, step0, &a.p1_hi, &a.p1_lo);
  pow_ff(cfg->beta2, step0, &a.p2_hi, &a.p2_lo);
  char* wsb = static_cast<char*>(workspace);
  a.ws = reinterpret_cast<MlpWs*>(wsb);
  a.team = reinterpret_cast<unsigned*>(wsb + L.team_off);
  for (int j = 0; j < n_inst; ++j) {
    const l2o_mlp_instance& in = inst[j];
    MxInst& o = a.inst[j];
    if (!in.indices || !in.fx) return fail(L2O_ERR_ARG, "l2o_mlp_unroll_multi: NULL indices / fx of instance %d", j);
    o.idx = in.indices; o.fx = in.fx;
    for (int k = 0; k < 4; ++k) {
      if (!in.x[k] || !in.st[k] || (rn && (!in.m[k] || !in.v[k])))
        return fail(L2O_ERR_ARG, "l2o_mlp_unroll_multi: NULL buffer of variable %d of instance %d", k, j);
      o.x[k] = in.x[k]; o.st[k] = in.st[k]; o.m[k] = rn ? in.m[k] : nullptr; o.v[k] = rn ? in.v[k] : nullptr;
      o.xscale[k] = in.x_scale[k];
    }
    char* ib = wsb + L.inst_off + (size_t)j * L.inst_bytes;
    o.P = reinterpret_cast<unsigned long long*>(ib);
    o.S = reinterpret_cast<unsigned long long*>(ib + L.p_bytes);
    o.Sm = reinterpret_cast<unsigned long long*>(ib + L.p_bytes + L.s_bytes);
    if (hist) {
      const l2o_mlp_hist& h = hist[j];
      MxHist& oh = a.hist[j];
      for (int k = 0; k < 4; ++k) {
        if (!h.st[k] || !h.g[k] || (rn && (!h.m[k] || !h.v[k])))
          return fail(L2O_ERR_ARG, "l2o_mlp_unroll_multi_record: NULL history buffer of variable %d of instance %d", k, j);
        oh.st[k] = h.st[k]; oh.g[k] = h.g[k];
        oh.m[k] = rn ? h.m[k] : nullptr; oh.v[k] = rn ? h.v[k] : nullptr;
      }
    }
  }
  HIP_TRY(hipMemsetAsync(wsb + L.team_off, 0, L.total - L.team_off, s));   // team counters + granules: the header survives
  const bool b128 = mlp->batch == 128;
  // one workgroup per CU of the whole chip: the 32 that land on XCD j < n_inst form instance j's team, the others exit
  const dim3 grid(kMxMaxInst * kMxMembers), block(four ? kMxThreads4 : kMxThreads);
  const int rc = with_pre(cfg->preprocess, [&](auto pre) {
    constexpr int PRE = decltype(pre)::value;
    const size_t lds = b128 ? mlp_xcd_lds_bytes<PRE, 128>() : mlp_xcd_lds_bytes<PRE, 64>();
    if (hist) {
      void (*fn)(MlpXcdHistArgs) = b128 ? k_mlp_xcd<PRE, 8, true, 128> : four ? k_mlp_xcd<PRE, 4, true> : k_mlp_xcd<PRE, 8, true>;
      return launch(fn, grid, block, lds, s, a);
    }
    void (*fn)(MlpXcdArgs) = b128 ? k_mlp_xcd<PRE, 8, false, 128> : four ? k_mlp_xcd<PRE, 4> : k_mlp_xcd<PRE, 8>;
    return launch(fn, grid, block, lds, s, static_cast<const MlpXcdArgs&>(a));
  });
  if (rc) return rc;
  note_form(L2O_FORM_MLP_XCD);
  return L2O_OK;
}

int l2o_mlp_unroll_multi(const l2o_net_cfg* cfg, const float* wpack, const l2o_mlp* mlp, const l2o_mlp_instance* inst,
                         int32_t n_inst, int32_t T, int32_t step0, void* workspace, void* stream) {
  return mlp_unroll_multi_launch(cfg, wpack, mlp, inst, n_inst, T, step0, nullptr, workspace, stream);
}
int l2o_mlp_unroll_multi_record(const l2o_net_cfg* cfg, const float* wpack, const l2o_mlp* mlp, const l2o_mlp_instance* inst,
                                int32_t n_inst, int32_t T, int32_t step0, const l2o_mlp_hist* hist, void* workspace,
                                void* stream) {
  if (!hist) return fail(L2O_ERR_ARG, "l2o_mlp_unroll_multi_record: NULL hist");
  return mlp_unroll_multi_launch(cfg, wpack, mlp, inst, n_inst, T, step0, hist, workspace, stream);
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

static int launch_bwd_tile(const BwdParams& p, int pre, hipStream_t s) {
  size_t nblk = ((size_t)p.tile_end[p.nseg - 1] + 3) / 4;
  size_t cap = (size_t)device_cu_count(s);              // persistent: one workgroup per CU walks the tile groups
  if (opt(L2O_OPT_BWD_BLOCKS) > 0) cap = (size_t)opt(L2O_OPT_BWD_BLOCKS);
  if (nblk > cap && p.T <= 1) nblk = cap;                  // (a T-step launch keeps one workgroup per four tiles: each lives T steps)
  const dim3 grid((unsigned)nblk), block(256);
  const bool mfma = p.wpack && opt(L2O_OPT_BWD_KERNEL) == 0;   // the matrix-core form needs the packed weights
  return with_pre(pre, [&](auto pr) {
    constexpr int PRE = decltype(pr)::value;
    if (mfma) return launch(k_cwlstm_bwd_mfma<PRE>, grid, block, sizeof(float) * BwdMfmaGeom<PRE>::kLdsFloats, s, p);
    return launch(k_cwlstm_bwd_tile<PRE>, grid, block, sizeof(float) * BwdTileGeom<PRE>::kLdsFloats, s, p);
  });
}

static void fill_bwd_net(BwdParams& p, const l2o_net_cfg* cfg, const l2o_net_weights* w, double pow1, double pow2) {
  p.pre = cfg->preprocess; p.tanh_output = cfg->tanh_output; p.n_layers = cfg->n_layers;
  p.scale = (float)cfg->scale;
  p.k_inv = cfg->logsign_k != 0.0 ? (float)(1.0 / cfg->logsign_k) : 0.0f;
  p.exp_k = (float)std::exp(cfg->logsign_k);
  p.beta1 = (float)cfg->beta1; p.beta2 = (float)cfg->beta2;
  p.om1 = (float)(1.0 - pow1); p.om2 = (float)(1.0 - pow2);
  p.wg1 = w->w_gates1; p.bg1 = w->b_gates1; p.wg2 = w->w_gates2; p.bg2 = w->b_gates2;
  p.wl = w->w_lin; p.bl = w->b_lin; p.wfc = w->w_fc; p.bfc = w->b_fc;
  p.wpack = w->wpack;
}

int l2o_cwlstm_bwd_multi(const l2o_net_cfg* cfg, const l2o_net_weights* w, const l2o_bwd_seg* segs, int32_t nseg,
                         const float* carry_in, float* carry_out, float* A, float* Bm, double pow1, double pow2,
                         void* stream) {
  OptScope opt_scope(cfg_optw(cfg));
  if (!cfg || !w || !segs || nseg < 1 || !carry_in || !carry_out || !A || !Bm)
    return fail(L2O_ERR_ARG, "l2o_cwlstm_bwd_multi: bad argument");
  if (nseg > 8) return fail(L2O_ERR_UNSUPPORTED, "l2o_cwlstm_bwd_multi: at most 8 panels");
  if (!net_ok_for_mfma(cfg) || cfg->n_layers == 0)
    return fail(L2O_ERR_UNSUPPORTED, "l2o_cwlstm_bwd_multi: only layers=(20,20) nets");
  if (!w->w_gates1 || !w->b_gates1 || !w->w_gates2 || !w->b_gates2 || !w->w_lin || !w->b_lin)
    return fail(L2O_ERR_ARG, "l2o_cwlstm_bwd_multi: NULL weights");
  const int pre = cfg->preprocess;
  if (pre == L2O_PRE_FC_ELU && (!w->w_fc || !w->b_fc)) return fail(L2O_ERR_ARG, "l2o_cwlstm_bwd_multi: fc weights");
  if (((uintptr_t)A & 15) || ((uintptr_t)Bm & 15)) return fail(L2O_ERR_ARG, "l2o_cwlstm_bwd_multi: A / Bm must be 16-byte aligned");
  BwdParams p;
  std::memset(&p, 0, sizeof(p));
  fill_bwd_net(p, cfg, w, pow1, pow2);
  p.carry_in = carry_in; p.carry_out = carry_out; p.act1 = A; p.dz1 = Bm;
  p.nseg = nseg;
  long tiles = 0;
  for (int i = 0; i < nseg; ++i) {
    const l2o_bwd_seg& sgm = segs[i];
    if (!sgm.g || !sgm.st_prev || !sgm.dx_next || sgm.B <= 0 || sgm.D <= 0 ||
        (pre == L2O_PRE_FC_ELU && (!sgm.m || !sgm.v)))
      return fail(L2O_ERR_ARG, "l2o_cwlstm_bwd_multi: bad panel %d", i);
    if (sgm.D % kTile != 0 && sgm.B != 1)
      return fail(L2O_ERR_UNSUPPORTED, "l2o_cwlstm_bwd_multi: panel %d needs D %% 16 == 0 or B == 1", i);
    const long n = (long)(sgm.B * sgm.D);
    tiles += (n + kTile - 1) / kTile;
    if (tiles > INT32_MAX / kTile) return fail(L2O_ERR_UNSUPPORTED, "l2o_cwlstm_bwd_multi: too many coordinates");
    p.tile_end[i] = (int)tiles;
    p.seg_n[i] = n;
    p.seg_d[i] = n; p.seg_tpp[i] = (int)((n + kTile - 1) / kTile);   // (tile-aligned or one row: the flat numbering)
    p.seg_g[i] = sgm.g; p.seg_m[i] = sgm.m; p.seg_v[i] = sgm.v; p.seg_st[i] = sgm.st_prev; p.seg_dx[i] = sgm.dx_next;
  }
  p.rows_total = tiles * kTile;
  return launch_bwd_tile(p, pre, (hipStream_t)stream);
}

static int bwd_unroll_impl(const l2o_net_cfg* cfg, const l2o_net_weights* w, const l2o_bwd_unroll_seg* segs,
                           int32_t nseg, const float* const* table, int32_t T, int64_t step0, const float* carry_in,
                           float* carry_out, float* A, float* Bm, void* stream, int compact);
int l2o_cwlstm_bwd_unroll(const l2o_net_cfg* cfg, const l2o_net_weights* w, const l2o_bwd_unroll_seg* segs,
                          int32_t nseg, const float* const* table, int32_t T, int64_t step0, const float* carry_in,
                          float* carry_out, float* A, float* Bm, void* stream) {
  return bwd_unroll_impl(cfg, w, segs, nseg, table, T, step0, carry_in, carry_out, A, Bm, stream, 0);
}
int l2o_cwlstm_bwd_unroll_compact(const l2o_net_cfg* cfg, const l2o_net_weights* w, const l2o_bwd_unroll_seg* segs,
                                  int32_t nseg, const float* const* table, int32_t T, int64_t step0, const float* carry_in,
                                  float* carry_out, float* Ac, float* Bm, void* stream) {
  return bwd_unroll_impl(cfg, w, segs, nseg, table, T, step0, carry_in, carry_out, Ac, Bm, stream, 1);
}
static int bwd_unroll_impl(const l2o_net_cfg* cfg, const l2o_net_weights* w, const l2o_bwd_unroll_seg* segs,
                           int32_t nseg, const float* const* table, int32_t T, int64_t step0, const float* carry_in,
                           float* carry_out, float* A, float* Bm, void* stream, int compact) {
  OptScope opt_scope(cfg_optw(cfg));
  if (!cfg || !w || !segs || nseg < 1 || !table || T < 1 || step0 < 0 || !A || !Bm)
    return fail(L2O_ERR_ARG, "l2o_cwlstm_bwd_unroll: bad argument");
  if (nseg > 8) return fail(L2O_ERR_UNSUPPORTED, "l2o_cwlstm_bwd_unroll: at most 8 panels");
  if (!net_ok_for_mfma(cfg) || cfg->n_layers == 0)
    return fail(L2O_ERR_UNSUPPORTED, "l2o_cwlstm_bwd_unroll: only layers=(20,20) nets");
  if (!w->wpack) return fail(L2O_ERR_ARG, "l2o_cwlstm_bwd_unroll: needs l2o_net_weights.wpack");
  if (((uintptr_t)A & 15) || ((uintptr_t)Bm & 15)) return fail(L2O_ERR_ARG, "l2o_cwlstm_bwd_unroll: A / Bm must be 16-byte aligned");
  const int pre = cfg->preprocess;
  BwdParams p;
  std::memset(&p, 0, sizeof(p));
  fill_bwd_net(p, cfg, w, 0.0, 0.0);
  p.carry_in = carry_in; p.carry_out = carry_out; p.act1 = A; p.dz1 = Bm;
  p.nseg = nseg; p.T = T; p.table = table;
  if (compact && opt(L2O_OPT_BWD_KERNEL) != 0)
    return fail(L2O_ERR_UNSUPPORTED, "l2o_cwlstm_bwd_unroll_compact: the matrix-core BPTT kernel only (L2O_OPT_BWD_KERNEL = 0)");
  p.compact_a = compact;
  p.pw1_last = std::pow((double)p.beta1, (double)(step0 + T - 1));
  p.pw2_last = std::pow((double)p.beta2, (double)(step0 + T - 1));
  long tiles = 0;
  for (int i = 0; i < nseg; ++i) {
    const l2o_bwd_unroll_seg& sgm = segs[i];
    if (sgm.B <= 0 || sgm.D <= 0) return fail(L2O_ERR_ARG, "l2o_cwlstm_bwd_unroll: bad panel %d", i);
    const long n = (long)(sgm.B * sgm.D);
    const long tpp = (long)tiles_per_problem(sgm.D);        // per-problem tiles, the packed-state layout of the forward
    tiles += (long)sgm.B * tpp;
    if (tiles > INT32_MAX / kTile) return fail(L2O_ERR_UNSUPPORTED, "l2o_cwlstm_bwd_unroll: too many coordinates");
    p.tile_end[i] = (int)tiles;
    p.seg_n[i] = n;
    p.seg_d[i] = (long)sgm.D;
    p.seg_tpp[i] = (int)tpp;
    p.seg_gfinal[i] = sgm.g_final;
  }
  p.rows_total = tiles * kTile;
  return launch_bwd_tile(p, pre, (hipStream_t)stream);
}

int l2o_cwlstm_bwd_step(const l2o_net_cfg* cfg, const l2o_net_weights* w, const l2o_bwd_io* io, double pow1,
                        double pow2, int64_t B, int64_t D, void* stream) {
  OptScope opt_scope(cfg_optw(cfg));
  if (!cfg || !w || !io || B <= 0 || D <= 0 || !io->g || !io->dx_next || !io->act1 || !io->dd || !w->w_lin ||
      !w->b_lin)
    return fail(L2O_ERR_ARG, "l2o_cwlstm_bwd_step: bad argument");
  BwdParams p;
  std::memset(&p, 0, sizeof(p));
  p.B = (int)B; p.D = (int)D; p.tpp = tiles_per_problem(D);
  p.pre = cfg->preprocess; p.tanh_output = cfg->tanh_output; p.n_layers = cfg->n_layers;
  p.scale = (float)cfg->scale;
  p.k_inv = cfg->logsign_k != 0.0 ? (float)(1.0 / cfg->logsign_k) : 0.0f;
  p.exp_k = (float)std::exp(cfg->logsign_k);
  p.beta1 = (float)cfg->beta1; p.beta2 = (float)cfg->beta2;
  p.om1 = (float)(1.0 - pow1); p.om2 = (float)(1.0 - pow2);
  p.wg1 = w->w_gates1; p.bg1 = w->b_gates1; p.wg2 = w->w_gates2; p.bg2 = w->b_gates2;
  p.wl = w->w_lin; p.bl = w->b_lin; p.wfc = w->w_fc; p.bfc = w->b_fc;
  p.wpack = w->wpack;
  p.g = io->g; p.m = io->m; p.v = io->v; p.st_prev = io->st_prev; p.dx_next = io->dx_next;
  p.carry_in = io->carry_in; p.carry_out = io->carry_out; p.act1 = io->act1; p.dz1 = io->dz1;
  p.act2 = io->act2; p.dz2 = io->dz2; p.h2o = io->h2; p.dd = io->dd; p.feats = io->feats; p.du = io->du;
  p.dg = io->dg;
  if (io->dg && cfg->preprocess == L2O_PRE_FC_ELU)
    return fail(L2O_ERR_UNSUPPORTED, "l2o_cwlstm_bwd_step: the input adjoint (dg) is implemented for the DM nets (identity / LogAndSign)");
  {
    const int pre_ = cfg->preprocess;
    const long P_ = cfg->n_layers == 0 ? 2 : (pre_ == L2O_PRE_FC_ELU ? kH : (pre_ == L2O_PRE_LOGSIGN ? 2 : 1));
    const long K1_ = cfg->n_layers == 0 ? 2 : P_ + kH;
    const long as = (long)io->a_stride, bs = (long)io->b_stride;
    p.s_act1 = as ? as : K1_; p.s_act2 = as ? as : 2 * kH; p.s_h2 = as ? as : kH; p.s_feats = as ? as : 2;
    p.s_dz1 = bs ? bs : 4 * kH; p.s_dz2 = bs ? bs : 4 * kH; p.s_dd = bs ? bs : 1; p.s_du = bs ? bs : kH;
  }
  hipStream_t s = (hipStream_t)stream;
  const size_t N = (size_t)B * D;
  if (cfg->n_layers == 0) {
    if (cfg->kind != L2O_NET_CW || cfg->preprocess == L2O_PRE_FC_ELU)
      return fail(L2O_ERR_UNSUPPORTED, "layers=() is implemented for CoordinateWiseDeepLSTM only");
    const dim3 grid((unsigned)((N + 255) / 256));
    if (cfg->preprocess == L2O_PRE_LOGSIGN) hipLaunchKernelGGL(k_linear_bwd_step<L2O_PRE_LOGSIGN>, grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(k_linear_bwd_step<L2O_PRE_IDENTITY>, grid, dim3(256), 0, s, p);
    HIP_TRY(hipGetLastError());
    return L2O_OK;
  }
  if (!net_ok_for_mfma(cfg)) return fail(L2O_ERR_UNSUPPORTED, "l2o_cwlstm_bwd_step: only layers=(20,20) / () nets");
  if (!w->w_gates1 || !w->b_gates1 || !w->w_gates2 || !w->b_gates2 || !io->st_prev || !io->carry_in ||
      !io->carry_out || !io->dz1 || !io->act2 || !io->dz2 || !io->h2)
    return fail(L2O_ERR_ARG, "l2o_cwlstm_bwd_step: NULL LSTM buffer");
  const int pre = cfg->preprocess;
  // fast path: tile-aligned panel + the interleaved A / Bm layout -> the quad / LDS-tile kernel
  {
    const int Pq = pre == L2O_PRE_FC_ELU ? kH : (pre == L2O_PRE_LOGSIGN ? 2 : 1);
    const int K1q = Pq + kH;
    const long KA = K1q + 3 * kH + (pre == L2O_PRE_FC_ELU ? 2 : 0) + 1, KB = 8 * kH + 1 + (pre == L2O_PRE_FC_ELU ? kH : 0);
    const bool layout = io->a_stride == KA && io->b_stride == KB && io->act2 == io->act1 + K1q &&
                        io->h2 == io->act1 + K1q + 2 * kH && io->dz2 == io->dz1 + 4 * kH && io->dd == io->dz1 + 8 * kH &&
                        (pre != L2O_PRE_FC_ELU || (io->feats == io->act1 + K1q + 3 * kH && io->du == io->dz1 + 8 * kH + 1 &&
                                                   io->m && io->v && w->w_fc && w->b_fc));
    if (layout && (D % kTile == 0 || B == 1) && ((uintptr_t)io->act1 & 15) == 0 && ((uintptr_t)io->dz1 & 15) == 0 &&
        opt(L2O_OPT_BWD_KERNEL) != 2 && !io->dg) {           // (the input adjoint is emitted by the generic kernel)
      p.nseg = 1;
      p.tile_end[0] = (int)((N + kTile - 1) / kTile);
      p.seg_n[0] = (long)N;
      p.seg_d[0] = (long)N; p.seg_tpp[0] = p.tile_end[0];
      p.seg_g[0] = io->g; p.seg_m[0] = io->m; p.seg_v[0] = io->v; p.seg_st[0] = io->st_prev; p.seg_dx[0] = io->dx_next;
      p.rows_total = (long)N;
      return launch_bwd_tile(p, pre, s);
    }
  }
  const size_t lds = 0;                                   // static LDS only (the per-thread input column)
  const dim3 grid((unsigned)((N + 63) / 64)), block(64);
  if (pre != L2O_PRE_IDENTITY && pre != L2O_PRE_LOGSIGN && (!io->m || !io->v || !io->feats || !io->du || !w->w_fc || !w->b_fc))
    return fail(L2O_ERR_ARG, "l2o_cwlstm_bwd_step: RNNProp needs m, v, feats, du and the fc weights");
  with_pre(pre, [&](auto pr) { hipLaunchKernelGGL(k_cwlstm_bwd_step<decltype(pr)::value>, grid, block, lds, s, p); });
  HIP_TRY(hipGetLastError());
  return L2O_OK;
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

int l2o_reduce_fx(const float* fx_part, int32_t T1, int32_t B_local, int32_t B_global, float* fx, void* stream) {
  if (!fx_part || !fx || T1 <= 0 || B_local <= 0 || B_global < B_local)
    return fail(L2O_ERR_ARG, "l2o_reduce_fx: bad argument");
  hipLaunchKernelGGL(k_reduce_fx, dim3(T1), dim3(64), 0, (hipStream_t)stream, fx_part, (int)T1, (int)B_local,
                     1.0f / (float)B_global, fx);
  HIP_TRY(hipGetLastError());
  return L2O_OK;
}

// ---- small vector passes of the meta-gradient (csrc/l2o_vecops.h; ABI v11) ---------------------------------
int l2o_suffix_sums(const float* const* g, const float* g_final, float* out, int64_t n, int32_t T, void* stream) {
  if (!g || !g_final || !out || n <= 0 || T < 0) return fail(L2O_ERR_ARG, "l2o_suffix_sums: bad argument");
  if (T == 0) return L2O_OK;
  hipLaunchKernelGGL(k_suffix_sums, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g, g_final, out,
                     (long)n, (int)T);
  HIP_TRY(hipGetLastError());
  return L2O_OK;
}
size_t l2o_colsum_scratch_floats(int64_t batch, int32_t cols) {
  if (batch <= 0 || cols <= 0) return 0;
  return (size_t)batch * kColsumSplit * (size_t)cols;
}
int l2o_colsum(const float* A, int64_t batch, int64_t rows, int32_t cols, float* out, int32_t accumulate, float* scratch,
               void* stream) {
  if (!A || !out || !scratch || batch <= 0 || rows <= 0 || cols <= 0 || batch > 65535)
    return fail(L2O_ERR_ARG, "l2o_colsum: bad argument");
  const unsigned gx = (unsigned)((cols + 255) / 256);
  hipLaunchKernelGGL(k_colsum_part, dim3(gx, kColsumSplit, (unsigned)batch), dim3(256), 0, (hipStream_t)stream, A, (long)rows,
                     (int)cols, scratch);
  hipLaunchKernelGGL(k_colsum_final, dim3(gx, (unsigned)batch), dim3(256), 0, (hipStream_t)stream, scratch, (int)cols, out,
                     (int)accumulate);
  HIP_TRY(hipGetLastError());
  return L2O_OK;
}
int l2o_lincomb(float* out, const float* a, float ca, const float* b, float cb, const float* c, float cc, int64_t n,
                void* stream) {
  if (!out || !a || n <= 0) return fail(L2O_ERR_ARG, "l2o_lincomb: bad argument");
  hipLaunchKernelGGL(k_lincomb, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, out, a, ca, b, cb, c, cc,
                     (long)n);
  HIP_TRY(hipGetLastError());
  return L2O_OK;
}
int l2o_rnnprop_input_adjoint(const float* Bm, int64_t ldb, int32_t du_col, int32_t H, const float* w_fc, const float* g,
                              const float* m, const float* v, double pow1, double pow2, double beta1, double beta2,
                              float* dm, float* dv, float* dg, int64_t n, void* stream) {
  if (!Bm || !w_fc || !g || !m || !v || !dm || !dv || !dg || n <= 0 || H <= 0 || du_col < 0 || ldb < du_col + H)
    return fail(L2O_ERR_ARG, "l2o_rnnprop_input_adjoint: bad argument");
  RnnpropAdjArgs a;
  a.Bm = Bm; a.ldb = (long)ldb; a.du_col = du_col; a.H = H; a.w_fc = w_fc; a.g = g; a.m = m; a.v = v;
  a.om1 = (float)(1.0 - pow1); a.om2 = (float)(1.0 - pow2);
  a.b1 = (float)beta1; a.b2 = (float)beta2;
  a.omb1 = 1.0f - a.b1; a.omb2 = 1.0f - a.b2;               // (fp32, like the forward's 1 - beta)
  a.dm = dm; a.dv = dv; a.dg = dg; a.n = (long)n;
  hipLaunchKernelGGL(k_rnnprop_input_adjoint, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return L2O_OK;
}

}  // extern "C"
