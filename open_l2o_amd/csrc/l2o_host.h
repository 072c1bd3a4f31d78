// l2o_host.h -- host code only: what the translation units of libl2o_hip.so (l2o_core.hip, l2o_unroll.hip, l2o_bwd.hip,
// l2o_mlp.hip, l2o_nets.hip, l2o_confocal.hip, l2o_twin.hip) share on the host side of the C ABI of include/l2o_abi.h --
// the error text, the launch helpers, the call-scoped option word, the device queries and the descriptor ->
// kernel-parameter conversions.
// Everything here is `inline` (C++17: functions AND variables), so the library holds exactly one g_err, t_optw, ... however
// many units include this; a helper with callers in one unit only lives in that unit as a `static`.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "l2o_common.h"
#include "l2o_params.h"

using namespace l2o;

#pragma GCC visibility push(hidden)   // internal to the library: nothing here is exported (or interposable)

// ---------------------------------------------------------------------------
// error plumbing
// ---------------------------------------------------------------------------
inline thread_local char g_err[512] = "";
// which kernel form the last l2o_unroll* / l2o_mlp_unroll* call of this thread launched (l2o_last_unroll_form, ABI v12):
// L2O_FORM_* | dispatches << 8.  Diagnostic only, like g_err -- no launch depends on it.
inline thread_local int g_last_form = 0;
// ... and which instantiation of that template (l2o_last_unroll_variant: the L2O_VARIANT_* fields of include/l2o_abi.h; the
// five unroll launchers set it right after note_form, every other form leaves the 0 note_form stores)
inline thread_local int g_last_variant = 0;
inline void note_form(int form, int dispatches = 1) { g_last_form = form | (dispatches << 8); g_last_variant = 0; }
inline void note_variant(int ch, bool hist, bool exact, bool fast, int kr, int nv) {
  g_last_variant = L2O_VARIANT(ch, hist ? 1 : 0, exact ? 1 : 0, fast ? 1 : 0, kr, nv);
}

inline int fail(int code, const char* fmt, ...) {
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
inline auto with_pre(int pre, F&& f) {
  switch (pre) {
    case L2O_PRE_IDENTITY: return f(std::integral_constant<int, L2O_PRE_IDENTITY>{});
    case L2O_PRE_LOGSIGN: return f(std::integral_constant<int, L2O_PRE_LOGSIGN>{});
    default: return f(std::integral_constant<int, L2O_PRE_FC_ELU>{});
  }
}
// a launch with `lds` bytes of dynamic LDS: raise the kernel's limit (every time: no host-side state), launch, check
template <class K, class... A>
inline int launch(K fn, dim3 grid, dim3 block, size_t lds, hipStream_t s, const A&... args) {
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(fn, grid, block, lds, s, args...);
  HIP_TRY(hipGetLastError());
  return L2O_OK;
}

// ---------------------------------------------------------------------------
// descriptors -> kernel parameters
// ---------------------------------------------------------------------------
inline bool net_ok_for_mfma(const l2o_net_cfg* c) {
  if (c->n_layers != 2 || c->hidden != kH) return false;
  if (c->kind == L2O_NET_CW) return c->preprocess == L2O_PRE_IDENTITY || c->preprocess == L2O_PRE_LOGSIGN;
  if (c->kind == L2O_NET_RNNPROP) return c->preprocess == L2O_PRE_FC_ELU;
  return false;
}

inline NetParams make_net_params(const l2o_net_cfg* c, const float* wpack) {
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

inline ProbParams make_prob_params(const l2o_problem* p) {
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

// float-float split of base^k computed in double
inline void pow_ff(double base, int k, float* hi, float* lo) {
  const double p = std::pow((double)(float)base, (double)k);
  *hi = (float)p;
  *lo = (float)(p - (double)*hi);
}

// ---------------------------------------------------------------------------
// options: A/B switches between kernels that compute the same thing.  The library keeps NO option state: every call
// carries its switches in the caller's own structs -- l2o_net_cfg.options (L2O_OPTW(option, value) words OR-ed
// together; 0 = every default), l2o_problem.flags (L2O_PROB_FG_TWO_PASS) and l2o_mlp.flags (L2O_MLP_GENERIC).  An entry
// point copies the word into a call-scoped thread-local (OptScope) that the launch helpers read through opt().
// ---------------------------------------------------------------------------
inline constexpr int64_t kOptDefault[L2O_OPT_COUNT_] = {
    /* L2O_OPT_PAIR */ 1, /* L2O_OPT_PAIR_PLAIN_STORES */ 1, /* L2O_OPT_UNROLL_CU */ 1,
    /* L2O_OPT_FG_TWO_PASS */ 0, /* L2O_OPT_MLP_GENERIC */ 0, /* L2O_OPT_BWD_BLOCKS */ 0,
    /* L2O_OPT_BWD_KERNEL */ 0, /* L2O_OPT_MLP_UNROLL */ 1, /* L2O_OPT_MLP_XCD_WAVES */ 0, /* L2O_OPT_EXACT_GATES */ 0,
    /* L2O_OPT_WPACK_NO_CLEAR */ 0, /* L2O_OPT_MLP_HIER */ 1, /* L2O_OPT_ONE_LDS */ 1, /* L2O_OPT_PAIR_FAST_LOAD */ 1};
inline thread_local uint64_t t_optw = 0;
struct OptScope {
  uint64_t saved;
  explicit OptScope(uint64_t w) : saved(t_optw) { t_optw = w; }
  ~OptScope() { t_optw = saved; }
};
inline uint64_t cfg_optw(const l2o_net_cfg* cfg) { return cfg ? cfg->options : 0; }
inline int64_t opt(int o) {
  if (o == L2O_OPT_BWD_BLOCKS) return (int64_t)((t_optw >> 48) & 0xfffu);      // a count: its own 12-bit field
  const unsigned nib = (unsigned)(t_optw >> (4 * L2O_OPT_FIELD_(o))) & 0xfu;
  return (nib & 8u) ? (int64_t)(nib & 7u) : kOptDefault[o];
}

// ---------------------------------------------------------------------------
// device queries
// ---------------------------------------------------------------------------
// CUs of the device the call runs on (the stream's device; the current device for the null stream).
// Immutable hardware facts cached per device ordinal -- not launch state.
inline int device_cu_count(hipStream_t s) {
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

inline int device_ordinal(hipStream_t s) {
  int dev = -1;
  if (s == nullptr || hipStreamGetDevice(s, &dev) != hipSuccess || dev < 0) {
    if (hipGetDevice(&dev) != hipSuccess) return -1;
  }
  return dev;
}
// measured co-resident one-per-CU workgroups per device (l2o_coresident_workgroups); 0 = never probed
inline std::atomic<int> g_measured_cus[64];

// CUs on which workgroups of a launch on stream `s` can be resident AT THE SAME TIME -- what the kernels with
// inter-workgroup exchanges (two-CU unroll, l2o_mlp_unroll) size their grids against:
//   the device's CU count (reflects ROC_GLOBAL_CU_MASK and the partition mode), the stream's own CU mask
//   (hipExtStreamCreateWithCUMask; 0.3 us per query), and the MEASURED capacity where the caller ran the probe
//   (restrictions below HIP, e.g. HSA_CU_MASK: the device still reports every CU).
inline int coresident_cus(hipStream_t s) {
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

#pragma GCC visibility pop
