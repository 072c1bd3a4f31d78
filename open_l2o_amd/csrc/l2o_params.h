// l2o_params.h -- the argument blocks the kernels take by value and the few helpers more than one kernel header uses.
#pragma once
#include "l2o_common.h"

using namespace l2o;   // (the kernel headers outside namespace l2o use its names unqualified)

static inline int tiles_per_problem(int64_t D) { return (int)((D + kTile - 1) / kTile); }

// ---------------------------------------------------------------------------
// kernel parameter blocks (plain structs passed by value)
// ---------------------------------------------------------------------------
struct NetParams {
  const float* wpack;
  float scale;
  float k_inv_ln2;   // ln2 / k   (LogAndSign: log(.)/k == log2(.) * ln2/k)
  float exp_k;       // fp32(e^k)
  float beta1, beta2, omb1, omb2;   // fp32(beta), fp32(1 - beta)
  int tanh_output;
};

struct ProbParams {
  int kind, B_local, D, M;
  int w_shared;      // W is one [M, D] matrix for every problem
  int hvp;           // Hessian-vector mode (l2o_problem_hvp): the residual is W xs (no y), no separable terms
  float inv_bg;      // 1 / B_global
  float l1, alpha;
  float twopi;       // 2*pi (rastrigin) or 2*3.1415926 (square_cos, DM/problems.py:989)
  const float* W;
  const float* y;
  const float* C;
  const float* x_scale;
};

typedef __attribute__((address_space(3))) void lds_void;
typedef const __attribute__((address_space(1))) void gbl_void;

struct UnrollArgs {
  NetParams np;
  ProbParams pp;
  float* x;
  float* st;
  float* m;
  float* v;
  float* fx_part;
  int T;
  float p1_hi, p1_lo, p2_hi, p2_lo;   // beta^step0 as float-float
  // optional per-step history for the meta-gradient (l2o_unroll_record): packed state BEFORE
  // step t, the gradient fed to the network at step t, RNNProp moments AFTER step t, and the
  // gradient at x_T.  All NULL for a plain unroll.
  float *hist_st, *hist_g, *hist_m, *hist_v, *hist_gfinal;
  // restart (l2o_unroll_reduce): read the iterate from x_in (x receives x_T) / start from the zero LSTM state and
  // zero moments instead of reading st, m, v -- `reset` + the first unroll in one launch, no memset / copy pass
  const float* x_in;
  int zero_state;
  long long* ticks;   // where k_unroll_lds leaves the step-loop cycle count of problem 0 (PairWs::ticks), or NULL
};

// a.b accumulated into FOUR independent partial sums (x, y, z, w lanes of `acc`): the
// chunk loop then carries 4 short dependency chains instead of one long one
__device__ __forceinline__ void dot4(const float4 a, const float4 b, float4& acc) {
#ifdef L2O_ABLATE_GEMV
  acc.x += a.x;
  return;
#endif
  acc.x = __builtin_fmaf(a.x, b.x, acc.x);
  acc.y = __builtin_fmaf(a.y, b.y, acc.y);
  acc.z = __builtin_fmaf(a.z, b.z, acc.z);
  acc.w = __builtin_fmaf(a.w, b.w, acc.w);
}
__device__ __forceinline__ float hsum4(const float4 a) { return (a.x + a.y) + (a.z + a.w); }
