// l2o_unroll_pair_loop.h -- a fragment of l2o_unroll_pair.h, NOT a header of its own: the step loop and the epilogue of the
// two-CU unroll, the text both bodies (unroll_pair_body_gather, unroll_pair_body) include behind their prologue, inside the
// function.  One text, so the two kernels cannot drift apart; two functions, so the code in front of the loop of one
// does not move the schedule of the other (profiles/r08_launch_fixed_cost.txt, section 8).  No include guard: included twice.
  f32x4 acc1[kNT], acc2[kNT];
  core.init(s, q);
  // accumulator inits of the first step (the biases).  Register form (kBiasRegs, set by the including body): the ten quads
  // are read from the staged table here, once, and the first step is armed from the same registers as every later one
  if constexpr (kBiasRegs) {
    core.hold_bias();
    core.arm(acc1, acc2);
  } else
    core.preload(acc1, acc2);
  // (both recurrent chunks -- L1H: h1(t-1) -> layer 1, L2B: h2(t-1) -> layer 2 -- are issued inside the step loop,
  //  in the window where the wave waits for its partner's partial residuals)
  PhaseClock pc;
  pc.start();

  // Step order (round 4; round 3's order and the variants measured against it: docs/DESIGN_history_r04.md 3.1b): the scaled
  // iterate goes to LDS the moment the update exists -- at the END of a step, ahead of the split of h2 (27 VALU + the
  // register copies of the loop-carried B operands sat between the update and its LDS write: ~200 cycles of the step's
  // critical path) -- and the split runs at the top of the next step UNDER the xs reads; the loss reduction runs under the
  // residual reads of the g pass; the two row partials share one swap butterfly.
  // (every q lane writes its coordinate's xs entry: the four q lanes of a coordinate hold the same bits of xv -- the
  //  network output is a quad_q_sum, whose adds meet a + b on one lane and b + a on its partner -- so the four writes
  //  agree, and the step loop carries no exec-masked region for them)
  xs[wv * kTile + c] = live ? xv * sc : 0.0f;
  const size_t hist_n = (size_t)pp.B_local * D;
  const bool pub_plain = gq < 2 && same_xcd;
  unsigned poll_salt = salt | (dead ? 0x80000000u : 0u);
#ifdef L2O_ABLATE_EXCHANGE
  poll_salt = salt | 0x80000000u;
#endif
#if L2O_PAIR_FX_PTR
  // the loss partial of (step t, this wave) lives at [(t nb + bl) 2 NWH + half NWH + wv]: a pointer that advances by one
  // step's row (round 12's open item "Cfx", round 13) instead of two scalar multiplies, adds and a shift per step.  The
  // including body chooses: the gather kernel keeps the address computed from t -- its loop's text, and so its ISA, is
  // what it was.
  float* fxp = pa.fx_half + (size_t)bl * (2 * NWH) + half * NWH + wv;
  const size_t fx_stride = (size_t)pa.nb * (2 * NWH);
#endif
  L2O_LAUNCH_MARK(4);
  const long long loop_t0 = __builtin_readcyclecounter();
  // The plain kernel ends with the loss at x_T, i.e. with the first half of a step.  That half stands once more BEHIND its
  // loop: the loop then has one exit, at its bottom, and hipcc closes it with one backward branch (with the exit in the
  // middle the structurizer gave it a second latch block: two taken branches per step and copies of the loop-carried B
  // operands in front of them).  The recording kernel keeps its exit behind the gradient at x_T.
  if constexpr (!HIST) {
    for (int t = 0; t < a.T; ++t) {
#include "l2o_unroll_pair_step_head.h"
#include "l2o_unroll_pair_step_tail.h"
    }
    {
      const int t = a.T;
#include "l2o_unroll_pair_step_head.h"
    }
  } else
  for (int t = 0;; ++t) {
#include "l2o_unroll_pair_step_head.h"
    if (t == a.T && !HIST) break;
#include "l2o_unroll_pair_step_tail.h"
  }
  L2O_LAUNCH_MARK(5);
#ifdef L2O_PROFILE_PHASES
  if (blockIdx.x == 0 && tid == 0) pc.dump(pa.ws->phases);
#endif
  if (bid == 0 && tid == 0) pa.ws->ticks = __builtin_readcyclecounter() - loop_t0;

  if (live && q == 0) {
    a.x[idx] = xv;
    if (PRE == L2O_PRE_FC_ELU) { a.m[idx] = mv; a.v[idx] = vv; }
  }
  if (tile_real) store_tile_state(s, st_tile, lane);
  if (bid == 0 && tid == 0) pa.ws->ticks_total = __builtin_readcyclecounter() - kernel_t0;
  L2O_LAUNCH_MARK(6);
  L2O_LAUNCH_MARK_LANDED(7);
#ifdef L2O_PROFILE_PHASES
  if (bid == 0 && tid == 0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) pa.ws->pad[i] = launch_marks[i];
  }
#endif
