// l2o_unroll_pair_loop.h -- NOT a header of its own: the step loop and the epilogue of the two-CU unroll, the text both
// bodies of l2o_unroll_pair.h (unroll_pair_body_gather, unroll_pair_body) include behind their prologue, inside the
// function.  One text, so the two kernels cannot drift apart; two functions, so the code in front of the loop of one
// does not move the schedule of the other (profiles/r08_launch_fixed_cost.txt, section 8).  No include guard: included twice.
  f32x4 acc1[kNT], acc2[kNT];
  core.init(s, q);
  core.preload(acc1, acc2);                                 // accumulator inits of the first step (the biases)
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
  L2O_LAUNCH_MARK(4);
  const long long loop_t0 = __builtin_readcyclecounter();
  for (int t = 0;; ++t) {
    const float xsv = xv * sc;
    const unsigned tag = salt | ((unsigned)t + 1u);     // (T + 1 < 65 535 when salt != 0; the handshake tag ends in 0xffff)
    const int par = t & 1;
    pc.mark(0);
    // (recording: barriers that wait for LDS traffic only -- a __syncthreads() also waits for the write acknowledgement
    //  of the 5 KB of history the wave has just stored)
    if (HIST || L2O_PAIR_LDS_BARRIERS) lds_barrier(); else __syncthreads();          // B1: this half's xs complete
    pc.mark(2);
    // ---- partial residual over this half's columns: rows 2 x 16 per wave, all SQ rows per half
    float part;
    {
      float4 r0 = {0.f, 0.f, 0.f, 0.f}, r1 = {0.f, 0.f, 0.f, 0.f};
      Acc4pk r0p = {{0.f, 0.f}, {0.f, 0.f}}, r1p = {{0.f, 0.f}, {0.f, 0.f}};
      l2o::f32x4 x4v[NWH];
      lds_load_f4<NWH>(x4v, xsq);
      core.refresh(s);                     // split h2(t-1) -> chunk L2B operand, under the LDS latency (t = 0: repeats core.init)
      __builtin_amdgcn_sched_group_barrier(0x100, NWH, 0);     // the DS reads first ...
      __builtin_amdgcn_sched_group_barrier(0x002, 48, 0);      // ... then the split's VALU block, then the FMAs
#pragma unroll
      for (int m = 0; m < NWH; ++m) {
        if (kPk) { dot4pk(wrq[0][m], x4v[m], r0p); dot4pk(wrq[1][m], x4v[m], r1p); }
        else { dot4v(wr[0][m], x4v[m], r0); dot4v(wr[1][m], x4v[m], r1); }
      }
      // both row partials through ONE butterfly: the 16-lane swap pairs row groups (0,1) and (2,3) of p0 AND p1 at once,
      // the 32-lane swap finishes both; odd lane groups end with the p1 sum, even ones with the p0 sum -- the lanes
      // that publish them.  Same additions in the same order as two quad_q_sum calls (bit-identical), 5 instead of 13
      // instructions and one dependent swap chain instead of two.
      const float h0 = kPk ? hsum4pk(r0p) : hsum4(r0), h1 = kPk ? hsum4pk(r1p) : hsum4(r1);
      const u32x2 sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(h0), __float_as_uint(h1), false, false);
      part = xor32_add(__uint_as_float(sw[0]) + __uint_as_float(sw[1]));
    }
    // ---- exchange the partial sums (one granule per row), the previous-h2 matrix work covers the latency
    if (gq < 2) {
      // partner on the same XCD (handshake below): a PLAIN 8-byte store keeps the granule in the XCD's L2, where
      // the partner's sc1 (L1-bypassing) poll finds it; an agent-scope (sc1) store drops the line from L2
      // and the poll pays the fabric round trip (profiles: 5.55 -> 5.89 G coordinate-steps/s on config 2)
      if (same_xcd)
        __hip_atomic_store(mine + par * SQ + myrow, pack_granule(part, tag), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      else
        __hip_atomic_store(mine + par * SQ + myrow, pack_granule(part, tag), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // (round 5) cos / sin of 2 pi x s for the rastrigin / square_cos terms: computed HERE, in front of the recurrent MFMAs
    // whose issue they interleave with, instead of behind the partner poll (the loss term) and inside the g pass (the
    // gradient term) -- both on the step's critical path.  Same function, same argument: bit-identical results.
    l2o::SinCos trig = {0.0f, 1.0f};
    if (kCos) trig = l2o::sincos_f(kTwoPi * xsv);
    pc.mark(3);                                             // partial r + publish
    // 30 MFMAs (L2B) give the partner time to publish; the first poll load goes out THEN and its L2 round trip
    // is covered by the other 30 MFMAs (L1H) -- in program order, a single wave issues in order
#ifndef L2O_PAIR_POLL_AT
#define L2O_PAIR_POLL_AT 20   // = after chunk L2B.  Packed chunks (20 MFMAs): 5 -> 7.72, 10 -> 7.86, 15 -> 7.95, 20 -> 8.02, 30 -> 7.98 G (config 2)
#endif
    constexpr int kPollAt = L2O_PAIR_POLL_AT < Core::kTotal ? L2O_PAIR_POLL_AT : Core::kTotal;   // MFMAs before the first poll load
    constexpr int kPollAt1 = L2O_PAIR_POLL_AT > Core::kTotal ? L2O_PAIR_POLL_AT - Core::kTotal : 0;
    core.template issue_l2_prev<0, kPollAt>(s, acc2);
    if (kPollAt1 > 0) core.template issue_l1_prev<0, kPollAt1>(s, acc1);
    const unsigned long long* src = theirs + par * SQ + (gq < 2 ? myrow : 0);
    unsigned long long g = 0;
#ifdef L2O_ABLATE_EXCHANGE
    dead = true;
#endif
    __builtin_amdgcn_sched_barrier(0);
    if (gq < 2 && !dead) g = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_sched_barrier(0);
    if (kPollAt < Core::kTotal) core.template issue_l2_prev<kPollAt, Core::kTotal>(s, acc2);
    core.template issue_l1_prev<kPollAt1, Core::kTotal>(s, acc1);
    float contrib = 0.0f;
    if (gq < 2) {
      int spins = 0;
      // The spin is the exception (the first poll load usually finds the granule): a wave whose lanes all have their
      // granule skips it with ONE uniform branch, and the expectation moves the spin's exec-masked blocks out of the
      // straight-line step (the asm statement keeps the compiler from merging the two conditions back into one mask)
      const bool wait = !dead && (unsigned)(g >> 32) != tag;
      if (__builtin_expect(__builtin_amdgcn_ballot_w64(wait) != 0, 0)) {
        asm volatile("");
        if (wait) {
#pragma nounroll
          for (;;) {
            g = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if ((unsigned)(g >> 32) == tag) break;
            if (++spins > (1 << 20)) { dead = true; atomicExch(&pa.ws->status, 1u); break; }
#ifndef L2O_POLL_NOSLEEP
            __builtin_amdgcn_s_sleep(1);
#endif
          }
        }
      }
      const float r = (part + __uint_as_float((unsigned)g)) - myy;   // rows >= M: W row and y are zero -> r == 0
      rs[myrow] = r;
      if (row_counted) contrib = coef * r * r;
    }
    if (live && q == 0) {
      if (KIND == L2O_PROB_LASSO) contrib += pp.l1 * __builtin_fabsf(xsv);
      if (kCos) contrib += pp.alpha - pp.alpha * cj * trig.c;
    }
    // the state BEFORE this step's update, for the meta-gradient.  Stored HERE: the poll above is this step's last wait
    // on vmcnt (loads and stores retire in order), the barriers of the recording kernel wait for LDS traffic only, so
    // the 5 KB per wave drain under the gate blocks instead of sitting in front of a wait (recording kernel / plain
    // kernel time at config-2 size: 1.26 -> 1.22, profiles/archive_r01_r03/r03t_*)
    // (non-temporal stores for these records: 240 -> 338 us per recording unroll -- they stall the store path)
    if (HIST && t < a.T && tile_real)
      store_tile_state(s, a.hist_st + ((size_t)t * pp.B_local * tpp + (size_t)b * tpp + tile_in_prob) *
                                          kStateFloatsPerTile, lane);
    pc.mark(1);                                             // previous-h2 MFMAs + partner poll
    if (HIST || L2O_PAIR_LDS_BARRIERS) lds_barrier(); else __syncthreads();          // B2: rs complete
    pc.mark(4);
    // this wave's share of f_b(x_t): reduced AFTER the barrier (the DPP chain fills the LDS latency of the g
    // pass instead of sitting in front of the barrier) and written straight to HBM -- no LDS round, no
    // thread-0 sum on the step's critical path; k_combine_halves adds the 2 x NWH partials per (step, problem)
    // (round 4: the residual reads of the g pass go out FIRST; the reduction's DPP chain and the store fill their latency --
    //  in round 3's ISA the chain sat in front of reads that carried their own wait)
    l2o::f32x4 rv4v[CH];
    lds_load_f4<CH>(rv4v, rsq);
    {
      const float fw = wave_sum64(contrib);
      __builtin_amdgcn_sched_group_barrier(0x100, CH, 0);      // the DS reads, then the reduction's DPP chain
      __builtin_amdgcn_sched_group_barrier(0x002, 24, 0);
      // (every lane stores: wave_sum64 leaves the same bits on all 64 lanes, so the one address gets one value and the
      //  store needs no exec-masked region -- 3 857 -> 3 813 cycles per step on config 2)
      pa.fx_half[((size_t)t * pa.nb + bl) * (2 * NWH) + half * NWH + wv] = fw;
    }
    if (t == a.T && !HIST) break;

    // ---- g = W^T r for this wave's 16 coordinates ------------------------------
    // all CH residual reads are issued back to back (hipcc serialises them on one register
    // quad otherwise: CH x LDS latency on the critical path), one wait, then the FMAs
    constexpr bool kPkG = L2O_GEMV_PK_G != 0;
    float4 gacc4 = {0.f, 0.f, 0.f, 0.f};
    Acc4pk gaccp = {{0.f, 0.f}, {0.f, 0.f}};
#pragma unroll
    for (int m = 0; m < CH; ++m) {
      if (kPkG) dot4pk(wtq[m], rv4v[m], gaccp);
      else dot4v(wt[m], rv4v[m], gacc4);
    }
    float gv = quad_q_sum(kPkG ? hsum4pk(gaccp) : hsum4(gacc4));
    if (KIND == L2O_PROB_SQUARE_COS) gv *= 2.0f;            // only the ||wx-y||^2 part carries the 2
    if (KIND == L2O_PROB_LASSO) gv += pp.l1 * (xsv > 0.f ? 1.f : (xsv < 0.f ? -1.f : 0.f));
    if (kCos) gv += kTwoPi * pp.alpha * cj * trig.s;
    gv = live ? gv * cg * sc : 0.0f;
    if (HIST && live && q == 0) {
      if (t < a.T) a.hist_g[(size_t)t * hist_n + idx] = gv;
      else a.hist_gfinal[idx] = gv;
    }
    if (HIST && t == a.T) break;                            // (history mode: the gradient at x_T was still needed)

    float in0, in1;
    if (PRE == L2O_PRE_FC_ELU) {
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
    float d = core.template finish<false, bx::NoShadow, false>(s, acc1, acc2, in0, in1, q, pc);   // (re-armed below)
    if (a.np.tanh_output) {                                 // a real (uniform) branch: as a select hipcc computes the
      asm volatile("");                                      // exp + rcp of tanh on every step of the nets without it
      d = tanhf_(d);
    }
    xv = __builtin_fmaf(d, a.np.scale, xv);
    // the next step's scaled iterate -> LDS NOW (its readers sit behind barrier B1; this step's readers of xs all
    // passed barrier B2 before any wave gets here)
    __builtin_amdgcn_sched_barrier(0);
    xs[wv * kTile + c] = live ? xv * sc : 0.0f;           // (all four q lanes, the same value: see above)
    __builtin_amdgcn_sched_barrier(0);
    // the next step's accumulator inits (the gate biases: 10 ds_read_b128) go out HERE: their latency overlaps the wait
    // for barrier B1, which drains this wave's LDS queue anyway
    core.preload_unpinned(acc1, acc2);
    __builtin_amdgcn_sched_barrier(0);
    pc.mark(9);
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
