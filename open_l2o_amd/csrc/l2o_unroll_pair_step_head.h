// l2o_unroll_pair_step_head.h -- a fragment of l2o_unroll_pair.h, NOT a header of its own: the first half of a step, from the
// scaled iterate to this wave's loss partial of f(x_t).  Text of l2o_unroll_pair_loop.h, which includes it inside the step loop AND
// once more behind the loop of the plain kernel (the final loss evaluation f(x_T)).  Expects `t` in scope.  No include guard.
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
      // split h2(t-1) -> chunk L2B operand, under the LDS latency (t = 0: repeats core.init); with a late chunk L2B: in the window
      if constexpr (kL2bLate == 0) core.refresh(s);
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
    // partner on the same XCD (handshake below): a PLAIN 8-byte store keeps the granule in the XCD's L2, where
    // the partner's sc1 (L1-bypassing) poll finds it; an agent-scope (sc1) store drops the line from L2
    // and the poll pays the fabric round trip (profiles: 5.55 -> 5.89 G coordinate-steps/s on config 2)
    // (the uniform choice stands OUTSIDE the lanes' mask and the agent-scope store is marked unlikely, with the asm statement
    //  that keeps it a block of its own: the confirmed pair -- the normal case -- falls through one untaken branch; as
    //  `if (same_xcd) .. else ..` inside the mask, hipcc laid both stores in line and the plain one jumped over the other)
    {
      unsigned long long* const pub = mine + par * SQ + myrow;
      if (__builtin_expect(!same_xcd, 0)) {
        asm volatile("");
        if (gq < 2) __hip_atomic_store(pub, pack_granule(part, tag), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      if (pub_plain) __hip_atomic_store(pub, pack_granule(part, tag), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
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
    // (kL2bLate MFMAs of chunk L2B are issued later -- kL2bB2 behind barrier B2, the rest by finish() under the layer-1 gates,
    //  see kPairL2bLate: the window holds the first kWinL2)
    constexpr int kL2bB2 = kL2bLate > 0 ? kPairL2bB2 : 0;
    constexpr int kWinL2 = Core::kTotal - kL2bLate;
    constexpr int kPollN = kL2bLate > 0 ? kPairPollAtLate : L2O_PAIR_POLL_AT;
    constexpr int kPollAt = kPollN < kWinL2 ? kPollN : kWinL2;   // MFMAs before the first poll load
    constexpr int kPollAt1 = kPollN > kWinL2 ? (kPollN - kWinL2 < Core::kTotal ? kPollN - kWinL2 : Core::kTotal) : 0;
    // Late chunk L2B: the window is its first kWinL2 MFMAs, chunk L1H and, in their gaps, the split of h2 -- two plain
    // instructions per gap (8 + 2 x 4 cycles of issue in the MFMA's 16); nothing of the window reads the split any more, so
    // left alone it sinks onto the dependent chain behind barrier B2.  One scheduling region: the poll load is issued by every
    // lane (lanes gq >= 2 read row 0's granule and drop it), so no exec-masked block cuts the window, and the group
    // barriers place it behind kPollN MFMAs.
    if constexpr (kL2bLate > 0) {
      core.refresh(s);
      core.template issue_l2_prev<0, kWinL2>(s, acc2);
      core.template issue_l1_prev<0, Core::kTotal>(s, acc1);
    } else {
      core.template issue_l2_prev<0, kPollAt>(s, acc2);
      if (kPollAt1 > 0) core.template issue_l1_prev<0, kPollAt1>(s, acc1);
    }
    const unsigned long long* src = theirs + par * SQ + (gq < 2 ? myrow : 0);
    unsigned long long g = 0;
    // "partner timed out" costs the straight-line step nothing: a wave that has given up (poll_salt carries bit 31, which no
    // step tag has) compares the granule against a tag that cannot match, so it leaves through the unlikely ballot branch
    // below, which is there for the spin anyway, and drops what the load returned there.  Wave-uniform and sticky: once a
    // lane of the wave has timed out, the whole wave stops waiting (its results are garbage from then on, the host reports it).
    const unsigned poll_tag = poll_salt | ((unsigned)t + 1u);
    if constexpr (kL2bLate > 0) {
#ifndef L2O_ABLATE_EXCHANGE
      g = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
      core.hold_b2();
#pragma unroll
      for (int i = 0; i < kWinL2 + Core::kTotal; ++i) {
        if (i == kPollN) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
      }
    } else {
      __builtin_amdgcn_sched_barrier(0);
#ifndef L2O_ABLATE_EXCHANGE
      if (gq < 2) g = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
      __builtin_amdgcn_sched_barrier(0);
      if (kPollAt < kWinL2) core.template issue_l2_prev<kPollAt, kWinL2>(s, acc2);
      core.template issue_l1_prev<kPollAt1, Core::kTotal>(s, acc1);
    }
    float contrib = 0.0f;
    if (gq < 2) {
      int spins = 0;
      // The spin is the exception (the first poll load usually finds the granule): a wave whose lanes all have their
      // granule skips it with ONE uniform branch, and the expectation moves the spin's exec-masked blocks out of the
      // straight-line step (the asm statement keeps the compiler from merging the two conditions back into one mask)
#ifdef L2O_ABLATE_EXCHANGE
      const bool wait = false;
#else
      const bool wait = (unsigned)(g >> 32) != poll_tag;
#endif
      if (__builtin_expect(__builtin_amdgcn_ballot_w64(wait) != 0, 0)) {
        asm volatile("");
        bool timed_out = false;
        if (poll_salt != salt) g = 0;                         // gave up earlier (or the injected fault): no partner value
        else if (wait) {
#pragma nounroll
          for (;;) {
            g = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if ((unsigned)(g >> 32) == tag) break;
            if (++spins > (1 << 20)) { timed_out = true; atomicExch(&pa.ws->status, 1u); break; }
#ifndef L2O_POLL_NOSLEEP
            __builtin_amdgcn_s_sleep(1);
#endif
          }
        }
        if (__builtin_amdgcn_ballot_w64(timed_out) != 0) poll_salt = salt | 0x80000000u;
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
      // (late chunk L2B: kL2bB2 of its MFMAs here, one per two instructions of the reduction's DPP chain, while the wave
      //  waits for the residual reads anyway)
      if constexpr (kL2bB2 > 0) core.template issue_l2_prev<kWinL2, kWinL2 + kL2bB2>(s, acc2);
      const float fw = wave_sum64(contrib);
      __builtin_amdgcn_sched_group_barrier(0x100, CH, 0);      // the DS reads, then the reduction's DPP chain
      if constexpr (kL2bB2 > 0) {
#pragma unroll
        for (int i = 0; i < kL2bB2; ++i) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
        }
      } else
      __builtin_amdgcn_sched_group_barrier(0x002, 24, 0);
      // (every lane stores: wave_sum64 leaves the same bits on all 64 lanes, so the one address gets one value and the
      //  store needs no exec-masked region -- 3 857 -> 3 813 cycles per step on config 2)
#if L2O_PAIR_FX_PTR                                                 // (the FAST body: an advancing pointer, one add per step)
      *fxp = fw;
      fxp += fx_stride;
#else
      pa.fx_half[((size_t)t * pa.nb + bl) * (2 * NWH) + half * NWH + wv] = fw;
#endif
      if constexpr (kL2bB2 > 0) __builtin_amdgcn_sched_barrier(0);    // (the groups above end here: the g pass is scheduled on its own)
    }
