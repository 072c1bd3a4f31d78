// l2o_unroll_pair_step_tail.h -- a fragment of l2o_unroll_pair.h, NOT a header of its own: the second half of a step, from the
// gradient g = W^T r through the optimizer net to the next scaled iterate.  Text of l2o_unroll_pair_loop.h, included inside the step
// loop behind l2o_unroll_pair_step_head.h, whose locals (xsv, trig, rv4v) it reads.  No include guard.
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
    float d;                                                // (re-armed below)
    if constexpr (kL2bLate > 0) d = core.template finish<false, bx::NoShadow, false, kL2bLate - kL2bB2, kL2aUnderSplit>(s, acc1, acc2, in0, in1, q, pc);
    else d = core.template finish<false, bx::NoShadow, false>(s, acc1, acc2, in0, in1, q, pc);
    // a real (uniform) branch: as a select hipcc computes the exp + rcp of tanh on every step of the nets without it.
    // Marked unlikely (a run-time field: the RNNProp nets do take it): the block moves out of line, and the nets without a
    // tanh output -- L2O-DM, the flagship -- fall through instead of jumping over it every step
    if (__builtin_expect(a.np.tanh_output != 0, 0)) {
      asm volatile("");
      d = tanhf_(d);
    }
    xv = __builtin_fmaf(d, a.np.scale, xv);
    // the next step's scaled iterate -> LDS NOW (its readers sit behind barrier B1; this step's readers of xs all
    // passed barrier B2 before any wave gets here)
    __builtin_amdgcn_sched_barrier(0);
    xs[wv * kTile + c] = live ? xv * sc : 0.0f;           // (all four q lanes, the same value: see above)
    __builtin_amdgcn_sched_barrier(0);
    // the next step's accumulator inits (the gate biases).  Register form (kPairBiasRegs): no instruction at all -- the first
    // MFMA of each chain takes its bias quad as C.  LDS form (the recording kernels, two gather instantiations): 10
    // ds_read_b128 go out HERE, in front of barrier B1.  Their latency is NOT free, as this comment said from round 4 to round
    // 13: the s_waitcnt lgkmcnt(0) in front of the barrier waits for all ten and not only for the xs write above, the four
    // waves of a CU arrive together and their 40 reads queue in front of it -- 130 cycles per step on the phase clock of
    // config 2, 100 in the step loop's counter (profiles/r14_bias_registers.txt)
    if constexpr (kBiasRegs) core.arm(acc1, acc2);
    else core.preload_unpinned(acc1, acc2);
    __builtin_amdgcn_sched_barrier(0);
    pc.mark(9);
