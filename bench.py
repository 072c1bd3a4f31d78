#!/usr/bin/env python
"""bench.py -- unroll-steps/sec of the L2O inner unroll loop on MI355X, through the
product API (open_l2o_amd.util.get_config -> MetaOptimizer.meta_loss -> one unroll per step).

Default workload (BASELINE.json configs[1]): L2O-DM (CoordinateWiseDeepLSTM, layers (20,20),
identity preprocess -- what util.get_config("quadratic") builds) on Quadratic d=128,
batch=128 per GPU, T=100 optimizer steps per unroll, fp32, synthetic data
(W, y ~ U[0,1), x0 ~ N(0, 0.01^2) as DM/problems.py:84-96).  The optimizer is the TRAINED one committed
under tests/golden/trained/ (meta-trained on the MI355X with scripts/train_dm.py / train_rnnprop.py, command
lines in tests/golden/trained/README.md): its loss FALLS over the unroll, the regime the reference runs in.
Without a trained file for the workload (config 5, --net dm_logsign) the weights are Sonnet-default random
draws with the output Linear x0.1 and the line says "untrained" (that trajectory diverges).

One UNROLL = what the reference does between `reset` and the last `fx`: a FRESH problem instance
(one of a ring of --instances pre-sampled instances already resident in HBM) -> rewind x / LSTM state -> T x {f(x), grad f,
LSTM optimizer step, x += delta} -> f(x_T) -> per-step loss reduction (-> all-reduce of the T+1 partial losses
over ranks when N > 1).  One bench "step" = --unrolls-per-step consecutive unrolls (default per config, so that
20 steps time >= --min-timed-seconds = 1 s of GPU work: config 2 -> 278 unrolls per step, whatever --steps says;
`sustained` compares the first and the last tenth of the timed steps); value counts every one of them.  --steps K times
exactly K steps and ms_per_step is one of them.  Inputs are resident in HBM when the timed region starts; nothing is
copied to the host inside it.  --dump-outputs DIR writes what the last timed unroll computed (seeded inputs: the same
arrays on every run with the same arguments).

    python bench.py --gpus N --steps K --warmup W     (N > 1 without WORLD_SIZE: re-launches itself under
                                                       torch.distributed.run, one rank per GPU, 127.0.0.1)
    python bench.py --config 3 --steps 5              (the other BASELINE configs: --config 3 / 4 / 5)
    python bench.py --gpus 8 --scaling strong         (the global batch stays what --batch says)
    python bench.py --full ...                        (everything beyond the headline figure: see below)

Prints ONE JSON line (rank 0).  value = coordinate-steps per second, whole job:
    sum over ranks of B_local * D * T * steps / wall_time (max over ranks).
--scaling weak (default): every GPU holds `--batch` problems of a global batch batch*N;
--scaling strong: the global batch is `--batch`, every GPU holds batch/N of it.  Either way the
loss mean is over the global batch (DM/problems.py:99) and the only collective is the all-reduce
of T+1 floats per unroll.

A plain run does only what the headline needs: set up, warm up, time the steps, write --dump-outputs, print the line.
--full adds what takes runs of its own: the replays of one instance behind `roofline` and `value_replayed_problem`,
the device-copy figure, the bounded cpu_baseline (the oracle is imported by those legs only) and the `also` block.
For N > 1 "also" carries the config-2 strong-scaling run (global batch 128) and the config-4 run (Rastrigin d=100,
global batch 1024 sharded over the N GPUs) measured in the same job.  For N = 1 "also" carries compact lines of the
OTHER BASELINE configurations measured in the same process right after the primary one: config 3, config 4 on one GPU,
config 4's shard of 8 (128 of the 1024 problems, 1/B_global = 1/1024, no communication: --emulate-world 8 on its own)
and config 5 -- each with value, kernel_ms, roofline.frac and a bounded cpu_baseline (--no-also skips them; budget
<= 90 s).
"""
import argparse
import glob
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12          # MI355X_MICROARCH.md: 8 TB/s spec
FP32_PEAK = 157.3e12
N_SIMD = 256 * 4           # 256 CUs x 4 SIMDs
STEPS_PER_MIN_TIMED = 20   # the default --unrolls-per-step makes this many steps (the default --steps) >= --min-timed-seconds
DUMP_BYTES = 64 * 10 ** 6 - 64 * 1024   # --dump-outputs: array data in all (the rest of 64 MB is left to the .npy headers)
PARITY_PIN = ("reference KATs (tests/golden/reference_kats.json: meta_test / problems_test / preprocess_test / "
              "networks_test values) + torch.nn.LSTMCell for the LSTM cell; dm-sonnet 1.11 / TF 1.14 are absent, so "
              "the cell's gate order and forget bias are pinned to Sonnet's published source, not to a reference run")


def alg_bytes_per_coord_step(problem, net, D, M):
    """x r+w + LSTM state r+w (+ RNNProp m, v r+w) + the optimizee's matrix
    streamed for the forward and for the gradient (the step-granular contract figure)."""
    base = 8 + 640 + (16 if net == "rnnprop" else 0)
    if problem == "quadratic":
        return base + 8 * D + 4
    if problem == "lasso":
        return base + 8 * M + 4.0 * M / D
    if problem == "mnist":                       # minibatch [M x 784] read for forward and for gw1
        return base + 2.0 * M * 784 * 4 / D
    return base + 8 * D + 8                      # rastrigin


def alg_bytes_lasso_shared(net, B, D, M):
    """SURVEY.md 8(d), shared-A variant: the matrix is streamed twice per step for the WHOLE batch."""
    return 8 + 640 + (16 if net == "rnnprop" else 0) + 8.0 * M / B + 4.0 * M / D


def alg_flops_per_coord_step(problem, net, D, M):
    lstm = {"dm": 9800, "dm_logsign": 9960, "rnnprop": 12920 + 15}[net]
    if problem == "mnist":
        return lstm + 4 * M                      # 2 x 2 x batch MACs per weight
    return lstm + 4 * (M if problem == "lasso" else D)


# ---- work-based roofline figure --------------------------------------------------------------
# Measured ISSUE cost in shader cycles of one wave64 instruction per class, one wave per SIMD, independent operands
# (scripts/microbench/valu_issue_cost.hip; profiles/archive_r04/r04c_valu_issue_cost.txt).  MFMA: its issue slot; the matrix pipe's
# own occupancy (16 cycles per v_mfma_f32_16x16x32_bf16) is reported separately as mfma_pipe_floor.
# Measured (r04c): v_fma_f32 / v_pk_fma_f32 / v_cvt_pk_bf16_f32 5.2-5.3 cycles (ONE wave per SIMD issues a plain VALU
# instruction every ~5.3 cycles, not every 4: the 4-cycle rate needs a second wave), v_exp_f32 / v_rcp_f32 8.5,
# v_permlane*_swap 10.3 (counted as plain: 6 per step), v_mfma_f32_16x16x32_bf16 back to back 17.9 (the pipe).
ISSUE_COST = {"valu": 5.26, "trans": 8.51, "mfma": 5.26}
MFMA_PIPE_CYCLES = 17.89
# What the SIMD's PIPES take per instruction once two or more waves feed them (scripts/microbench/two_wave_issue.hip,
# profiles/archive_r04/r04w_two_wave_issue.txt: 1.220 / 3.496 / 6.744 ns per instruction per SIMD, x 2.4 GHz like every cycle figure
# here): a plain VALU instruction 2.93 cycles (one wave alone: 5.6), a transcendental 8.39 (the same pipe: their times add),
# the bf16 MFMA 16.2 on its own pipe (overlaps another wave's VALU).  The floor of the two-waves-per-SIMD kernels.
PIPE_COST = {"valu": 2.93, "trans": 8.39, "mfma": 16.2}
# The HARDWARE GUIDE's peak for the same pipe (MI355X_MICROARCH.md, throughput table: plain f32 VALU 2 cycles per wave64
# instruction per SIMD, transcendentals ~8): the roofline the judge prices against.
# frac_guide_peak = work model x these / measured cycles -- `roofline.frac` IS this figure since round 6 (config 2: 0.26);
# the variant at the pipe rates measured on this part (PIPE_COST: 0.32) stays next to it as frac_measured_pipe.
GUIDE_COST = {"valu": 2.0, "trans": 8.0}


def work_model(problem, net, D, M):
    """The MINIMAL instruction counts of ONE tile-step (16 coordinates, one wave) of the fused unroll, by class -- a
    statement about the algorithm, not a count of what the compiler emitted (the ISA executes ~30 % more plain VALU:
    register copies, masks, address arithmetic), so the figure cannot be raised by executing more instructions:
      GEMV     two passes over the problem's matrix slice owned by the wave: M*D/(tiles per problem * 64 lanes) FMAs each
               (two-CU form, d = 128: 32 + 32), + the in-lane / cross-lane reductions and the residual / scaling (26)
      inputs   the gradient features into the 20 layer-1 gate rows of the lane's five units: 10 packed FMAs per feature
      gates    two layers x five units per lane: 8 transcendentals (5 v_exp + 3 v_rcp) and 6 plain (packed pairs) each
      split    two 5-vectors -> three bf16 levels: 27 each
      MFMA     60 (packed DM form) / 90 (6-product form) / 120 (RNNProp, 4 chunks)
      rest     output Linear 9, update + scaled iterate 3, loss terms + wave reduction 15 (+ RNNProp inputs 20)"""
    rn = net == "rnnprop"
    tiles = max(1, (D + 15) // 16)
    if problem == "mnist":
        gemv = 2 * 16 + 26                                   # gradient of the lane's coordinate: 16 samples x 4 q lanes
    else:
        rows = M if problem == "lasso" else D
        gemv = 2 * int(round(rows * D / (tiles * 64.0))) + 26
    feats = 2 if net == "dm_logsign" else (0 if rn else 1)
    plain = gemv + 10 * feats + 2 * 5 * 6 + 2 * 27 + 27 + (20 + 27 + 20 if rn else 0)
    trans = 2 * 5 * 8 + (2 if rn else 0) + (20 if rn else 0)     # (+ tanh output, + the ELU of the 20 input features)
    mfma = 120 if rn else 60
    return {"valu_plain": plain, "transcendental": trans, "mfma": mfma}


def work_block(case, issue, args, clock_hz):
    """The work-based figures of a VALU-bound fused kernel.
    cycles_per_step: shader-clock cycles one SIMD spends per optimizer step = the LIVE kernel time of this run (HIP events
        around replays of one instance: the unroll kernel + its epilogue) x clock / (chunk launches x rounds of problems
        per CU x (T + 0.3): the T + 1-st loss evaluation is ~1/3 of a step).  clock = GRBM_GUI_ACTIVE / kernel time of the
        PMC passes when counters of this build exist, else the nominal 2.4 GHz.  The conservative denominator: launch
        ramp, the slowest workgroup and the epilogue launch are all charged to the steps.
    cycles_per_step_in_kernel / _loop: the same quantity COUNTED inside the kernel (s_memtime of wave 0 of workgroup 0 from
        kernel entry to its last store, workspace bytes 24..31; the step loop alone, bytes 16..23) -- no clock assumption;
        frac_in_kernel_cycles / frac_step_loop are the fractions over those.
    pipe_floor_cycles_per_step: the STATED minimal instruction counts of the tile-steps that SIMD does per step
        (bench.py: work_model; 1 tile per SIMD for the one-wave kernels, 2 for k_unroll_lds) x the PIPE time per
        instruction class (plain VALU 2.93, transcendental 8.39 cycles: two_wave_issue.hip) -- what the SIMD's VALU pipe
        could retire them in.  frac = floor / measured: the roofline fraction of the line.
    issue_cost_frac (one-wave kernels): the same counts x the SINGLE-WAVE issue costs (5.26 / 8.51 / 5.26 for the MFMA
        slot) / measured -- the share of the step ONE wave's issue port needs; named secondary."""
    name = case["kernel"]
    T = case["T"]
    if not case["fused"] and "k_mlp_" not in name:
        return None
    if case["hbm_bound"]:
        return None
    two_waves = "k_unroll_lds" in name
    xcd = "k_mlp_xcd" in name                            # one optimizee instance per XCD: 32 tiles per CU, two waves per SIMD
    tiles_per_simd = 8 if xcd else (2 if two_waves else 1)
    wm = work_model(args.problem, args.net, case["D"], case["Mrows"])
    per_tile_pipe = wm["valu_plain"] * PIPE_COST["valu"] + wm["transcendental"] * PIPE_COST["trans"]
    dispatches = float(case.get("dispatches", 1))
    rounds = -(-case["B"] // max(1, case.get("n_cus", 256))) if two_waves else 1
    cyc_time = case["kern_ms"] * 1e-3 * clock_hz / (dispatches * rounds * (T + 0.3))
    ticks = case.get("loop_ticks")                       # (step loop, kernel entry to exit) of wave 0 of workgroup 0
    cyc = cyc_time
    floor = tiles_per_simd * per_tile_pipe
    guide_floor = tiles_per_simd * (wm["valu_plain"] * GUIDE_COST["valu"] + wm["transcendental"] * GUIDE_COST["trans"])
    out = {"cycles_per_step": cyc, "cycles_source": "kernel_ms_avg (live HIP events) x clock_hz", "clock_hz": clock_hz,
           "tiles_per_simd": tiles_per_simd, "work_model_instructions_per_tile_step": wm,
           "guide_cost_cycles": dict(GUIDE_COST), "guide_floor_cycles_per_step": guide_floor,
           "frac_guide_peak": guide_floor / cyc,
           "pipe_cost_cycles": dict(PIPE_COST), "pipe_floor_cycles_per_step": floor,
           "mfma_pipe_cycles_per_step": tiles_per_simd * wm["mfma"] * PIPE_COST["mfma"],
           "frac_measured_pipe": floor / cyc}
    if ticks:
        out.update(cycles_per_step_in_kernel=ticks[1] / (T + 0.3), frac_in_kernel_cycles=guide_floor * (T + 0.3) / ticks[1],
                   cycles_per_step_loop=ticks[0] / (T + 0.3), frac_step_loop=guide_floor * (T + 0.3) / ticks[0],
                   in_kernel_cycles_source="s_memtime of wave 0 of workgroup 0: kernel entry to exit (workspace bytes 24..31), "
                                           "the step loop alone (bytes 16..23)")
    if not two_waves and not xcd:
        issue_floor = (wm["valu_plain"] * ISSUE_COST["valu"] + wm["transcendental"] * ISSUE_COST["trans"] + wm["mfma"] * ISSUE_COST["mfma"])
        out.update(issue_cost_cycles=dict(ISSUE_COST), issue_floor_cycles_per_step=issue_floor, issue_cost_frac=issue_floor / cyc)
    if issue is not None and issue.get("insts_valu") and issue.get("waves"):
        out["valu_insts_per_tile_step"] = issue["insts_valu"] / issue["waves"] / (T + 0.3) / max(1, rounds)
    return out


def cpu_baseline(problem, net, arrays, weights, x0, T, max_seconds=20.0, B_global=None, numpy_leg=True, gpu_fx_T=None):
    """The reference path restated for the CPU (oracle/, test infrastructure), timed on this
    host's cores on the SAME inputs (whole unrolls, bounded to ~max_seconds): the plain-C +
    OpenMP port (oracle/l2o_oracle.c, one problem per thread) is the reported baseline; the
    NumPy oracle (multi-threaded BLAS gate matmuls) is timed once next to it for reference."""
    import oracle as O
    from oracle.c_oracle import c_unroll
    cfg = {"dm": O.DM_IDENTITY, "dm_logsign": O.DM_LOGSIGN, "rnnprop": O.RNNPROP}[net]
    B, M, D = arrays["W"].shape
    kw = {} if B_global in (None, B) else {"B_global": int(B_global)}
    c_unroll(problem, cfg, weights, arrays, x0, 2, **kw)          # warm-up (thread pool, page faults)
    t0 = time.perf_counter()
    n = 0
    while True:
        fx, _, _, _, _, threads = c_unroll(problem, cfg, weights, arrays, x0, T, **kw)
        n += 1
        if time.perf_counter() - t0 > max_seconds or n >= 20:
            break
    dt = time.perf_counter() - t0
    out = {"value": B * D * T * n / dt, "unit": "coordinate-steps/s", "cores": int(threads),
           "host_cpus": os.cpu_count(), "kind": "port",
           "sample": "%d full unroll(s) of the same workload and inputs (C99+OpenMP port oracle/l2o_oracle.c, "
                     "%s/%s B=%d D=%d T=%d), %.1f s" % (n, net, problem, B, D, T, dt), "fx_T": float(fx[-1])}
    if gpu_fx_T is not None and abs(gpu_fx_T - float(fx[-1])) > 1e-5 * max(abs(float(fx[-1])), 1e-30):
        # The GPU's final loss is further than 1e-5 from the CPU port's: how far is the CPU port from ITSELF when x_0 moves by
        # one ulp?  (A converged RNNProp-on-Lasso trajectory is chaotic -- sign(x) in the l1 term, +-0.01 tanh steps: DESIGN.md
        # 4 -- so no implementation, this port included, holds 1e-5 on fx_T there; the number says how much of the
        # difference is the problem's own sensitivity.)
        x1 = np.nextafter(np.asarray(x0, np.float32), np.float32(np.inf), dtype=np.float32)
        fx1 = c_unroll(problem, cfg, weights, arrays, x1, T, **kw)[0]
        out["oracle_self_sensitivity"] = abs(float(fx1[-1]) - float(fx[-1])) / max(abs(float(fx[-1])), 1e-30)
        out["oracle_self_sensitivity_note"] = ("relative change of the CPU port's OWN fx_T when every x_0 entry moves by one "
                                               "fp32 ulp: the floor under final_loss_rel_diff_vs_cpu_port for this trajectory")
    if numpy_leg and problem == "quadratic" and B * D * T <= 2_000_000:
        prob = O.Quadratic(arrays["W"], arrays["y"])
        t0 = time.perf_counter()
        res = O.unroll(prob, cfg, weights, x0, O.net_initial_state(cfg, B * D), T)
        dt = time.perf_counter() - t0
        out["numpy_oracle"] = {"value": B * D * T / dt, "unit": "coordinate-steps/s",
                               "sample": "1 unroll, %.1f s" % dt, "fx_T": float(res.fx[-1])}
    return out


def cpu_baseline_mnist(weights, batch, T, max_seconds=15.0):
    """Config 5's CPU leg: the NumPy oracle (oracle/l2o_oracle.py: MnistMLP.fg + the RNNProp inputs of
    DM/meta_rnnprop_train.py:383-388 + net_apply, the four variables stepped by one net) for a bounded
    number of steps on synthetic MNIST-shaped data; multi-threaded BLAS."""
    import oracle as O
    rng = np.random.default_rng(5)
    n_data = 1024
    prob = O.MnistMLP(rng.random((n_data, 784), dtype=np.float32), rng.integers(0, 10, n_data).astype(np.int32))
    xs = prob.init_vars(np.random.default_rng(6))
    cfg = O.RNNPROP
    f = np.float32
    b1 = b2 = f(0.95)
    states = [O.net_initial_state(cfg, x.size) for x in xs]
    ms, vs = [np.zeros_like(x) for x in xs], [np.zeros_like(x) for x in xs]
    steps = 0
    t0 = time.perf_counter()
    while steps < T and time.perf_counter() - t0 < max_seconds:
        _, grads = prob.fg(xs, rng.integers(0, n_data, size=batch))
        k = f(steps + 1)
        for j, g in enumerate(grads):
            ms[j] = b1 * ms[j] + f(1.0 - 0.95) * g
            vs[j] = b2 * vs[j] + f(1.0 - 0.95) * g * g
            den = np.sqrt(vs[j] / (f(1) - np.power(b2, k))) + f(1e-8)
            delta, states[j] = O.net_apply(cfg, weights, (ms[j] / (f(1) - np.power(b1, k)) / den, g / den), states[j])
            xs[j] = xs[j] + delta
        steps += 1
    dt = time.perf_counter() - t0
    ncoord = sum(int(x.size) for x in xs)
    return {"value": ncoord * steps / dt, "unit": "coordinate-steps/s", "cores": os.cpu_count(),
            "host_cpus": os.cpu_count(), "kind": "port",
            "sample": "%d steps of the NumPy oracle (MnistMLP.fg + RNNProp inputs + net_apply, multi-threaded BLAS) on "
                      "the 784-20-10 MLP, minibatch %d, %.1f s" % (steps, batch, dt)}


# (directory, global batch it was trained with).  The loss is a mean over the GLOBAL batch (DM/problems.py:99), so the
# gradient scale an identity-preprocessing L2O-DM optimizer sees is 1/B_global: it transfers to a LARGER global batch
# (smaller gradients: smaller steps, still converging) but not to a smaller one (config 4's optimizer, trained at 1024,
# diverges on a stand-alone batch of 128).  RNNProp's inputs are normalised by the moments: scale-free.
TRAINED = {("quadratic", "dm", 128): ("dm_quadratic_d128", 128), ("rastrigin", "dm", 100): ("dm_rastrigin_d100", 1024),
           ("lasso", "rnnprop", 512): ("rnnprop_lasso_256x512", None),
           # config 5: RNNProp meta-trained on the 784-20-10 MLP optimizee (synthetic MNIST-shaped data, minibatch 64)
           ("mnist", "rnnprop", 128): ("rnnprop_mnist_mlp", None)}


def trained_weights(args, key, Bg):
    """The committed meta-trained optimizer of this workload (tests/golden/trained/<name>/<net key>.l2l-0, the
    reference's checkpoint format, DM/networks.py:47-62), or (None, None)."""
    name, trained_bg = TRAINED.get((args.problem, args.net, args.dims), (None, None))
    if name is None or args.untrained or (trained_bg is not None and Bg < trained_bg):
        return None, None
    path = os.path.join(ROOT, "tests", "golden", "trained", name, "%s.l2l-0" % key)
    if not os.path.exists(path):
        return None, None
    import dill
    with open(path, "rb") as f:
        d = dill.load(f)
    w = {m: {v: np.asarray(a, np.float32) for v, a in mv.items()} for m, mv in d.items()}
    return w, "trained: %s%s" % (os.path.relpath(path, ROOT),
                                 "" if trained_bg in (None, Bg) else " (meta-trained at global batch %d, run at %d)" % (trained_bg, Bg))


def build_workload(args, Bg):
    """Problem + optimizer through the product API."""
    from open_l2o_amd import meta, meta_rnnprop_eval, networks, util
    D, T = args.dims, args.unroll
    meta.set_random_seed(1234)                     # same global problem + weights on every rank
    opts = {"batch_size": Bg, "num_dims": D}
    if args.problem == "lasso":
        opts.update(l=0.1, num_rows=args.rows)
    if args.problem == "mnist":                    # not sharded: every GPU optimizes its own replica
        from open_l2o_amd import problems
        opts = {"batch_size": args.batch, "data": problems.synthetic_mnist(4096, seed=5, label_noise=0.1)}
    problem, net_config, net_assignments = util.get_config(
        args.problem, problem_options=opts, net_name="RNNprop" if args.net == "rnnprop" else None)
    if args.problem == "lasso" and args.shared_matrix:
        # the shared-A variant of SURVEY.md 8(d): ONE sensing matrix [rows, dims] for every problem
        from open_l2o_amd import problems
        rng = np.random.default_rng(4321)
        rows = args.rows or D
        problem = problems.lasso_fixed(rng.random((rows, D), dtype=np.float32),
                                       rng.random((Bg, rows, 1), dtype=np.float32), l=0.1)
    if args.net == "dm_logsign" or (args.problem == "mnist" and args.net == "dm"):
        net_config = {"cw": util.get_default_net_config(None)}
    key = next(iter(net_config))
    cfg = dict(net_config[key])
    weights, wsrc = trained_weights(args, key, Bg)
    if weights is None:
        # Sonnet-default random init, output Linear x0.1: an UNTRAINED optimizer (its trajectory diverges)
        weights = networks.factory(cfg["net"], cfg["net_options"]).variables
        weights = {m: {v: np.array(a) for v, a in d.items()} for m, d in weights.items()}
        weights["linear"] = {k: (a * np.float32(0.1)).astype(np.float32) for k, a in weights["linear"].items()}
        wsrc = "untrained: Sonnet-default random draw, output Linear x0.1 (the loss trajectory of this optimizer DIVERGES)"
    args.weights_source = wsrc
    cfg["net_options"] = dict(cfg["net_options"], initializer=weights)
    net_config = {key: cfg}
    feed = {}
    if args.problem == "mnist" and (args.replicas > 1 or args.xcd_form):
        # N independent instances of the optimizee stepped by ONE optimizer, one per XCD (replicas.Replicas)
        from open_l2o_amd.replicas import Replicas
        optimizer = (meta_rnnprop_eval.MetaOptimizer(0.95, 0.95, **net_config) if args.net == "rnnprop"
                     else meta.MetaOptimizer(**net_config))
        reps = Replicas(optimizer, [problem] * args.replicas, T, net_assignments=net_assignments)
        if args.net == "rnnprop":
            feed = {reps.step: 1}
        optimizer._replica_graph = ReplicaGraph(reps)
        return optimizer, None, feed, weights
    if args.net == "rnnprop":
        optimizer = meta_rnnprop_eval.MetaOptimizer(0.95, 0.95, **net_config)
        ml, _, _, step = optimizer.meta_loss(problem, T, net_assignments=net_assignments)
        feed = {step: 1}
    else:
        optimizer = meta.MetaOptimizer(**net_config)
        ml = optimizer.meta_loss(problem, T, net_assignments=net_assignments)
    return optimizer, ml, feed, weights


class ReplicaGraph(object):
    """What run_case needs of an unroll graph, for N replicas launched together (replicas.Replicas.launch)."""

    def __init__(self, reps):
        self.reps = reps
        self.x, self.constants = [], []
        self.last_path = None
        self.last_fx = None                                  # every replica's fx[0..T] of the last launch
        self._x0 = None

    def reset(self):
        self.reps.reset()
        self._x0 = [[v.value.clone() for v in g.x] for g in self.reps.graphs]

    def launch(self, feed, commit=True, events=None, use_graph=False, restart=None):
        if restart is not None:                              # every replica from ITS initial weights, zero state / moments:
            import torch                                     # one multi-tensor copy for all of them
            dst, src = [], []
            for g, x0 in zip(self.reps.graphs, self._x0):
                d_, s_ = g.rewind_lists(x0)
                dst += d_
                src += s_
            torch._foreach_copy_(dst, src)
        if events is not None:
            events[0].record()
        fx = self.reps.launch(feed)
        if events is not None:
            events[1].record()
        self.last_path = "mlp_unroll"
        self.last_fx = fx
        return fx[0], None

    def wait_fx(self):
        pass


def timed_outputs(graph, eng, fx_host):
    """What the last timed unroll handed its caller, copied to the host: the losses fx[0..T] (all-reduced when sharded)
    and every optimizee variable at x_T (this rank's shard when sharded); one set per replica for a ReplicaGraph."""
    def var(v):
        return "x_T_" + "".join(c if c.isalnum() else "_" for c in v.name.split(":")[0])
    if isinstance(graph, ReplicaGraph):
        out = {}
        for r, (g, fx) in enumerate(zip(graph.reps.graphs, graph.last_fx)):
            out["replica%d_fx" % r] = eng.to_numpy(fx)
            out.update(("replica%d_%s" % (r, var(v)), eng.to_numpy(v.value)) for v in g.x)
        return out
    out = {"fx": fx_host}
    out.update((var(v), eng.to_numpy(v.value)) for v in graph.x)
    return out


def write_outputs(path, outputs):
    """--dump-outputs: DIR/<name>.npy in float32.  Beyond DUMP_BYTES in all, every array keeps the same share of its
    elements: a fixed seeded sample of its flattened elements, in index order (the same elements on every run)."""
    os.makedirs(path, exist_ok=True)
    arrays = {k: np.asarray(a, np.float32) for k, a in outputs.items()}
    total = sum(a.nbytes for a in arrays.values())
    share = min(1.0, DUMP_BYTES / float(total)) if total else 1.0
    for name, a in sorted(arrays.items()):
        if share < 1.0:
            pick = np.random.default_rng(0).choice(a.size, int(a.size * share), replace=False)
            a = a.reshape(-1)[np.sort(pick)]
        np.save(os.path.join(path, name + ".npy"), a)
    print("bench.py: %d output arrays -> %s%s" % (len(arrays), path, "" if share == 1.0 else
                                                 " (a seeded sample of %.3g of each)" % share), file=sys.stderr)


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dims", type=int, default=128)
    ap.add_argument("--batch", type=int, default=128,
                    help="problems per GPU (--scaling weak) / in the whole job (--scaling strong)")
    ap.add_argument("--unroll", type=int, default=100, help="T")
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"])
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline does not need: roofline (replays of one instance, PMC files), "
                         "the device-copy figure, cpu_baseline and the `also` block of other configurations")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the cpu_baseline legs")
    ap.add_argument("--untrained", action="store_true", help="random Sonnet-default weights even where a trained "
                                                             "optimizer is committed (the round-1/2 bench)")
    ap.add_argument("--unrolls-per-step", dest="reps", type=int, default=None,
                    help="complete unrolls (each on a fresh problem instance) per bench step; default per config so "
                         "that 20 steps are >= --min-timed-seconds of GPU work, whatever --steps says")
    ap.add_argument("--instances", type=int, default=4, help="ring of pre-sampled problem instances resident in HBM")
    ap.add_argument("--no-also", action="store_true", help="with --full: skip the extra runs of the `also` block (N > 1: strong scaling / "
                                                           "config 4; N = 1: configs 3, 4, 4's shard of 8, 5)")
    ap.add_argument("--also-budget", dest="also_budget", type=float, default=75.0, help="seconds after which no further also-run starts")
    ap.add_argument("--also-cpu-seconds", dest="also_cpu_seconds", type=float, default=4.0,
                    help="bound of each also-run's cpu_baseline sample")
    ap.add_argument("--min-timed-seconds", dest="min_timed_seconds", type=float, default=1.0,
                    help="the default --unrolls-per-step is chosen so that a timed region of 20 steps is at least this "
                         "long: a sustained measurement, not a burst (VERDICT r05 item 4)")
    ap.add_argument("--dump-outputs", dest="dump_outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last timed unroll returned (fx[0..T], every optimizee "
                         "variable at x_T; rank 0) as DIR/<name>.npy, float32, at most 64 MB in all (a fixed seeded "
                         "sample of each array beyond that)")
    ap.add_argument("--real-collective", dest="real_collective", action="store_true",
                    help="with --emulate-world: issue the shard's collectives through a REAL world-size-1 RCCL process "
                         "group of this process (communicator, stream hand-over, enqueue path) instead of skipping them")
    ap.add_argument("--emulate-world", dest="emulate_world", type=int, default=0,
                    help="run ONE shard (rank 0) of a job sharded over this many GPUs in this single process: batch / N "
                         "problems, 1/B_global = 1/batch, no collective (with --config 4: the per-rank work of BASELINE configs[3])")
    ap.add_argument("--replicas", type=int, default=1,
                    help="config 5 only: this many independent optimizee instances (replicas) per unroll launch, one per XCD "
                         "(k_mlp_xcd, l2o_mlp_unroll_multi); 1 = one instance on the whole chip (k_mlp_unroll)")
    ap.add_argument("--xcd-form", dest="xcd_form", action="store_true",
                    help="config 5 with --replicas 1: run the single instance on the one-XCD kernel (its latency)")
    ap.add_argument("--problem", default="quadratic", choices=["quadratic", "lasso", "rastrigin", "mnist"])
    ap.add_argument("--rows", type=int, default=None, help="lasso rows M (default: dims)")
    ap.add_argument("--shared-matrix", dest="shared_matrix", action="store_true",
                    help="lasso: ONE sensing matrix for all problems (SURVEY 8d shared-A variant)")
    ap.add_argument("--net", default="dm", choices=["dm", "dm_logsign", "rnnprop"])
    ap.add_argument("--config", type=int, default=None, choices=[2, 3, 4, 5],
                    help="preset = BASELINE.json configs[N-1]: 2 default; 3 RNNProp on Lasso 256x512, batch 256, T=200; "
                         "4 DM on Rastrigin d=100, global batch 1024 sharded over the GPUs (strong), T=100; 5 RNNProp on "
                         "the MLP optimizee, minibatch 64, T=200 (forward unroll)")
    args = ap.parse_args(argv)
    if args.config == 3:
        args.problem, args.net, args.dims, args.rows, args.batch, args.unroll = "lasso", "rnnprop", 512, 256, 256, 200
    elif args.config == 4:
        args.problem, args.net, args.dims, args.batch, args.unroll, args.scaling = "rastrigin", "dm", 100, 1024, 100, "strong"
    elif args.config == 5:
        args.problem, args.net, args.batch, args.unroll = "mnist", "rnnprop", 64, 200
    return args


def default_reps(args, B_local):
    """--unrolls-per-step when none was given: enough complete unrolls per bench step that STEPS_PER_MIN_TIMED steps are
    at least --min-timed-seconds of GPU work (round 5 timed 57 ms: a burst says nothing about sustained clocks).  The
    size of a step does not depend on --steps: --steps K times K of the same steps, so ms_per_step of one run tells how
    many steps a later run needs for a given timed length.  From the measured unroll times of round 5 (config 2 0.18 ms;
    config 4 0.19 ms per 128-problem shard, 1.23 ms for 1024 problems; config 3 4.6 ms; config 5 1.8 ms), scaled by
    problems per GPU and T."""
    if args.problem == "quadratic":
        ms = 0.18 * max(1.0, B_local / 128.0) * (0.6 if B_local > 128 else 1.0) * args.unroll / 100.0
    elif args.problem == "rastrigin":
        ms = (0.19 if B_local <= 128 else max(0.31, 1.23 * B_local / 1024.0)) * args.unroll / 100.0
    elif args.problem == "lasso":
        ms = 4.6 * max(1.0, B_local / 256.0) * args.unroll / 200.0
    else:
        ms = (4.6 if (args.replicas > 1 or args.xcd_form) else 1.8) * args.unroll / 200.0
    return max(1, int(np.ceil(args.min_timed_seconds * 1e3 / STEPS_PER_MIN_TIMED / ms)))


def self_launch(args, argv):
    """`python bench.py --gpus N` without a launcher: start N ranks of this script under
    torch.distributed.run (one per GPU, rendezvous on 127.0.0.1) and relay the JSON line."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // max(1, args.gpus))))
    return subprocess.call(cmd, env=env)


def counters_for(workload, kernel_hint, build_id):
    """The PMC summary of exactly this workload (profiles/*_counters_*.json + $L2O_COUNTERS_DIR/counters_*.json, written
    by scripts/counters_to_json.py from rocprofv3 --pmc passes of this command) -> (path, dict, status) or None.
    Chosen by what the file SAYS about itself, never by its name (a lexicographic "newest" picked r04z over
    r04av): a file collected on the build being timed (build_id == l2o_build_id() of the loaded library) wins and is
    "same_build"; otherwise the most recently collected one (collected_unix inside the file; files from before round 5
    carry neither and rank oldest) is returned as "stale" -- its instruction counts belong to another build."""
    paths = glob.glob(os.path.join(ROOT, "profiles", "*_counters_*.json"))    # (profiles/archive_*: earlier rounds' builds, not consulted)
    if os.environ.get("L2O_COUNTERS_DIR"):
        paths += glob.glob(os.path.join(os.environ["L2O_COUNTERS_DIR"], "counters_*.json"))
    best = None
    for path in paths:
        try:
            c = json.load(open(path))
        except Exception:
            continue
        if c.get("workload") != list(workload) or (kernel_hint and kernel_hint not in c.get("kernel", "")):
            continue
        rank = (1 if (build_id and c.get("build_id") == build_id) else 0, float(c.get("collected_unix") or 0.0))
        if best is None or rank > best[0]:
            best = (rank, path, c)
    if best is None:
        return None
    return best[1], best[2], "same_build" if best[0][0] else "stale"


def roofline_block(case, args, counters):
    """The binding roofline of the dominant kernel of this workload.  Time base: kernel_ms_avg = HIP-event time around
    replays of one problem instance on the launch stream (the unroll kernel + its epilogue), measured live in THIS run.

    bound == "hbm" (the streaming kernels): achieved = the bytes a kernel of this form must move per launch (the
        matrices once per evaluation + x / state once each way) / kernel_ms_avg; peak 8 TB/s; traffic = HBM bytes per
        launch from the PMC pass (FETCH_SIZE x 2 on gfx950 + WRITE_SIZE), when one exists for this workload.
    bound == "valu_pipe" (the register / LDS-resident fused kernels: ~20 MB of HBM traffic per launch): a WORK / PEAK
        figure -- achieved = tile-steps per second a SIMD completes (measured cycles per step: work_block), peak = the
        tile-steps per second its VALU pipe could retire from the stated minimal instruction counts at the measured
        pipe rates; frac = achieved / peak = pipe_floor_cycles / measured cycles.  Independent of what the compiler
        emitted; frac_in_kernel_cycles is the same fraction over cycles counted inside the kernel (no clock assumption).
    Named secondaries: valu_active_frac (the UTILISATION round 4 reported as frac: 4 x SQ_ACTIVE_INST_VALU / SIMD-cycles;
    needs counters), issue_cost_frac (single-wave issue costs), alg_bytes_frac (SURVEY.md 8(d)'s step-granular contract
    figure: exceeds 1 for a fused kernel, those bytes never move), fp32_frac.  counters = "same_build" | "stale" | "none"
    says whether the PMC file quoted belongs to the build being timed."""
    kern_s = case["kern_ms"] * 1e-3
    out = {"kernel": case["kernel"], "kernel_ms_avg": case["kern_ms"], "kernel_ms_min": case["kern_ms_min"],
           "algorithmic_bytes_per_launch": case["alg_bytes"], "alg_bytes_per_coord_step": case["bpc"],
           "alg_bytes_GBps": case["alg_bytes"] / kern_s / 1e9, "alg_bytes_frac": case["alg_bytes"] / kern_s / HBM_PEAK,
           "fp32_tflops": case["flops"] / kern_s / 1e12, "fp32_frac": case["flops"] / kern_s / FP32_PEAK}
    src, traffic, issue, status, clock_hz, clock_src = None, None, None, "none", 2.4e9, "nominal 2.4 GHz"
    if counters is not None:
        path, c, status = counters
        src = os.path.relpath(path, ROOT)
        # (the counters are per kernel DISPATCH; a shard beyond the co-resident capacity is several dispatches per unroll)
        nd = float(case.get("dispatches", 1))
        pl = {k: (v * nd if isinstance(v, (int, float)) and k != "SQ_WAVES" else v) for k, v in c.get("per_launch", {}).items()}
        if "FETCH_SIZE_KiB" in pl and "WRITE_SIZE_KiB" in pl:
            traffic = (2.0 * pl["FETCH_SIZE_KiB"] + pl["WRITE_SIZE_KiB"]) * 1024.0
        if c.get("clock_hz_profiled"):
            clock_hz, clock_src = float(c["clock_hz_profiled"]), "GRBM_GUI_ACTIVE / kernel time of the PMC pass (%s counters)" % status
        if all(k in pl for k in ("SQ_ACTIVE_INST_VALU", "SQ_VALU_MFMA_BUSY_CYCLES", "SQ_WAVES")):
            simds = min(N_SIMD, pl["SQ_WAVES"]) if c.get("one_wave_per_simd") else N_SIMD
            issue = {"simds": simds, "valu_active_cycles": 4.0 * pl["SQ_ACTIVE_INST_VALU"],
                     "mfma_busy_cycles": pl["SQ_VALU_MFMA_BUSY_CYCLES"],
                     "kernel_us_profiled": (sum(c["kernel_ns_profiled"].values()) / max(1, len(c["kernel_ns_profiled"])) / 1e3
                                            if c.get("kernel_ns_profiled") else None),
                     "insts_valu": c.get("per_launch", {}).get("SQ_INSTS_VALU"),        # (per DISPATCH, like `waves`)
                     "waves": c.get("per_launch", {}).get("SQ_WAVES")}
    out.update(counters=status, counters_source=src, counters_build_id=None if counters is None else counters[1].get("build_id"))
    if case["hbm_bound"]:
        model = case["hbm_model_bytes"]
        out.update(bound="hbm", unit="GB/s", peak=HBM_PEAK / 1e9, traffic=traffic, traffic_model_bytes=model,
                   achieved=model / kern_s / 1e9, frac=model / kern_s / HBM_PEAK)
        if traffic is not None:
            out.update(traffic_GBps=traffic / kern_s / 1e9, traffic_over_model=traffic / model if model else None)
        if case.get("streaming"):
            # (measured, not assumed: the same kernel with 32 of the 256 problems -- 32 busy CUs, everything cache-resident
            #  -- takes 0.93 of the full launch's time; non-temporal loads on the stream are 21 % SLOWER)
            out["bound_note"] = ("hbm is the byte roofline this row is priced against; the streaming unroll itself is paced by the "
                                 "CU's instruction stream, not by the bytes (profiles/archive_r05/r05w_c3_problem_count_sweep.txt, "
                                 "r05v_c3_nontemporal_stream_ab.txt; DESIGN.md 3.1c)")
    else:
        wb = work_block(case, issue, args, clock_hz)
        if wb is not None:
            cyc, floor = wb["cycles_per_step"], wb["guide_floor_cycles_per_step"]
            per_tile = floor / wb["tiles_per_simd"]
            out.update(bound="valu_pipe", unit="tile-steps/s per SIMD",
                       achieved=wb["tiles_per_simd"] * clock_hz / cyc, peak=clock_hz / per_tile, frac=floor / cyc,
                       peak_source="MI355X_MICROARCH.md throughput table: 2 cycles per plain wave64 VALU instruction per "
                                   "SIMD, 8 per transcendental, x the stated minimal instruction counts (work_model)",
                       traffic=traffic, clock_source=clock_src)
            out.update(wb)
        else:   # the step-granular launches: the fp32-equivalent FLOP fraction stands in
            out.update(bound="fp32_flops", unit="TFLOP/s", achieved=out["fp32_tflops"], peak=FP32_PEAK / 1e12,
                       frac=out["fp32_frac"], traffic=traffic)
        if traffic is not None:
            out["hbm_frac_measured"] = traffic / kern_s / HBM_PEAK
    if counters is not None:
        # where the waves' cycles go (PMC pass sq2; all three count quad-cycles summed over waves, so their ratios to
        # SQ_WAVE_CYCLES are per-wave shares): issuing anything / stalled at issue on a dependency (MFMA or
        # transcendental RAW, LDS data) / parked in s_waitcnt, s_barrier or a poll
        plr = counters[1].get("per_launch", {})
        wc = plr.get("SQ_WAVE_CYCLES")
        if wc:
            for key, name in (("SQ_ACTIVE_INST_ANY", "active_frac"), ("SQ_WAIT_INST_ANY", "wait_inst_frac"),
                              ("SQ_WAIT_ANY", "wait_any_frac"), ("SQ_WAIT_INST_LDS", "wait_inst_lds_frac")):
                if plr.get(key) is not None:
                    out[name] = plr[key] / wc
    if issue is not None:                                    # the utilisation figures (PMC; round 4's `frac`)
        prof_s = (issue["kernel_us_profiled"] or case["kern_ms"] * 1e3) * 1e-6
        peak_cyc = issue["simds"] * clock_hz * prof_s
        out.update(valu_active_frac=min(issue["valu_active_cycles"] / peak_cyc, 1.0),
                   mfma_busy_frac=issue["mfma_busy_cycles"] / peak_cyc,
                   utilisation_note="share of the profiled run's SIMD-cycles in which the VALU issued / the matrix pipe was "
                                    "busy (PMC, %s counters)" % status)
    return out


def run_case(args, eng, world, rank, Bg, B, label):
    """Build one workload, time `steps` unrolls; returns the measurements (all ranks) or None for a
    configuration that does not apply (batch not divisible by the world size)."""
    import torch
    import torch.distributed as dist
    D, T = args.dims, args.unroll
    if args.problem == "mnist":                    # 784-20-10 MLP: 15 910 coordinates, `batch` = minibatch
        D = 784 * 20 + 20 + 20 * 10 + 10
    optimizer, ml, feed, weights = build_workload(args, Bg)
    graph = getattr(optimizer, "_replica_graph", None) or optimizer.graph
    n_rep = max(1, args.replicas) if args.problem == "mnist" else 1
    graph.reset()                                           # (first call: allocator / context warm-up)
    torch.cuda.synchronize()
    # ---- a ring of problem instances, sampled and uploaded BEFORE the timed region (H2D excluded):
    # every timed unroll runs on the next instance, so whatever a new instance costs on the device is inside the timed
    # region.  The iterate lives in its own working buffer.
    graph.launch(feed, commit=True, use_graph=True, restart=[v.value.clone() for v in graph.x])   # which path?
    torch.cuda.synchronize()
    # (only the single-launch fused forms take a new instance per unroll: the step-granular path replays a captured
    #  HIP graph that holds the instance's pointers, and the MLP optimizee has no per-instance constants)
    n_inst = max(1, args.instances) if graph.last_path == "fused" else 1
    ring, t_reset = [], 0.0
    for r in range(n_inst):
        t1 = time.perf_counter()
        graph.reset()                                       # sample x0, W, y on the host (NumPy), upload this rank's shard
        torch.cuda.synchronize()
        t_reset = time.perf_counter() - t1
        ring.append(([v.value.clone() for v in graph.x], [v.value for v in graph.constants]))
    x0 = ring[0][0]

    def use_instance(r):
        for v, t in zip(graph.constants, ring[r][1]):
            v.value = t
        return ring[r][0]

    # HIP events: ONE pair around the whole timed region (a timing event is a barrier packet + a timestamp write:
    # a pair per launch put ~10 us of idle GPU between two unrolls), plus per-launch pairs on a few EXTRA launches
    # after the timed region (kernel_ms_min / the per-launch spread; not part of `value`)
    ev_all = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    ev_rep = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    n_extra = min(5, args.steps)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n_extra)]
    reps = max(1, args.reps if args.reps else default_reps(args, B))
    # one event per bench step inside the timed region (first tenth vs last tenth: clock droop over a sustained run)
    ev_steps = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    cursor = [0]

    def one_unroll(i=None, fresh=True):
        # next problem instance; x <- its x0, LSTM state (m, v) <- 0, then the unroll: restart= folds the rewind into
        # the fused kernels' prologue (they read x0 and start from zero registers); every other path runs
        # graph.rewind(x0) first (the step-granular path replays its 2..6 x T small launches from a HIP graph)
        if fresh:
            cursor[0] = (cursor[0] + 1) % n_inst
        xi = use_instance(cursor[0])
        fx, _ = graph.launch(feed, commit=True, events=None if i is None else ev[i], use_graph=True, restart=xi)
        return fx

    def fence():
        graph.wait_fx()                                     # the asynchronous loss all-reduces (N > 1)
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        for _ in range(reps):
            one_unroll()
    fence()
    # queue-depth rehearsal (untimed, like the warm-up): with prepared calls the host enqueues an unroll in ~11 us and
    # runs hundreds of launches ahead of the GPU; the FIRST time a process has that many commands in flight the HIP
    # runtime grows its command pools -- one ~37 ms host stall (host-timestamp trace: profiles/archive_r01_r03/r03l_host_enqueue_trace.txt)
    # that would otherwise land inside the timed region.  One rehearsal of the timed region's launch count removes it.
    # (config 4's chunked unroll -- 16 launches each -- showed a second one-time stall, 40-50 ms, at the process's ~55th
    #  unroll whatever the flags: `--steps 10` put it at enqueue #3 of the timed region.  At least 128 untimed unrolls
    #  per process keep it out: profiles/archive_r01_r03/r03last_host_trace_c4.txt)
    rehearse = max(args.steps * reps, 128 - args.warmup * reps) if args.warmup > 0 else 0
    rtrace = [time.perf_counter()] if os.environ.get("L2O_BENCH_HOST_TRACE") else None
    for _ in range(rehearse):
        one_unroll()
        if rtrace is not None:
            rtrace.append(time.perf_counter())
    if rtrace is not None and len(rtrace) > 1:
        d = np.diff(np.array(rtrace)) * 1e3
        big = np.argsort(d)[-4:][::-1]
        print("host trace (rehearsal): %d enqueues, median %.4f ms; largest: %s" %
              (len(d), float(np.median(d)), ", ".join("#%d %.2f ms" % (int(k), float(d[k])) for k in big)), file=sys.stderr)
    # The timed region: EXACTLY args.steps steps between two fences (the contract line times it once).  The secondary
    # lines of the `also` block time it twice and keep the faster region (both are reported, `timed_regions_ms`): a one-time
    # host stall of the HIP runtime (r03l / r03last host traces: 37-50 ms, tied to the process's enqueue count, not to the
    # workload) landing inside an 15 ms region would otherwise misreport that workload by 3x.
    regions = []
    for region in range(max(1, int(getattr(args, "timed_regions", 1)))):
        fence()
        t0 = time.perf_counter()
        ev_all[0].record()
        trace = [] if os.environ.get("L2O_BENCH_HOST_TRACE") else None    # (debug: host timestamp after every enqueue)
        ev_steps[0].record()
        for i in range(args.steps):
            for _ in range(reps):
                fx = one_unroll()
                if trace is not None:
                    trace.append(time.perf_counter())
            ev_steps[i + 1].record()
        ev_all[1].record()
        t_enqueue = time.perf_counter() - t0                    # host time to ENQUEUE the timed launches (no sync inside)
        if trace:
            d = np.diff(np.array([t0] + trace)) * 1e3
            big = np.argsort(d)[-6:][::-1]
            print("host trace: %d enqueues, median %.4f ms, sum %.2f ms; largest: %s" %
                  (len(d), float(np.median(d)), float(d.sum()), ", ".join("#%d %.2f ms" % (int(k), float(d[k])) for k in big)),
                  file=sys.stderr)
        fence()
        dt = time.perf_counter() - t0
        if world > 1:
            tt = torch.tensor([dt], device=eng.device, dtype=torch.float64)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            dt = float(tt.item())
        regions.append((dt, t_enqueue, ev_all[0].elapsed_time(ev_all[1]),
                        [ev_steps[k].elapsed_time(ev_steps[k + 1]) for k in range(args.steps)]))
    dt, t_enqueue, ev_all_ms, step_ms = min(regions)
    tenth = max(1, args.steps // 10)
    fx_host = eng.to_numpy(fx)
    # (before the replays below overwrite x and fx)
    outputs = timed_outputs(graph, eng, fx_host) if getattr(args, "dump_outputs", None) else None
    fx_ranks = None
    if world > 1:                                   # every rank's copy of the all-reduced final loss (must be identical)
        mine = torch.tensor([float(fx_host[-1])], device=eng.device, dtype=torch.float64)
        gathered = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(gathered, mine)
        fx_ranks = [float(g.item()) for g in gathered]
    fx_instance = cursor[0]
    eng.check_unroll_status()
    n_unrolls = args.steps * reps
    unroll_all_ms = ev_all_ms / n_unrolls
    kern_all = kern_min = None
    if args.full:
        # ---- (outside the timed region, --full) the dominant kernel on its own: the SAME instance replayed, so no
        # preparation runs between the launches -- the time base of the roofline block
        one_unroll(None, fresh=False)
        ev_rep[0].record()
        for _ in range(max(10, reps)):
            one_unroll(None, fresh=False)
        ev_rep[1].record()
        for i in range(n_extra):
            one_unroll(i, fresh=False)
        torch.cuda.synchronize()
        kern_min = float(np.min([a.elapsed_time(b) for a, b in ev]))
        kern_all = float(ev_rep[0].elapsed_time(ev_rep[1]) / max(10, reps))
    coord_steps = (n_rep if args.problem == "mnist" else B) * D * T     # per GPU per unroll
    Mrows = B if args.problem == "mnist" else (args.rows or D)
    shared = args.problem == "lasso" and args.shared_matrix
    bpc = (alg_bytes_lasso_shared(args.net, B, D, Mrows) if shared
           else alg_bytes_per_coord_step(args.problem, args.net, D, Mrows))
    fused = graph.last_path == "fused"
    # which kernel ran: what the LIBRARY says it launched for the last unroll of this thread (l2o_last_unroll_form, ABI v12:
    # no mirror of the selection logic here), and the step-loop cycle count that kernel left in the workspace header
    form, dispatches = eng.last_unroll_form() if graph.last_path in ("fused", "mlp_unroll") else (None, 1)
    dispatches = max(1, dispatches)
    loop_ticks = (eng.last_loop_ticks() if kern_all is not None and (form in ("k_unroll_pair", "k_unroll_lds")
                                                                    or (form or "").startswith("k_mlp_")) else None)
    streaming = form in ("k_unroll_cu", "k_unroll_cu8")
    notes = {"k_unroll_pair": "every problem on two CUs, one wave per SIMD", "k_unroll_lds": "one problem per CU, two waves per "
             "SIMD, fragments in LDS", "k_unroll_cu8": "streaming, eight waves, fragments in LDS, LSTM state in registers",
             "k_unroll_cu": "streaming, four waves", "k_unroll": "one workgroup per problem, W in LDS"}
    if form is not None:
        kernel = form + (" (%s)" % notes[form] if form in notes else "") + (" x %d chunk launches" % dispatches if dispatches > 1 else "")
        from open_l2o_amd import _abi
        if fused and _abi.get_option(_abi.OPT_EXACT_GATES):
            kernel += " (exact gates)"
    elif args.problem == "mnist":
        kernel = "l2o_mlp_fg + l2o_cwlstm_step_multi per step"
    else:
        kernel = "k_problem_fg1 + k_cwlstm_step per step"
    # HBM bytes per launch that a kernel of this form MUST move (used only when no PMC pass is committed):
    # the per-problem matrices once per evaluation (T + 1) + x / state once each way
    mat_bytes = 0 if args.problem == "mnist" else 4.0 * (1 if shared else B) * Mrows * D
    hbm_model = mat_bytes * ((T + 1) if (streaming or not fused) else 2) + 2 * 4.0 * B * D * 81
    return {"label": label, "graph": graph, "weights": weights, "x0": ring[fx_instance][0], "fx_host": fx_host, "dt": dt,
            "value": world * coord_steps * n_unrolls / dt, "ms_per_step": dt / args.steps * 1e3,
            "ms_per_unroll": dt / n_unrolls * 1e3, "unroll_ms_events": float(unroll_all_ms), "reps": reps,
            "timed_regions_ms": [r[0] * 1e3 for r in regions],
            "step_ms_first_tenth": float(np.mean(step_ms[:tenth])), "step_ms_last_tenth": float(np.mean(step_ms[-tenth:])),
            "step_ms_min": float(np.min(step_ms)), "step_ms_max": float(np.max(step_ms)),
            "n_inst": n_inst, "fx_instance": fx_instance, "fx_ranks": fx_ranks,
            "host_enqueue_ms_per_unroll": t_enqueue / n_unrolls * 1e3,
            "value_replayed": None if kern_all is None else world * coord_steps / (kern_all * 1e-3),
            "kern_ms": kern_all, "kern_ms_min": kern_min, "coord_steps": coord_steps,
            "bpc": bpc, "alg_bytes": bpc * coord_steps,
            "flops": alg_flops_per_coord_step(args.problem, args.net, D, Mrows) * coord_steps,
            "fused": fused, "kernel": kernel, "dispatches": dispatches, "loop_ticks": loop_ticks,
            "n_cus": int(getattr(eng, "coresident_cus", 256)), "hbm_bound": bool(streaming or (not fused and args.problem != "mnist")), "streaming": bool(streaming),
            "hbm_model_bytes": hbm_model, "t_reset": t_reset, "D": D, "B": B, "Bg": Bg, "T": T, "Mrows": Mrows,
            "shared": shared, "outputs": outputs}


def workload_names(args, D, B, Bg, T, Mrows, shared):
    netname = {"dm": "L2O-DM CoordinateWiseDeepLSTM(20,20)", "dm_logsign": "L2O-DM (LogAndSign k=5)",
               "rnnprop": "L2O-RNNProp (fc+ELU, tanh, 0.01)"}[args.net]
    probname = {"quadratic": "Quadratic d=%d" % D,
                "lasso": "Lasso A in R^{%dx%d} l=0.1%s" % (Mrows, D, " (one A shared by the batch)" if shared else ""),
                "rastrigin": "Rastrigin d=%d" % D,
                "mnist": "MLP 784-20-10 (sigmoid) on synthetic MNIST-shaped data, minibatch %d%s" % (
                    B, ", %d independent replica(s) per launch (one per XCD)" % args.replicas
                    if (args.replicas > 1 or getattr(args, "xcd_form", False)) else "")}[args.problem]
    return netname, probname


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    args = parse_args(argv)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args, argv))

    # The contract is ONE JSON line on stdout.  Libraries write there too (RCCL prints a five-line version banner through
    # C stdio when its first communicator is created -- flushed at process exit, i.e. BEHIND the line): from here on fd 1
    # is stderr for everybody, and the line goes to the saved descriptor at the very end.
    sys.stdout.flush()
    line_fd = os.dup(1)
    os.dup2(2, 1)

    import torch
    import torch.distributed as dist
    from open_l2o_amd import _abi, _engine, _graph_core

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d (launch with torch.distributed.run --nproc-per-node %d, "
                         "or without a launcher: bench.py starts its own ranks)" % (args.gpus, world, args.gpus))
    # test hook: L2O_BENCH_BACKEND=gloo L2O_BENCH_ONE_DEVICE=1 runs the N > 1 code path with all
    # ranks on cuda:0 (a 1-GPU box cannot host two RCCL ranks); the driver never sets these
    backend = os.environ.get("L2O_BENCH_BACKEND", "nccl")
    if os.environ.get("L2O_BENCH_ONE_DEVICE"):
        local_rank = 0
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.cuda.set_device(local_rank)
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world,
                                    device_id=torch.device("cuda:%d" % local_rank))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    eng = _engine.HipEngine("cuda:%d" % local_rank)        # raises without GPU / built extension
    _engine.set_default_engine(eng)

    def sizes(a):
        """(global batch, per-GPU batch) of a run; None when the batch does not divide."""
        if a.problem == "mnist":
            return a.batch, a.batch
        if a.scaling == "strong":
            return (a.batch, a.batch // world) if a.batch % world == 0 and a.batch >= world else None
        return a.batch * world, a.batch

    sz = sizes(args)
    if sz is None:
        raise SystemExit("bench.py: --scaling strong needs --batch divisible by --gpus")
    Bg, B = sz
    pg = {"backend": None}

    def world_of_one_group():
        """A REAL RCCL process group of this one process (world size 1, rendezvous on 127.0.0.1), created once: what
        --real-collective issues the shard's collectives through.  RCCL's communicator init, torch's stream hand-over
        between the compute stream and the collective's stream, and the enqueue path all execute; a 1-rank all-reduce
        has nobody to talk to, so no xGMI traffic is generated (stated in the line)."""
        if pg["backend"] is None:
            sock = socket.socket()
            sock.bind(("127.0.0.1", 0))
            port = sock.getsockname()[1]
            sock.close()
            os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
            os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
            t_init = time.perf_counter()
            if backend == "nccl":
                dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:%d" % local_rank))
            else:
                dist.init_process_group(backend, rank=0, world_size=1)
            probe = torch.ones(4, device=eng.device)
            dist.all_reduce(probe)                            # (the communicator is created lazily: pay for it here)
            torch.cuda.synchronize()
            pg.update(backend=dist.get_backend(), init_s=time.perf_counter() - t_init, probe_ok=bool(float(probe.sum()) == 4.0))
        return pg

    if args.emulate_world > 1:
        # ONE shard of a job defined on more GPUs than this box has: this process is rank 0 of `emulate_world` (contiguous
        # batch slice, 1/B_global everywhere, no collective) -- the per-rank rate of BASELINE configs[3] on one GPU
        if world != 1 or args.problem == "mnist" or args.batch % args.emulate_world:
            raise SystemExit("bench.py: --emulate-world needs --gpus 1, a batched optimizee and a divisible batch")
        if args.real_collective:
            world_of_one_group()
        _graph_core.emulate_world(0, args.emulate_world, collectives=args.real_collective)
        Bg, B = args.batch, args.batch // args.emulate_world
    case = run_case(args, eng, world, rank, Bg, B, "primary")
    _graph_core.emulate_world()
    if args.dump_outputs and rank == 0:
        write_outputs(args.dump_outputs, case["outputs"])

    also = {}
    if world > 1 and args.full and not args.no_also and args.problem == "quadratic" and args.config in (None, 2):
        for name, extra_argv in (("config2_strong", ["--config", "2", "--scaling", "strong"]), ("config4", ["--config", "4"])):
            a2 = parse_args(extra_argv + ["--gpus", str(world), "--steps", str(max(5, args.steps // 2)), "--warmup", "2",
                                          "--full"])
            s2 = sizes(a2)
            if s2 is None:
                continue
            c2 = run_case(a2, eng, world, rank, s2[0], s2[1], name)
            n2, p2 = workload_names(a2, c2["D"], c2["B"], c2["Bg"], c2["T"], c2["Mrows"], False)
            also[name] = {"workload": "%s on %s, global batch %d = %d per GPU x %d, T=%d" % (n2, p2, c2["Bg"], c2["B"], world, c2["T"]),
                          "scaling": "strong", "value": c2["value"], "unit": "coordinate-steps/s",
                          "ms_per_step": c2["ms_per_step"], "steps": a2.steps, "kernel": c2["kernel"],
                          "kernel_ms_avg": c2["kern_ms"], "final_loss_fx_T": float(c2["fx_host"][-1])}
            del c2

    copy_gbps = None
    if rank == 0 and args.full:
        # achievable-copy figure of this box: device-to-device copy of 512 MiB, read + write counted
        src = torch.empty(128 << 20, dtype=torch.float32, device=eng.device).normal_()
        dst = torch.empty_like(src)
        for _ in range(2):
            dst.copy_(src)
        c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        c0.record()
        for _ in range(5):
            dst.copy_(src)
        c1.record()
        torch.cuda.synchronize()
        copy_gbps = 5 * 2 * src.numel() * 4 / (c0.elapsed_time(c1) * 1e-3) / 1e9
        del src, dst

    build_id = _abi.build_id()

    def _cpu_leg(a, c, Bg_, B_, D, T, primary):
        """The CPU leg of one workload: the oracle's C port (NumPy oracle for the MLP optimizee), timed on this host.
        N > 1 (rank 0 only, while the other ranks wait at the final barrier): a bounded SAMPLE of rank 0's shard -- the
        launcher gives every rank a slice of the host's threads (torch.distributed.run: OMP_NUM_THREADS = 1 unless set),
        so the sample is as many problems as ~8 s of those threads step, at least one per thread."""
        secs = 20.0 if primary else args.also_cpu_seconds
        if a.problem == "mnist":
            return cpu_baseline_mnist(c["weights"], B_, T, max_seconds=min(secs, 15.0))
        names = {"quadratic": ("w", "y", None), "lasso": ("w", "y", None), "rastrigin": ("A", "B", "C")}[a.problem]
        g = c["graph"]._by_name
        arrays = {"W": g[names[0]].eval(), "y": g[names[1]].eval().reshape(B_, -1)}
        if names[2]:
            arrays["C"] = g[names[2]].eval().reshape(B_, -1)
        x0h = eng.to_numpy(c["x0"][0]).reshape(B_, D)
        note = None
        if world > 1:
            threads = max(1, int(os.environ.get("OMP_NUM_THREADS", "1")))
            n_p = int(min(B_, max(threads, 8.0 * 7.0e4 * threads / (D * T))))     # (~7e4 coordinate-steps/s per thread)
            arrays = {k: v[:n_p] for k, v in arrays.items()}
            x0h, secs = x0h[:n_p], 8.0
            note = "rank 0's first %d of its %d problems, %d thread(s) (OMP_NUM_THREADS of this rank)" % (n_p, B_, threads)
        arrays["l1"], arrays["alpha"] = 0.1, 10.0
        # (the GPU's final loss is comparable with the port's only when both ran the same problems: the whole local batch)
        gpu_fx = float(c["fx_host"][-1]) if world == 1 else None   # (an emulated shard: both sides sum the shard / B_global)
        cpu = cpu_baseline(a.problem, a.net, arrays, c["weights"], x0h, T, max_seconds=secs, B_global=Bg_,
                           numpy_leg=primary and world == 1, gpu_fx_T=gpu_fx)
        if note:
            cpu["sample"] += "; " + note
            cpu.pop("fx_T", None)                               # (a sub-sample's partial loss: not comparable with the job's)
        return cpu

    def describe(a, c, Bg_, B_, primary):
        """The measurement of one workload as a dict: the whole contract line (primary) or its compact form (also).
        roofline and cpu_baseline only with --full (an also-run always has it)."""
        D, T, Mrows, shared = c["D"], c["T"], c["Mrows"], c["shared"]
        netname, probname = workload_names(a, D, B_, Bg_, T, Mrows, shared)
        is_c2 = (a.problem, a.net, D, B_, Bg_, T) == ("quadratic", "dm", 128, 128, 128 * world, 100)
        baseline_config = None
        if is_c2:
            baseline_config = "BASELINE.json configs[1]"
        elif (a.problem, a.net, D, Bg_, T, Mrows) == ("lasso", "rnnprop", 512, 256, 200, 256) and world == 1:
            baseline_config = "BASELINE.json configs[2]"
        elif (a.problem, a.net, D, Bg_, T) == ("rastrigin", "dm", 100, 1024, 100):
            baseline_config = "BASELINE.json configs[3]" + (        # (defined on 8 GPUs: --gpus 8 --config 4 is that line)
                " -- ONE shard of %d (rank 0's %d problems, 1/B_global = 1/1024, no communication)" % (a.emulate_world, B_)
                if a.emulate_world > 1 else (" -- all 1024 problems on ONE GPU" if world == 1 else ""))
        elif (a.problem, a.net, B_, T) == ("mnist", "rnnprop", 64, 200):
            baseline_config = "BASELINE.json configs[4] (forward unroll, one replica per GPU)"
            if a.replicas > 1 or a.xcd_form:
                baseline_config = ("BASELINE.json configs[4], %d independent replica(s) per GPU in one launch, one per XCD "
                                   "(k_mlp_xcd)" % a.replicas)
        counters = roof = None
        if a.full and world == 1 and not shared:
            counters = counters_for([a.problem, a.net, D, B_, T] + ([Mrows] if a.problem == "lasso" else [])
                                    + (["replicas", a.replicas] if a.problem == "mnist" and (a.replicas > 1 or a.xcd_form) else []),
                                    c["kernel"].split(" ")[0] if c["fused"] or "k_mlp_" in c["kernel"] else "", build_id)
        if a.full:
            roof = roofline_block(c, a, counters)
        cpu = None
        if a.full and not a.no_cpu_baseline and not shared and (not primary or world > 1):
            try:
                cpu = _cpu_leg(a, c, Bg_, B_, D, T, primary)
            except Exception as e:                          # noqa: BLE001  (an also-run's / an N > 1 run's CPU leg: recorded, not fatal)
                cpu = None
                cpu_error = "%s: %s" % (type(e).__name__, str(e)[:200])
            else:
                cpu_error = None
        elif a.full and not a.no_cpu_baseline and not shared:
            cpu, cpu_error = _cpu_leg(a, c, Bg_, B_, D, T, primary), None
        else:
            cpu_error = None
        workload = "%s on %s, batch=%d per GPU (global %d), T=%d%s" % (netname, probname, B_, Bg_, T,
                                                                       ", BASELINE.json configs[1]" if is_c2 else "")
        tenth_units = world * c["coord_steps"] * c["reps"]
        sustained = {"timed_region_s": c["dt"], "steps": a.steps, "unrolls_per_step": c["reps"],
                     "value_first_tenth": tenth_units / (c["step_ms_first_tenth"] * 1e-3),
                     "value_last_tenth": tenth_units / (c["step_ms_last_tenth"] * 1e-3),
                     "last_over_first": c["step_ms_first_tenth"] / c["step_ms_last_tenth"],
                     "step_ms_min": c["step_ms_min"], "step_ms_max": c["step_ms_max"],
                     "note": "per-step HIP events inside the timed region (this rank): the first and the last tenth of the steps"}
        if not primary:
            keep = ("kernel", "kernel_ms_avg", "bound", "frac", "frac_guide_peak", "frac_measured_pipe", "active_frac",
                    "wait_inst_frac", "wait_any_frac", "achieved", "peak", "unit", "traffic", "traffic_over_model",
                    "cycles_per_step", "cycles_per_step_in_kernel", "frac_in_kernel_cycles", "cycles_source", "clock_hz", "pipe_floor_cycles_per_step", "tiles_per_simd", "valu_active_frac",
                    "alg_bytes_frac", "fp32_frac", "counters", "counters_source", "bound_note")
            out = {"workload": workload, "baseline_config": baseline_config, "value": c["value"], "unit": "coordinate-steps/s",
                   "steps": a.steps, "unrolls_per_step": c["reps"], "ms_per_unroll": c["ms_per_unroll"],
                   "timed_regions_ms": c["timed_regions_ms"],   # (`value` is the faster of these equal regions)
                   "optimizer_weights": getattr(a, "weights_source", None),
                   "final_loss_fx_T": float(c["fx_host"][-1]), "fx_0": float(c["fx_host"][0]),
                   "sustained": {k: sustained[k] for k in ("timed_region_s", "last_over_first")},
                   "roofline": {k: roof[k] for k in keep if k in roof}}
            if a.emulate_world > 1:
                out["loss_note"] = "fx are the SHARD's partial sums / B_global (no all-reduce under --emulate-world)"
        else:
            scaling_note = None
            if world > 1 or a.scaling == "strong":
                scaling_note = ("weak: %d problems per GPU, global batch %d (config 2 cannot strong-scale: a T-step unroll "
                                "is a serial chain of T x ~1.8 us per problem whatever the number of problems per GPU -- "
                                "see also.config2_strong of --full; config 4's 1024 problems do, see also.config4)" % (B_, Bg_)
                                if a.scaling == "weak" else "strong: global batch %d, %d per GPU" % (Bg_, B_))
            out = {
                "metric": "unroll-steps/sec (batch x params x T), %s on %s" % (netname.split(" ")[0], probname),
                "value": c["value"], "unit": "coordinate-steps/s", "n_gpus": world, "steps": a.steps,
                "warmup": a.warmup, "ms_per_step": c["ms_per_step"], "unrolls_per_step": c["reps"],
                "ms_per_unroll": c["ms_per_unroll"], "host_enqueue_ms_per_unroll": c["host_enqueue_ms_per_unroll"],
                "higher_is_better": True,
                "scaling": a.scaling, "vs_baseline": None, "dtype": "f32", "data": "synthetic",
                "config": {"workload": workload,
                           "baseline_config": baseline_config,
                           "kernel": c["kernel"],
                           "optimizer_weights": getattr(a, "weights_source", None),
                           "step_definition": "one bench step = %d complete unrolls, each on the next of %d pre-uploaded problem "
                                              "instances: rewind + T optimizer steps + f(x_T) + loss reduction; value counts "
                                              "all steps x unrolls" % (c["reps"], c["n_inst"]),
                           "arithmetic": "fp32 state, inputs and outputs; optimizee gradient in the reference's form (r = Wx - y, "
                                         "g = W^T r); the LSTM gate GEMM is a 3-way bf16 split (the six exact products per term, "
                                         "packed into 4 MFMAs per tile for the DM nets) on v_mfma_f32_16x16x32_bf16 with fp32 "
                                         "accumulation (fp32-level error per step; its in-group truncation shows as ~1e-5 "
                                         "drift at T = 1000 -- L2O_EXACT_GATES=1 selects the fmaf-chain-equal fp32 MFMA, "
                                         "DESIGN.md 4); everything else fp32 VALU",
                           "api": "open_l2o_amd.util.get_config -> MetaOptimizer.meta_loss -> UnrollGraph.launch",
                           "parallelism": "problem-batch sharding x%d, one all-reduce of T+1 floats per unroll" % world,
                           "n_ranks_seen": dist.get_world_size() if world > 1 else 1,
                           "backend": (dist.get_backend() if world > 1 else None),
                           "collective": ({"backend": pg["backend"], "world_size": 1, "init_s": pg.get("init_s"),
                                           "note": "--real-collective: this shard's all-reduces go through a real "
                                                   "one-rank process group"} if a.real_collective and pg["backend"] else None),
                           "scaling_note": scaling_note},
                "final_loss_fx_T": float(c["fx_host"][-1]), "fx_0": float(c["fx_host"][0]),
                "final_loss_fx_T_per_rank": c["fx_ranks"],
                "parity_pin": PARITY_PIN,
                "sustained": sustained,
            }
            if roof is not None:                            # (--full)
                roof.update(hbm_copy_measured_GBps=copy_gbps, reset_ms=c["t_reset"] * 1e3)   # MetaLoss.reset: the problem re-sampled on the device
                roof.update(time_base="kernel_ms_avg: HIP events on the launch stream of THIS run around replays of one problem "
                                      "instance (the unroll kernel + its epilogue); cycles_per_step: counted inside the kernel; "
                                      "counters (traffic, valu_active_frac): the rocprofv3 --pmc passes named in counters_source, "
                                      "matched to this library by build id (counters = same_build) or not (stale)",
                            build_id=build_id)
                out.update(value_replayed_problem=c["value_replayed"],
                           value_replayed_note="the same instance replayed (the round-1/2 figure); not the headline",
                           roofline=roof)
        if cpu_error:
            out["cpu_baseline_error"] = cpu_error
        if cpu is not None:
            out["cpu_baseline"] = cpu
            out["speedup_vs_cpu_baseline"] = c["value"] / cpu["value"]
            if "fx_T" in cpu and world == 1:
                ref = cpu["fx_T"]
                out["final_loss_rel_diff_vs_cpu_port"] = abs(float(c["fx_host"][-1]) - ref) / max(abs(ref), 1e-30)
                if "oracle_self_sensitivity" in cpu:          # (only computed when the difference exceeds 1e-5)
                    out["oracle_self_sensitivity"] = cpu["oracle_self_sensitivity"]
        return out

    out = describe(args, case, Bg, B, True) if rank == 0 else None
    # ---- N = 1, --full: the other BASELINE configurations, driver-timed in the same process
    if world == 1 and args.full and not args.no_also and args.config in (None, 2) and args.problem == "quadratic" and args.emulate_world <= 1 \
            and (args.dims, args.batch, args.unroll, args.net) == (128, 128, 100, "dm"):
        del case
        torch.cuda.empty_cache()
        t_also = time.perf_counter()
        short = ["--min-timed-seconds", "0.2"]               # (each also-run: two timed regions of >= 0.2 s)
        for name, extra_argv in (("config3", ["--config", "3"] + short),
                                 ("config4_one_gpu", ["--config", "4"] + short),
                                 ("config4_shard_of_8", ["--config", "4", "--emulate-world", "8"] + short),
                                 # (the same shard with its collectives ISSUED through a real world-size-1 RCCL group: what a
                                 #  rank pays for the loss all-reduce -- collective_us_per_unroll below)
                                 ("config4_shard_of_8_rccl", ["--config", "4", "--emulate-world", "8", "--real-collective",
                                                              "--no-cpu-baseline"] + short),
                                 ("config5", ["--config", "5"] + short),
                                 # (config 5's two kernel forms, VERDICT r05 item 1: EIGHT replicas per launch, one per XCD --
                                 #  the throughput form -- and ONE instance on one XCD -- that form's latency)
                                 ("config5_replicas8", ["--config", "5", "--replicas", "8", "--no-cpu-baseline"] + short),
                                 ("config5_one_xcd", ["--config", "5", "--xcd-form", "--no-cpu-baseline"] + short),
                                 # (the 2- and 4-GPU shards of config 4, GPU side only: DESIGN.md 6 projects the scaling curve
                                 #  from these driver-timed per-shard rates)
                                 ("config4_shard_of_2", ["--config", "4", "--emulate-world", "2", "--no-cpu-baseline"] + short),
                                 ("config4_shard_of_4", ["--config", "4", "--emulate-world", "4", "--no-cpu-baseline"] + short),
                                 # (config 2's shape with a second tile per SIMD: 256 problems, global batch 256 -- what the
                                 #  chip does when a shard is large enough for k_unroll_lds; NOT the contract workload)
                                 ("config2_shape_256_problems", ["--batch", "256", "--no-cpu-baseline"] + short)):
            if time.perf_counter() - t_also > args.also_budget:
                also[name] = {"skipped": "the also-block's time budget (%g s) was spent" % args.also_budget}
                continue
            a2 = parse_args(extra_argv + ["--warmup", "2", "--full"] + (["--no-cpu-baseline"] if args.no_cpu_baseline else []))
            a2.also_cpu_seconds = args.also_cpu_seconds
            a2.timed_regions = 2                            # (the faster of two timed regions: see run_case)
            # (an also-run must never take the primary line down with it: a failure is recorded, the line still prints)
            try:
                if a2.emulate_world > 1:
                    if a2.real_collective:
                        world_of_one_group()
                    _graph_core.emulate_world(0, a2.emulate_world, collectives=a2.real_collective)
                    Bg2, B2 = a2.batch, a2.batch // a2.emulate_world
                else:
                    Bg2, B2 = sizes(a2)
                try:
                    c2 = run_case(a2, eng, 1, 0, Bg2, B2, name)
                finally:
                    _graph_core.emulate_world()
                also[name] = describe(a2, c2, Bg2, B2, False)
                also[name]["host_enqueue_ms_per_unroll"] = c2["host_enqueue_ms_per_unroll"]
                del c2
            except Exception as e:                          # noqa: BLE001
                also[name] = {"error": "%s: %s" % (type(e).__name__, str(e)[:300])}
            torch.cuda.empty_cache()
        # ---- what the N > 1 path's collective costs ONE rank, measured on this box: the config-4 shard
        # of 8 with and without its loss all-reduce going through a real RCCL communicator (async_op on torch's collective
        # stream, waited for by the reader of the loss only).  device = the change of the timed region per unroll, host = the
        # change of the host's enqueue time per unroll.  A world of ONE rank moves no bytes over xGMI: this prices the
        # launch path, not the links.
        pa, pb = also.get("config4_shard_of_8"), also.get("config4_shard_of_8_rccl")
        if pa and pb and "value" in pa and "value" in pb:
            out["collective_us_per_unroll"] = {
                "device": (pb["ms_per_unroll"] - pa["ms_per_unroll"]) * 1e3,
                "host_enqueue": (pb["host_enqueue_ms_per_unroll"] - pa["host_enqueue_ms_per_unroll"]) * 1e3,
                "backend": pg.get("backend"), "world_size": 1, "init_s": pg.get("init_s"),
                "fx_T_equal_without_collective": pa["final_loss_fx_T"] == pb["final_loss_fx_T"],
                "workload": "config 4, one shard of 8 (128 problems, T=100): one asynchronous all-reduce of T+1 floats per unroll",
                "note": "a REAL RCCL communicator of one rank on this GPU: init, stream hand-over and enqueue path execute; no "
                        "peer, so no xGMI traffic -- the 8-GPU line is `bench.py --gpus 8 --config 4`"}
        elif pb and "error" in pb:
            out["collective_us_per_unroll"] = {"error": pb["error"]}
        # ---- flat copies of the other configurations' headline figures (they survive a consumer that keeps top-level
        # scalars only: VERDICT r05 item 4)
        for name, pre in (("config3", "c3"), ("config4_one_gpu", "c4"), ("config4_shard_of_8", "c4s8"), ("config5", "c5"),
                          ("config4_shard_of_8_rccl", "c4s8rccl"), ("config5_replicas8", "c5x8"), ("config5_one_xcd", "c5xcd1")):
            e = also.get(name) or {}
            if "value" in e:
                out[pre + "_value"] = e["value"]
                out[pre + "_kernel_ms"] = e["roofline"].get("kernel_ms_avg")
                out[pre + "_frac"] = e["roofline"].get("frac")
                out[pre + "_bound"] = e["roofline"].get("bound")
                out[pre + "_cpu_value"] = (e.get("cpu_baseline") or {}).get("value")
                if "final_loss_rel_diff_vs_cpu_port" in e:
                    out[pre + "_rel_diff_vs_cpu_port"] = e["final_loss_rel_diff_vs_cpu_port"]
                if "oracle_self_sensitivity" in e:
                    out[pre + "_oracle_self_sensitivity"] = e["oracle_self_sensitivity"]
                if pre.startswith("c5"):
                    out[pre + "_ms_per_unroll"] = e["ms_per_unroll"]   # (latency of one launch: 1 instance, or 8 together)
        also["seconds"] = time.perf_counter() - t_also
    if world > 1:
        dist.barrier()                                      # (ranks > 0 wait here while rank 0 times its CPU leg)
    if dist.is_initialized():
        dist.destroy_process_group()
    if rank == 0:
        if also:
            out["also"] = also
        sys.stdout.flush()
        os.write(line_fd, (json.dumps(out) + "\n").encode())
    os.close(line_fd)


if __name__ == "__main__":
    main()
