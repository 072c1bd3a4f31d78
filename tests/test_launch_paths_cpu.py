"""UnrollGraph.launch path by path, without a GPU: which of its four paths ("fused", "mlp_unroll", "confocal_unroll",
"steps") a plain and a recording launch take, which engine entry points they call in which order (with the arguments that
tell the forms apart: hist, x0, zero_state, step0), which loss buffer comes back, what the launch memo says, who takes a
recovery snapshot, what lands in `record`, and what `commit` changes -- on the oracle engine, on the oracle-backed engines
that claim the fused MLP / confocal kernels, and on one with prepared calls.  Plus the prepared-call cache, the x-scale
buffer cache and the HIP-graph capture state machine of the step path (torch's graph classes replaced by counters)."""
import numpy as np
import pytest
import torch

from helpers import ORACLE_CFGS, make_params, make_problem
from oracle_engine import OracleEngine
from open_l2o_amd import _engine, meta, meta_rnnprop_eval, problems
from test_confocal_replicas_cpu import _Claiming as ClaimingConfocalMulti, make_replicas as confocal_replicas
from test_fused_host_paths_cpu import ClaimingMlp
from test_meta_api import _net_config

ENTRY_POINTS = ("unroll", "prepared_unroll", "mlp_unroll", "confocal_unroll", "problem_fg", "mlp_fg", "confocal_fg",
                "lstm_step_multi", "reduce_fx")
STEP_TEXT = r"^You must feed a value for placeholder 'step' \(DM/util.py:59-60\)$"


class ClaimingMlpGeneric(ClaimingMlp):
    def mlp_unroll_supported(self, spec, d):
        return 1                                             # (the kernel applies, but not in its FAST form)


class ClaimingConfocal(ClaimingConfocalMulti):
    def confocal_unroll(self, *a, **kw):                     # (the base refuses the single form; here it is the one under test)
        pass


class PreparedOracle(OracleEngine):
    """The oracle engine plus prepared calls: a closure over self.unroll that reports "stale" when told to."""
    stale = False

    def prepared_unroll(self, spec, wpack, p, x, st, m, v, T, fx_part, x0, zero_state):
        def call(fx, step0=1):
            self.trace.append(("prepared_call", step0))
            if self.stale:
                return False
            self.unroll(spec, wpack, p, x, st, m, v, T, step0, fx_part, fx=fx, x0=x0, zero_state=zero_state)
            return True
        return call


def traced(eng):
    """Wrap the engine's entry points: eng.trace lists the outermost calls in order."""
    eng.trace, depth = [], [0]

    def wrap(name, fn):
        def inner(*a, **kw):
            if not depth[0]:
                if name == "unroll":
                    step0 = a[8] if len(a) > 8 else kw["step0"]
                    eng.trace.append((name, step0, kw.get("hist") is not None, kw.get("x0") is not None,
                                      bool(kw.get("zero_state", False))))
                elif name in ("mlp_unroll", "confocal_unroll"):
                    eng.trace.append((name, kw.get("hist") is not None))
                else:
                    eng.trace.append((name,))
            depth[0] += 1
            try:
                return fn(*a, **kw)
            finally:
                depth[0] -= 1
        return inner
    for name in ENTRY_POINTS:
        if hasattr(eng, name):
            setattr(eng, name, wrap(name, getattr(eng, name)))
    return eng


@pytest.fixture
def install():
    old = _engine._default_engine

    def use(eng):
        _engine.set_default_engine(traced(eng))
        return eng
    yield use
    _engine.set_default_engine(old)


def unroll(step0=1, hist=False, x0=False, zero_state=False):
    return ("unroll", step0, hist, x0, zero_state)


def steps(fg, T, reduce=False):
    return [(fg,), ("lstm_step_multi",)] * T + [(fg,)] + ([("reduce_fx",)] if reduce else [])


def wide_ring(g, n=3):
    """A ring of n loss buffers, as a sharded graph has (FX_RING of them): shows which launches rotate it."""
    T = g.len_unroll
    store = g.engine.zeros(n, T + 1)
    g._fx_cache[T] = {"store": store, "bufs": [store[k] for k in range(n)], "work": [None] * n, "i": 0, "pending": []}
    return g


def analytic_graph(kind="quadratic", name="dm", T=3, second_derivatives=False, seed=50):
    cfg, B, D = ORACLE_CFGS[name], 2, 16
    params = make_params(cfg, seed=seed, trained_like=True)
    prob, x0, _ = make_problem(kind, B, D, seed=seed + 1)
    make = problems.quadratic if kind == "quadratic" else problems.lasso
    problem = make(B, D, data={"w": prob.w, "y": prob.y, "x": x0})
    if name == "rnnprop":
        opt = meta_rnnprop_eval.MetaOptimizer(0.95, 0.95, **_net_config(cfg, params, key="rp"))
    else:
        opt = meta.MetaOptimizer(**_net_config(cfg, params))
    opt.meta_loss(problem, T, second_derivatives=second_derivatives)
    g = opt.graph
    g.reset()
    return wide_ring(g)


def mnist_graph(T=3):
    rng = np.random.default_rng(60)
    data = {"images": rng.random((32, 6)).astype(np.float32), "labels": rng.integers(0, 10, size=32)}
    idx = rng.integers(0, 32, size=(T + 1, 4))
    params = make_params(ORACLE_CFGS["dm"], seed=61, trained_like=True)
    meta.set_random_seed(62)
    opt = meta.MetaOptimizer(**_net_config(ORACLE_CFGS["dm"], params))
    opt.meta_loss(problems.mnist(layers=(20,), batch_size=4, data=data, sampler=lambda n, b, N: idx[:n]), T)
    g = opt.graph
    g.reset()
    return wide_ring(g)


def confocal_graph(fused, T=3):
    g = confocal_replicas("dm", 1, T, batch=2, points=1, roi=(4, 5, 3), fused=fused).graphs[0]
    g.reset()
    return wide_ring(g)


FUSED_KEYS = {"step0", "shapes", "g", "st", "m", "v", "g_final", "plan"}
STEP_KEYS = FUSED_KEYS - {"plan"}


def check_launch(g, path, calls, commit=True, record=False, restart=None, feed=None, snapshot=False, rotates=False,
                 keys=None, plan=None, computes=True, **kw):
    """One launch and everything a cell asserts about it; returns (fx, xs, record)."""
    eng, T = g.engine, g.len_unroll
    ring = g._fx_cache[T]
    i0 = ring["i"]
    live = [v.value for v in g.x]
    states = [s.state for s in g.slots]
    x_before = [t.clone() for t in live]
    st_before = [s.state.packed.clone() for s in g.slots]
    snaps, take = [], g._snapshot
    g._snapshot = lambda slots: (snaps.append(1), take(slots))
    del eng.trace[:]
    rec = {} if record else None
    try:
        fx, xs = g.launch(feed, commit, record=rec, restart=restart, **kw)
    finally:
        del g.__dict__["_snapshot"]
    assert g.last_path == path
    assert eng.trace == calls
    # the loss buffer: only a plain fused launch rotates the ring; every other launch uses and leaves slot 0
    if rotates:
        assert fx is ring["bufs"][i0] and ring["i"] == (i0 + 1) % len(ring["bufs"])
    else:
        assert fx is ring["bufs"][0] and ring["i"] == 0
    assert g._last_launch == {"restart": restart if (restart is not None and commit and not record) else None,
                              "snapshot": snapshot, "commit": commit}
    assert len(snaps) == (1 if snapshot else 0)
    if record:
        assert set(rec) == keys
        assert rec["step0"] == (int(feed[g.step]) if g.rnnprop else 1)
        assert rec["shapes"] == [tuple(g._panel_shape(v)) for v in g.x]
        if plan is not None:
            assert rec["plan"] is g.__dict__[plan]
    # commit: in place on the live tensors, and the slots hold the states the launch advanced; otherwise on copies
    assert all(v.value is t for v, t in zip(g.x, live)) and len(xs) == len(live)
    assert all((a is b) == commit for a, b in zip(xs, live))
    assert all(s.state is st for s, st in zip(g.slots, states))
    if computes and T > 0:
        assert all(torch.equal(t, b) != commit for t, b in zip(live, x_before))
        assert all(torch.equal(s.state.packed, b) != commit for s, b in zip(g.slots, st_before))
        assert all(not torch.equal(a, b) for a, b in zip(xs, x_before))
    return fx, xs, rec


# ---- quadratic, B = 2, D = 16, DM net ------------------------------------------------------------------------------------
@pytest.mark.parametrize("commit", [True, False])
def test_plain_fused(install, commit):
    install(OracleEngine())
    g = analytic_graph()
    for _ in range(2):
        check_launch(g, "fused", [unroll()], commit=commit, snapshot=commit, rotates=True)
    assert g._fx_cache[3]["i"] == 2


def test_recording_fused(install):
    install(OracleEngine())
    g = analytic_graph()
    check_launch(g, "fused", [unroll()], snapshot=True, rotates=True)       # (a plain launch first: the ring stands at 1)
    plans = []
    for _ in range(2):
        fx, _, rec = check_launch(g, "fused", [unroll(hist=True)], record=True, keys=FUSED_KEYS, plan="_fused_plan")
        plans.append(rec["plan"])
        assert len(rec["g"]) == len(rec["st"]) == 3 and rec["g"][0][0].shape == (2, 16) and rec["g_final"][0].shape == (2, 16)
        assert rec["m"] == rec["v"] == [[None]] * 3
    assert plans[0] is plans[1] and set(plans[0]["hist"]) == {"st", "g", "g_final"}


def test_gradients_records_zero_steps(install):
    install(OracleEngine())
    g = analytic_graph()
    g.len_unroll = 0
    wide_ring(g)
    for _ in range(2):
        _, _, rec = check_launch(g, "steps", [("problem_fg",), ("reduce_fx",)], commit=False, record=True, keys=STEP_KEYS)
        assert rec["g"] == [] and rec["g_final"][0].shape == (2, 16)
    g.len_unroll = 3
    assert g.gradients()[0].shape == (2, 16) and g.last_path == "steps" and g.len_unroll == 3


def test_restart_is_folded_into_the_fused_kernel_or_rewound(install, monkeypatch):
    for eng, folded in ((ClaimingMlp(), True), (OracleEngine(), False)):
        install(eng)
        g = analytic_graph()
        x0 = [v.value.clone() for v in g.x]
        rewinds, rewind = [], g.rewind
        g.rewind = lambda x: (rewinds.append(x), rewind(x))
        outs = []
        for k in range(2):
            fx, xs, _ = check_launch(g, "fused", [unroll(x0=folded, zero_state=folded)], restart=x0, rotates=True,
                                     computes=k == 0)          # (the second ends where it stood: at the first's x_T)
            outs.append((fx.clone(), xs[0].clone()))
            assert len(rewinds) == (0 if folded else k + 1) and all(r is x0 for r in rewinds)
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])   # the same unroll twice
        # a restart that cannot be folded after all (the step path): rewound once the path is known
        g.len_unroll = 2
        wide_ring(g)
        del rewinds[:]
        monkeypatch.setenv("L2O_DISABLE_FUSED", "1")
        check_launch(g, "steps", steps("problem_fg", 2, reduce=True), restart=x0)
        monkeypatch.delenv("L2O_DISABLE_FUSED")
        assert len(rewinds) == 1
        # neither a recording nor an uncommitted launch folds it, nor do they note it in the memo
        check_launch(g, "fused", [unroll(hist=True)], record=True, restart=x0, keys=FUSED_KEYS, plan="_fused_plan",
                     computes=False)
        assert len(rewinds) == 2
        check_launch(g, "fused", [unroll()], commit=False, restart=x0, rotates=True, computes=False)
        assert len(rewinds) == 3 and torch.equal(g.x[0].value, x0[0])       # (the live x was rewound, the unroll ran on a copy)


def test_disable_fused_takes_the_step_path(install, monkeypatch):
    install(OracleEngine())
    monkeypatch.setenv("L2O_DISABLE_FUSED", "1")
    g = analytic_graph()
    for _ in range(2):
        check_launch(g, "steps", steps("problem_fg", 3, reduce=True))
    for _ in range(2):
        check_launch(g, "steps", steps("problem_fg", 3, reduce=True), record=True, keys=STEP_KEYS)
    check_launch(g, "steps", steps("problem_fg", 3, reduce=True), commit=False)


def test_recording_with_second_derivatives_takes_the_step_path(install):
    install(OracleEngine())
    g = analytic_graph(second_derivatives=True)
    for _ in range(2):
        _, _, rec = check_launch(g, "steps", steps("problem_fg", 3, reduce=True), record=True, keys=STEP_KEYS | {"x", "descs"})
        assert len(rec["x"]) == 3 and rec["x"][0][0].shape == (2, 16)
        assert len(rec["descs"]) == 1 and rec["descs"][0].D == 16
    check_launch(g, "fused", [unroll()], snapshot=True, rotates=True)      # (a plain launch is not affected)


# ---- lasso under RNNProp: the fed step ------------------------------------------------------------------------------------
def test_rnnprop_step_is_fed(install):
    install(OracleEngine())
    g = analytic_graph("lasso", "rnnprop")
    check_launch(g, "fused", [unroll(step0=1)], feed={g.step: 1}, snapshot=True, rotates=True)
    check_launch(g, "fused", [unroll(step0=4)], feed={g.step: 4}, snapshot=True, rotates=True)
    _, _, rec = check_launch(g, "fused", [unroll(step0=7, hist=True)], feed={g.step: 7}, record=True, keys=FUSED_KEYS,
                             plan="_fused_plan")
    assert set(rec["plan"]["hist"]) == {"st", "g", "g_final", "m", "v"} and rec["m"][0][0].shape == (2, 16)
    memo = dict(g._last_launch)
    for kw in ({}, {"record": {}}):
        with pytest.raises(ValueError, match=STEP_TEXT):
            g.launch({}, True, **kw)
    assert g._last_launch == dict(memo, snapshot=False)


# ---- a fed x-scale: one persistent device buffer per variable ----------------------------------------------------------------
def test_x_scale_buffer_is_reused_and_refilled(install):
    eng = install(OracleEngine())
    g = analytic_graph()
    a = np.random.default_rng(70).uniform(0.5, 2.0, size=(2, 16)).astype(np.float32)
    check_launch(g, "fused", [unroll()], feed={g.scale[0]: a}, snapshot=True, rotates=True)
    ent = g._scale_bufs["x"]
    assert ent[0] is a and np.array_equal(eng.to_numpy(ent[1]), a) and g._mlp_scales == [None]
    check_launch(g, "fused", [unroll()], feed={g.scale[0]: a}, snapshot=True, rotates=True)
    assert g._scale_bufs["x"] is ent                          # the same array again: nothing is uploaded
    b = (a * 1.5).astype(np.float32)
    check_launch(g, "fused", [unroll()], feed={g.scale[0]: b}, snapshot=True, rotates=True)
    new = g._scale_bufs["x"]
    assert new[0] is b and new[1] is ent[1] and np.array_equal(eng.to_numpy(ent[1]), b)    # copied into the same buffer
    check_launch(g, "fused", [unroll()], snapshot=True, rotates=True)
    assert g._scale_bufs["x"] is new                          # (no feed: the buffer stays, the launch does not see it)


# ---- problems.mnist, 6-20-10, on the engines that claim l2o_mlp_unroll ------------------------------------------------------
@pytest.mark.parametrize("level", [2, 1])
def test_mlp_unroll_paths(install, monkeypatch, level):
    eng = install(ClaimingMlp() if level == 2 else ClaimingMlpGeneric())
    g = mnist_graph()
    st = steps("mlp_fg", 3)
    for _ in range(2):
        check_launch(g, "mlp_unroll", [("mlp_unroll", False)], snapshot=True, computes=False)
        assert eng.singles[-1]["hist"] is None and eng.singles[-1]["indices"] is g._mlp_idx[0]
    check_launch(g, "mlp_unroll", [("mlp_unroll", False)], commit=False, computes=False)
    plans = []
    for _ in range(2):
        if level == 2:
            _, _, rec = check_launch(g, "mlp_unroll", [("mlp_unroll", True)], record=True, keys=FUSED_KEYS,
                                     plan="_mlp_record_plan", computes=False)
            plans.append(rec["plan"])
            assert eng.singles[-1]["hist"] is rec["plan"]["hist"]
        else:
            check_launch(g, "steps", st, record=True, keys=STEP_KEYS)     # (the generic form records no faster than the steps)
    assert level == 1 or plans[0] is plans[1]
    monkeypatch.setenv("L2O_MLP_UNROLL_RECORD_GENERIC", "1")
    for _ in range(2):
        check_launch(g, "mlp_unroll", [("mlp_unroll", True)], record=True, keys=FUSED_KEYS, plan="_mlp_record_plan",
                     computes=False)
    monkeypatch.setenv("L2O_NO_MLP_UNROLL_RECORD", "1")
    for _ in range(2):
        check_launch(g, "steps", st, record=True, keys=STEP_KEYS)
    check_launch(g, "mlp_unroll", [("mlp_unroll", False)], snapshot=True, computes=False)     # (plain launches: unaffected)
    monkeypatch.setenv("L2O_DISABLE_FUSED", "1")
    check_launch(g, "steps", st)


# ---- confocal_microscopy_3d, batch 2, one point, roi (4, 5, 3) ---------------------------------------------------------------
def test_confocal_unroll_paths(install):
    install(ClaimingConfocal())
    g = confocal_graph(fused=True)
    for _ in range(2):
        check_launch(g, "confocal_unroll", [("confocal_unroll", False)], computes=False)
    plans = []
    for _ in range(2):
        _, _, rec = check_launch(g, "confocal_unroll", [("confocal_unroll", True)], record=True, keys=FUSED_KEYS,
                                 plan="_mlp_record_plan", computes=False)
        plans.append(rec["plan"])
    assert plans[0] is plans[1] and "_mlp_idx" not in g.__dict__ and "_snap" not in g.__dict__   # no draw, no snapshot
    g = confocal_graph(fused=False)
    for _ in range(2):
        check_launch(g, "steps", steps("confocal_fg", 3))
    check_launch(g, "steps", steps("confocal_fg", 3), record=True, keys=STEP_KEYS)


# ---- the prepared call ------------------------------------------------------------------------------------------------------
def test_prepared_call_replay_eviction_stale_and_reset(install):
    eng = install(PreparedOracle())
    g = analytic_graph()
    g.slots[0].net.wpack(eng)                                # (the key holds the packed weights: upload them first)
    assert "_fast_unrolls" not in g.__dict__
    check_launch(g, "fused", [unroll(), ("prepared_unroll",)], snapshot=True, rotates=True)
    assert len(g._fast_unrolls) == 1
    key3, ent = next(iter(g._fast_unrolls.items()))
    assert key3[0] == 3 and key3[1] is False and ent["keep"][1] is g.x[0].value and ent["keep"][2] is g.slots[0].state.packed
    for _ in range(2):                                       # the identical launch: ONE call (which launches), no argument building
        _, xs, _ = check_launch(g, "fused", [("prepared_call", 1), unroll()], snapshot=True, rotates=True)
        assert xs == [g.x[0].value] and g._fast_unrolls[key3] is ent
    # neither events nor record nor commit=False nor a fed x-scale is a candidate
    check_launch(g, "fused", [unroll()], commit=False, rotates=True)
    check_launch(g, "fused", [unroll(hist=True)], record=True, keys=FUSED_KEYS, plan="_fused_plan")
    check_launch(g, "fused", [unroll()], feed={g.scale[0]: np.ones((2, 16), np.float32)}, snapshot=True, rotates=True)
    assert list(g._fast_unrolls) == [key3]
    # a stale closure drops its entry and the general path runs (and registers the launch again); the replay attempt had
    # claimed a loss buffer and taken the snapshot already
    eng.stale = True
    i0 = g._fx_cache[3]["i"]
    del eng.trace[:]
    fx, xs = g.launch({}, True)
    eng.stale = False
    assert eng.trace == [("prepared_call", 1), unroll(), ("prepared_unroll",)] and g.last_path == "fused"
    assert fx is g._fx_cache[3]["bufs"][(i0 + 1) % 3] and g._fx_cache[3]["i"] == (i0 + 2) % 3
    assert list(g._fast_unrolls) == [key3] and g._fast_unrolls[key3] is not ent and g._last_launch["snapshot"]
    check_launch(g, "fused", [("prepared_call", 1), unroll()], snapshot=True, rotates=True)
    # 16 entries at most, the oldest evicted first
    for T in range(4, 19):
        g.len_unroll = T
        g.launch({}, True)
    assert len(g._fast_unrolls) == 16 and next(iter(g._fast_unrolls)) == key3
    g.len_unroll = 19
    g.launch({}, True)
    keys = list(g._fast_unrolls)
    assert len(keys) == 16 and key3 not in keys and [k[0] for k in keys] == list(range(4, 20))
    g.len_unroll = 3
    check_launch(g, "fused", [unroll(), ("prepared_unroll",)], snapshot=True, rotates=True)      # (not a replay any more)
    assert [k[0] for k in g._fast_unrolls] == list(range(5, 20)) + [3]
    g.reset()
    assert "_fast_unrolls" not in g.__dict__


# ---- the HIP-graph capture state machine of the step path ------------------------------------------------------------------
def test_capture_state_machine(install, monkeypatch):
    eng = install(OracleEngine())
    eng.device = torch.device("cuda")                        # (what `graphable` asks; the tensors stay where they are)
    monkeypatch.setenv("L2O_DISABLE_FUSED", "1")
    counts = {"graphs": 0, "captures": 0, "replays": 0, "runs": 0}

    class Graph(object):
        def __init__(self):
            counts["graphs"] += 1

        def replay(self):
            counts["replays"] += 1

    class Capture(object):
        def __init__(self, graph):
            assert isinstance(graph, Graph)

        def __enter__(self):
            counts["captures"] += 1

        def __exit__(self, *exc):
            return False
    monkeypatch.setattr(torch.cuda, "CUDAGraph", Graph)
    monkeypatch.setattr(torch.cuda, "graph", Capture)
    g = analytic_graph("quadratic", "rnnprop")
    run = g._run_steps

    def counted(*a, **kw):
        counts["runs"] += 1
        return run(*a, **kw)
    g._run_steps = counted
    calls = steps("problem_fg", 3, reduce=True)

    def go(step, want, feed=(), **kw):
        kw.setdefault("use_graph", True)
        feed = dict(feed, **{}) if feed else {}
        feed[g.step] = step
        check_launch(g, "steps", calls if want["runs"] > counts["runs"] else [], feed=feed, computes=False, **kw)
        assert counts == want, (counts, want)
    go(1, dict(graphs=0, captures=0, replays=0, runs=1))     # 1st: eager
    assert g._hip_graphs == {1: "warm"}
    go(1, dict(graphs=1, captures=1, replays=1, runs=2))     # 2nd: captured once, replayed once
    assert isinstance(g._hip_graphs[1], Graph)
    go(1, dict(graphs=1, captures=1, replays=2, runs=2))     # 3rd: only replayed
    go(5, dict(graphs=1, captures=1, replays=2, runs=3))     # another step0 starts over
    assert g._hip_graphs[5] == "warm" and isinstance(g._hip_graphs[1], Graph)
    go(5, dict(graphs=2, captures=2, replays=3, runs=4))
    go(1, dict(graphs=2, captures=2, replays=4, runs=4))
    g.reset()
    wide_ring(g)
    assert "_hip_graphs" not in g.__dict__
    go(1, dict(graphs=2, captures=2, replays=4, runs=5))
    assert g._hip_graphs == {1: "warm"}
    g.reset()
    wide_ring(g)
    # commit=False, a fed x-scale, use_graph=False or a recording launch never capture
    scale = np.ones((2, 16), np.float32)
    n = 5
    for kw in (dict(commit=False), dict(feed={g.scale[0]: scale}), dict(use_graph=False),
               dict(record=True, keys=STEP_KEYS)):
        for _ in range(2):
            n += 1
            go(1, dict(graphs=2, captures=2, replays=4, runs=n), **dict(kw))
    assert "_hip_graphs" not in g.__dict__
