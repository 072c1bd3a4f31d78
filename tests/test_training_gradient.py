"""The training meta-gradient against a float64 reference, in the situation training is mostly in: an unroll that starts
from CARRIED state.  The reference trains with num_steps / unroll_length = 5 unrolls per epoch and resets only at the
start of an epoch (DM/train_dm.py:42-43, 67-71), so four of five train steps start with a non-zero LSTM state, x != x0
and (RNNProp) non-zero Adam moments with `step` = 21, 41, ...

Every train step's gradient (captured in front of the meta-Adam) is compared with helpers.oracle_meta_grad in float64,
started from a snapshot of what that step started from: the network weights, x, the unpacked LSTM state, m and v.  That
isolates the gradient of the step from trajectory drift; the carry itself (snapshot after step k == the reference's end
state of step k) is checked on its own.  Bound: every weight-gradient block within 5e-4 of its largest entry.

  * consecutive unrolls through the product API at the reference's training shape (quadratic 128 x 10, T = 20) and at
    config 2's d = 128;
  * each recording kernel of the fused forward (the kernel that ran is asserted: engine.last_unroll_form());
  * each backward pipeline (default compact bf16x3, exact gates, tile kernel, generic kernel: the calls are spied on);
  * l2o_cwlstm_bwd_unroll_compact / l2o_cwlstm_wgrad_compact directly, and the contraction at config 2's length;
  * config 2's training step at full size with its trained weights.
"""
import os

import dill
import numpy as np
import pytest
import torch

import oracle as O
from helpers import (ORACLE_CFGS, as_float64, block_errors, lib_option, make_params, make_problem, oracle_meta_grad,
                     random_state, spec_of)
from open_l2o_amd import _abi, _engine, meta, meta_dm_train, meta_rnnprop_eval, meta_rnnprop_train, problems
from open_l2o_amd.session import Session
from test_meta_api import _net_config

pytestmark = pytest.mark.gpu

TRAINED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trained")
GRAD_TOL = 5e-4          # every block within 5e-4 of its largest entry (the suite's bound for the meta-gradient)
CARRY_TOL = 1e-5         # the carried x / LSTM state / moments against the reference's end state, of each array's largest
#                          (or 3 x the float32 oracle's own distance from float64 where that is larger: RNNProp's g / sqrt(v))


@pytest.fixture
def eng():
    e = _engine.HipEngine()
    old = _engine._default_engine
    _engine.set_default_engine(e)
    yield e
    _engine.set_default_engine(old)


def _case(kind, B, D, seed, M=None):
    """(oracle problem, x0 in the oracle's shape, product-API problem on the same data)."""
    stddev = {"rastrigin": 0.3, "quadratic": 0.2, "lasso": 0.2, "square_cos": 0.2}[kind]
    prob, x0, _ = make_problem(kind, B, D, seed=seed, M=M, stddev=stddev)
    if kind == "quadratic":
        api = problems.quadratic(B, D, data={"w": prob.w, "y": prob.y, "x": x0})
    elif kind == "lasso":
        api = problems.lasso(B, D, l=prob.l, num_rows=prob.w.shape[1], data={"w": prob.w, "y": prob.y, "x": x0})
    elif kind == "rastrigin":
        api = problems.rastrigin(B, D, data={"A": prob.A, "B": prob.B, "C": prob.C, "x": x0})
    else:
        api = problems.square_cos(B, D, data={"w": prob.w, "y": prob.y, "wcos": prob.wcos, "x": x0})
    return prob, x0, api


class Trainer(object):
    """meta_minimize driven the way the training harness drives it (reset, then train steps that carry x / state /
    moments), with a snapshot of every step's starting point and the gradient each step hands to the meta-Adam.
    fork: the random-scaling training forks (meta_dm_train / meta_rnnprop_train, DM/util.py:40-54) instead of meta /
    meta_rnnprop_eval; ``scale_feed`` (a list of arrays, one per variable) is then fed to every train step."""

    def __init__(self, eng, name, params, api, T, lr=1e-3, fork=False):
        self.eng, self.cfg, self.T = eng, ORACLE_CFGS[name], T
        self.rn = self.cfg.kind == "rnnprop"
        self.key = "rp" if self.rn else "cw"
        self.scale_ph, self.scale_feed = None, None
        if fork and self.rn:
            self.opt = meta_rnnprop_train.MetaOptimizer(0, 0.95, 0.95, **_net_config(self.cfg, params, key="rp"))
            out = self.opt.meta_minimize(api, T, learning_rate=lr)
            self.ms, self.scale_ph, self.step_ph = out[0], out[1], out[5]
        elif fork:
            self.opt = meta_dm_train.MetaOptimizer(0, **_net_config(self.cfg, params))
            out = self.opt.meta_minimize(api, T, learning_rate=lr)
            self.ms, self.scale_ph, self.step_ph = out[0], out[1], None
        elif self.rn:
            self.opt = meta_rnnprop_eval.MetaOptimizer(0.95, 0.95, **_net_config(self.cfg, params, key="rp"))
            out = self.opt.meta_minimize(api, T, learning_rate=lr)
            self.ms, self.step_ph = out[0], out[3]
        else:
            self.opt = meta.MetaOptimizer(**_net_config(self.cfg, params))
            self.ms, self.step_ph = self.opt.meta_minimize(api, T, learning_rate=lr), None
        self.graph = self.opt.graph
        self.caps = []
        orig = self.graph._adam_apply
        self.graph._adam_apply = lambda grads, lr_, **kw: (
            self.caps.append({k: np.array(v, np.float64) for k, v in grads[self.key].items()}), orig(grads, lr_, **kw))[1]
        self.sess = Session()
        self.step0 = 1

    def reset(self):
        self.sess.run(self.ms.reset)
        self.step0 = 1

    def snapshot(self):
        """What the next unroll starts from: float64 weights, step0 and, per variable in the graph's order, x,
        ((h1, c1), (h2, c2)), m, v ("vars").  x / state / m / v: those of the one variable, or for several the
        concatenation in the same order (flat x, m, v; stacked state rows) -- every variable goes through the same
        coordinate-wise net, so that is what the reference unrolls."""
        g, eng = self.graph, self.eng
        w = {m: {v: np.asarray(a, np.float64).copy() for v, a in d.items()} for m, d in self.opt._nets[self.key].variables.items()}
        slot_of = {s.var_index: s for s in g.slots}
        per = []
        for j, var in enumerate(g.x):
            s = slot_of[j]
            B, D = s.state.B, s.state.D
            h1, c1, h2, c2 = (eng.to_numpy(a).astype(np.float64) for a in eng.state_unpack(s.state.packed, B, D))
            m = eng.to_numpy(s.m).astype(np.float64).reshape(B, D) if self.rn else None
            v = eng.to_numpy(s.v).astype(np.float64).reshape(B, D) if self.rn else None
            per.append(dict(x=var.eval().astype(np.float64), state=((h1, c1), (h2, c2)), m=m, v=v))
        snap = dict(w=w, step0=self.step0, vars=per)
        if len(per) == 1:
            snap.update(per[0])
        else:
            cat = lambda arrs: np.concatenate([a.reshape(-1) for a in arrs])
            snap.update(x=cat([p["x"] for p in per]),
                        state=tuple((np.concatenate([p["state"][l][0] for p in per]),
                                     np.concatenate([p["state"][l][1] for p in per])) for l in range(2)),
                        m=cat([p["m"] for p in per]) if self.rn else None, v=cat([p["v"] for p in per]) if self.rn else None)
        return snap

    def train_step(self):
        """One sess.run([fx, update, step]); returns the gradient handed to Adam."""
        feed = {self.step_ph: self.step0} if self.rn else {}
        if self.scale_feed is not None:
            feed.update(zip(self.scale_ph, self.scale_feed))
        n = len(self.caps)
        self.sess.run([self.ms.fx, self.ms.update, self.ms.step], feed_dict=feed)
        assert len(self.caps) == n + 1
        self.step0 += self.T
        return self.caps[-1]

    def reference(self, prob, snap, dtype=np.float64):
        """oracle_meta_grad from the snapshot, in float64 (prob: a float64 problem) or float32 (the float32 problem);
        prob may also be an ``fg(x, t)`` (helpers.mnist_fg), which takes x as the snapshot holds it."""
        x0 = snap["x"].astype(dtype)
        if hasattr(prob, "grad"):
            x0 = x0.reshape(prob_x_shape(prob, snap["x"]))
        w = {m: {v: a.astype(dtype) for v, a in d.items()} for m, d in snap["w"].items()}
        st = tuple((h.astype(dtype), c.astype(dtype)) for h, c in snap["state"])
        m0, v0 = ((None, None) if snap["m"] is None else (snap["m"].astype(dtype), snap["v"].astype(dtype)))
        return oracle_meta_grad(self.cfg, w, prob, x0, st, self.T, m0=m0, v0=v0, step0=snap["step0"])


def prob_x_shape(prob, x):
    B = x.shape[0]
    return (B, -1, 1) if isinstance(prob, O.Rastrigin) else (B, -1)


def check_grad(got, want, what):
    errs = block_errors(got, want)
    worst = max(errs, key=errs.get)
    assert errs[worst] < GRAD_TOL, (what, worst, errs[worst])
    return errs


def _carried(d):
    """{name: flat float64 array} of x, h1, c1, h2, c2 (and m, v) of a snapshot or an oracle end state."""
    (h1, c1), (h2, c2) = d["state"]
    out = dict(x=d["x"], h1=h1, c1=c1, h2=h2, c2=c2)
    if d["m"] is not None:
        out.update(m=d["m"], v=d["v"])
    return {k: np.asarray(a, np.float64).reshape(-1) for k, a in out.items()}


def split_carry(d, shapes):
    """An end state of oracle_meta_grad over the flat concatenation of several variables -> one dict (x, state, m, v)
    per variable, as Trainer.snapshot's "vars" holds them."""
    offs = np.concatenate([[0], np.cumsum([int(np.prod(sh)) for sh in shapes])]).astype(int)
    out = []
    for a, b in zip(offs[:-1], offs[1:]):
        out.append(dict(x=d["x"].reshape(-1)[a:b], state=tuple((h[a:b], c[a:b]) for h, c in d["state"]),
                        m=None if d["m"] is None else d["m"].reshape(-1)[a:b],
                        v=None if d["v"] is None else d["v"].reshape(-1)[a:b]))
    return out


def spy_bwd_unroll(eng, monkeypatch):
    """Record the (B, D) of the panels of every BPTT launch the graph makes through eng.bwd_unroll (not an engine's
    own inner calls); returns the list it appends to."""
    launches, depth = [], [0]
    real = eng.bwd_unroll

    def spy(spec, w, panels, *a, **kw):
        if not depth[0]:
            launches.append([(pn["B"], pn["D"]) for pn in panels])
        depth[0] += 1
        try:
            return real(spec, w, panels, *a, **kw)
        finally:
            depth[0] -= 1
    monkeypatch.setattr(eng, "bwd_unroll", spy)
    return launches


def check_carry(snap, end, end32, what):
    """The state the graph carried into the next unroll == the reference's end state of the unroll that produced it:
    within CARRY_TOL of each array's largest entry, or 3 x the float32 oracle's own error where that is larger."""
    got, ref, r32 = _carried(snap), _carried(end), _carried(end32)
    worst = {}
    for nm in ref:
        scale = max(float(np.abs(ref[nm]).max()), 1e-30)
        err = float(np.abs(got[nm] - ref[nm]).max()) / scale
        own = float(np.abs(r32[nm] - ref[nm]).max()) / scale
        assert err < max(CARRY_TOL, 3 * own), (what, nm, err, own)
        worst[nm] = (err, own)
    return worst


# ------------------------------------------------------------------------------------------------------------------
# 1. consecutive unrolls: reset, 3 train steps that carry, reset, 1 more
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,D", [(128, 10), (8, 128)])
@pytest.mark.parametrize("name", ["dm", "dm_logsign", "rnnprop"])
def test_consecutive_unrolls_vs_float64(eng, name, B, D):
    """The harness' epoch: every step's gradient vs float64 from that step's own start; the carry between steps vs the
    reference's end state; `reset` really restarts from x0 and the zero state."""
    T = 20
    prob, x0, api = _case("quadratic", B, D, seed=400 + D)
    prob64 = as_float64(prob)
    tr = Trainer(eng, name, make_params(ORACLE_CFGS[name], seed=401, trained_like=True), api, T)
    worst = {}
    prev = None
    for k, do_reset in enumerate((True, False, False, True)):
        if do_reset:
            tr.reset()
        snap = tr.snapshot()
        if do_reset:
            assert np.array_equal(snap["x"], x0.astype(np.float64)) and snap["step0"] == 1
            assert not any(a.any() for hc in snap["state"] for a in hc)
            assert snap["m"] is None or not (snap["m"].any() or snap["v"].any())
        else:
            check_carry(snap, prev, prev32, "carry into step %d" % k)
            assert any(a.any() for hc in snap["state"] for a in hc)          # a carried, non-zero start
        got = tr.train_step()
        want, prev = tr.reference(prob64, snap)
        prev32 = tr.reference(prob, snap, np.float32)[1]
        for key, e in check_grad(got, want, "step %d" % k).items():
            worst[key] = max(worst.get(key, 0.0), e)
        assert tr.graph.last_path == "fused"
    print("consecutive %s %dx%d: worst block errors %s" % (name, B, D, {"/".join(k): "%.2g" % e for k, e in worst.items()}))


# ------------------------------------------------------------------------------------------------------------------
# 2. every recording kernel of the fused forward, on the second unroll
# ------------------------------------------------------------------------------------------------------------------
# (name, problem, B, D, M, the kernel launch_unroll_ch / launch_unroll_cu pick on a 256-CU MI355X)
FORMS = [
    ("quadratic", 128, 10, None, "k_unroll", ("dm", "dm_logsign", "rnnprop")),
    ("square_cos", 16, 2, None, "k_unroll", ("dm", "dm_logsign", "rnnprop")),          # one tile per problem
    ("quadratic", 8, 128, None, "k_unroll_pair", ("dm", "dm_logsign", "rnnprop")),
    ("rastrigin", 4, 100, None, "k_unroll_pair", ("dm", "dm_logsign", "rnnprop")),     # ragged per-problem tiles
    ("lasso", 6, 64, 40, "k_unroll_pair", ("dm", "dm_logsign", "rnnprop")),
    ("rastrigin", 200, 100, None, "k_unroll_lds", ("dm", "dm_logsign", "rnnprop")),    # B > #CU / 2
    ("quadratic", 2, 256, None, "k_unroll_cu8", ("dm", "dm_logsign")),                 # KR = 2
    ("quadratic", 2, 512, None, "k_unroll_cu8", ("dm", "dm_logsign")),                 # KR = 3
    ("lasso", 2, 512, 256, "k_unroll_cu", ("rnnprop",)),                               # RNNProp's recording at D > 256
]
FORM_CASES = [pytest.param(name, kind, B, D, M, form, id="%s-%s-%dx%d-%s" % (form, kind, B, D, name))
              for kind, B, D, M, form, names in FORMS for name in names]


@pytest.mark.parametrize("name,kind,B,D,M,form", FORM_CASES)
def test_recording_kernel_gradient_vs_float64(eng, name, kind, B, D, M, form):
    """The gradient built from each recording kernel's history, on an unroll that starts from carried state; the kernel
    is asserted after every step, so that a change of dispatch cannot quietly move a case onto another kernel."""
    T = 6
    prob, x0, api = _case(kind, B, D, seed=500 + B + D, M=M)
    prob64 = as_float64(prob)
    tr = Trainer(eng, name, make_params(ORACLE_CFGS[name], seed=501, trained_like=True), api, T)
    tr.reset()
    for k in range(2):
        snap = tr.snapshot()
        got = tr.train_step()
        assert tr.graph.last_path == "fused", (k, tr.graph.last_path)
        assert eng.last_unroll_form()[0] == form, (k, eng.last_unroll_form())
    want, _ = tr.reference(prob64, snap)
    errs = check_grad(got, want, "second unroll")
    print("%s %s %s %dx%d: worst block error %.2g" % (form, name, kind, B, D, max(errs.values())))


# ------------------------------------------------------------------------------------------------------------------
# 3. every backward pipeline
# ------------------------------------------------------------------------------------------------------------------
PIPELINES = {"default": {}, "exact_gates": {_abi.OPT_EXACT_GATES: 1}, "tile": {_abi.OPT_BWD_KERNEL: 1},
             "generic": {_abi.OPT_BWD_KERNEL: 2}}


@pytest.mark.parametrize("pipeline", list(PIPELINES))
@pytest.mark.parametrize("kind,B,D", [("quadratic", 8, 128), ("rastrigin", 4, 100)])
@pytest.mark.parametrize("name", ["dm", "dm_logsign", "rnnprop"])
def test_backward_pipeline_vs_float64(eng, name, kind, B, D, pipeline, monkeypatch):
    """The four backward pipelines behind options, on the second unroll, each against float64 -- and each run is
    shown to take the pipeline it names (the engine's BPTT / contraction entry points are spied on):
    default: l2o_cwlstm_bwd_unroll_compact + l2o_cwlstm_wgrad_compact; exact gates: l2o_cwlstm_bwd_unroll + the fp32
    l2o_cwlstm_wgrad; L2O_OPT_BWD_KERNEL 1 / 2: per step l2o_cwlstm_bwd_multi (tile-aligned panel) or
    l2o_cwlstm_bwd_step (ragged), with that option set inside the call, + l2o_cwlstm_wgrad."""
    T = 6
    prob, x0, api = _case(kind, B, D, seed=600 + D)
    prob64 = as_float64(prob)
    tr = Trainer(eng, name, make_params(ORACLE_CFGS[name], seed=601, trained_like=True), api, T)
    tr.reset()
    tr.train_step()                                       # (the default pipeline) -> a carried start
    calls, depth = [], [0]
    for fn in ("bwd_unroll", "wgrad_compact", "wgrad", "bwd_multi", "bwd_step"):
        real = getattr(eng, fn)

        def spy(*a, _fn=fn, _real=real, **kw):
            if not depth[0]:                              # (the calls the graph makes, not an engine's own inner ones)
                calls.append((_fn, bool(kw.get("compact", False)), _abi.get_option(_abi.OPT_BWD_KERNEL),
                              _abi.get_option(_abi.OPT_EXACT_GATES)))
            depth[0] += 1
            try:
                return _real(*a, **kw)
            finally:
                depth[0] -= 1
        monkeypatch.setattr(eng, fn, spy)
    snap = tr.snapshot()
    opts = PIPELINES[pipeline]
    with lib_option(_abi.OPT_EXACT_GATES, opts.get(_abi.OPT_EXACT_GATES, 0)), \
            lib_option(_abi.OPT_BWD_KERNEL, opts.get(_abi.OPT_BWD_KERNEL, 0)):
        got = tr.train_step()
    names = [c[0] for c in calls]
    if pipeline == "default":
        assert names == ["bwd_unroll", "wgrad_compact"] and calls[0][1], calls
    elif pipeline == "exact_gates":
        assert names == ["bwd_unroll", "wgrad"] and not calls[0][1] and calls[0][3] == 1, calls
    else:
        step_fn = "bwd_multi" if D % 16 == 0 else "bwd_step"
        assert names == [step_fn] * T + ["wgrad"], names
        assert all(c[2] == opts[_abi.OPT_BWD_KERNEL] for c in calls), calls
    want, _ = tr.reference(prob64, snap)
    errs = check_grad(got, want, pipeline)
    print("%s %s %dx%d %s: worst block error %.2g" % (pipeline, name, B, D, kind, max(errs.values())))


# ------------------------------------------------------------------------------------------------------------------
# 4. the compact BPTT rows and their contraction, directly
# ------------------------------------------------------------------------------------------------------------------
_WNAMES = {"w_gates1": ("lstm_1", "w_gates"), "b_gates1": ("lstm_1", "b_gates"), "w_gates2": ("lstm_2", "w_gates"),
           "b_gates2": ("lstm_2", "b_gates"), "w_lin": ("linear", "w"), "b_lin": ("linear", "b"),
           "w_fc": ("input_projection", "w"), "b_fc": ("input_projection", "b")}


def _expand_compact(Ac, P, fc):
    """The plain rows [in | h1(t-1) | h1(t) | h2(t-1) | h2(t) | feats | 1] of steps 0..T-1 from the compact blocks
    [in | h1(t) | h2(t) | feats | 1] of l2o_cwlstm_bwd_unroll_compact (block 0 = the state before step 0)."""
    prev, cur = Ac[:-1], Ac[1:]
    return np.concatenate([cur[..., :P], prev[..., P:P + 20], cur[..., P:P + 20], prev[..., P + 20:P + 40],
                           cur[..., P + 20:P + 40], cur[..., P + 40:]], -1)


def _grad_blocks(P, fc):
    """(row slice, column slice) of A^T Bm that are weight gradients (l2o_cwlstm_wgrad computes only those)."""
    K1 = P + 20
    KA = K1 + 60 + (2 if fc else 0) + 1
    out = [(slice(0, K1), slice(0, 80)), (slice(K1, K1 + 40), slice(80, 160)), (slice(K1 + 40, K1 + 60), slice(160, 161)),
           (slice(KA - 1, KA), slice(0, 161 + (20 if fc else 0)))]
    if fc:
        out.append((slice(K1 + 60, K1 + 62), slice(161, 181)))
    return out


@pytest.mark.parametrize("T", [1, 20])
@pytest.mark.parametrize("name", ["dm", "dm_logsign", "rnnprop"])
def test_compact_bwd_unroll_and_wgrad(eng, name, T):
    """l2o_cwlstm_bwd_unroll_compact on ragged multi-panel shapes from a NON-zero state before step 0 and random carries:
    block 0 holds exactly h1 / h2 of step 0's st_prev (zeros elsewhere), blocks 1..T are the plain launch's rows, Bm and
    the carries are the plain launch's (the history is consistent: the state before step t + 1 is step t's output, which
    the compact rows assume); l2o_cwlstm_wgrad_compact == a float64 A^T Bm of those rows."""
    cfg = ORACLE_CFGS[name]
    spec = spec_of(cfg)
    params = make_params(cfg, seed=701, trained_like=True)
    t_ = eng.tensor
    wdev = {kk: t_(params[mm][nn]) for kk, (mm, nn) in _WNAMES.items() if mm in params}
    wfused = dict(wdev, wpack=eng.pack_weights(spec, params))
    fc = cfg.kind == "rnnprop"
    P = cfg.in_dim
    KA = P + 20 + 60 + (2 if fc else 0) + 1
    KB = 161 + (20 if fc else 0)
    step0 = 21
    shapes = [(3, 100), (2, 37), (1, 40), (4, 32)]
    rows = [b * ((d + 15) // 16) * 16 for b, d in shapes]
    R = sum(rows)
    rng = np.random.default_rng(702)
    panels, maps, st0 = [], [], []
    off = 0
    for i, (B, D) in enumerate(shapes):
        N = B * D
        tpp = (D + 15) // 16
        bb, jj = np.divmod(np.arange(N), D)
        maps.append(off + (bb * tpp + jj // 16) * 16 + jj % 16)
        off += rows[i]
        gs = [(rng.standard_normal((B, D)) * 0.5).astype(np.float32) for _ in range(T)]
        ms = [(rng.standard_normal((B, D)) * 0.1).astype(np.float32) for _ in range(T)] if fc else [None] * T
        vs = [(rng.random((B, D)) * 0.1 + 0.01).astype(np.float32) for _ in range(T)] if fc else [None] * T
        # a consistent history (what the compact rows assume: the state before step t + 1 is step t's output), from a
        # random non-zero state before step 0
        state = random_state(cfg, N, 710 + i)
        st0.append(state)
        sts = []
        for k in range(T):
            sts.append(eng.state_pack(*[t_(a) for hc in state for a in hc], B, D))
            if fc:
                f = np.float32
                pw1, pw2 = f(f(0.95) ** (step0 + k)), f(f(0.95) ** (step0 + k))
                den = np.sqrt(vs[k] / (f(1) - pw2)) + f(1e-8)
                inputs = ((ms[k] / (f(1) - pw1) / den).reshape(-1), (gs[k] / den).reshape(-1))
            else:
                inputs = gs[k].reshape(-1)
            state = O.net_apply(cfg, params, inputs, state)[1]
        g_final = t_((rng.standard_normal(N) * 0.5).astype(np.float32))
        panels.append(dict(B=B, D=D, gs=[t_(a) for a in gs], ms=[None if a is None else t_(a) for a in ms],
                           vs=[None if a is None else t_(a) for a in vs], sts=sts, dxs=None, g_final=g_final))
    live = np.zeros(R, bool)
    for mp in maps:
        live[mp] = True
    cin = (rng.standard_normal((4, R, 20)) * 0.3).astype(np.float32)
    cin[:, ~live] = 0.0
    A, Bm, c = eng.empty(T, R, KA), eng.empty(T, R, KB), eng.zeros(4, R, 20)
    eng.bwd_unroll(spec, wfused, panels, T, step0, A, Bm, carry_in=t_(cin), carry_out=c)
    Ac, Bc, cc = eng.empty(T + 1, R, KA - 40), eng.empty(T, R, KB), eng.zeros(4, R, 20)
    Ac.fill_(7.0); Bc.fill_(7.0)                          # every row is written
    eng.bwd_unroll(spec, wfused, panels, T, step0, Ac, Bc, carry_in=t_(cin), carry_out=cc, compact=True)
    G = eng.to_numpy(eng.wgrad_compact(spec, Ac, Bc))
    A, Bm, c, Ac, Bc, cc = (eng.to_numpy(a) for a in (A, Bm, c, Ac, Bc, cc))
    # block 0: h1 / h2 of the state before step 0, zeros in every other column and in the padding rows -- exactly
    blk0 = np.zeros((R, KA - 40), np.float32)
    for mp, ((h1, _), (h2, _)) in zip(maps, st0):
        blk0[mp, P:P + 20] = h1
        blk0[mp, P + 20:P + 40] = h2
    np.testing.assert_array_equal(Ac[0], blk0)

    def close(got, ref, what):
        tol = 2e-5 * np.maximum(np.abs(ref).max(axis=0, keepdims=True), 1e-30) + 1e-9
        assert (np.abs(got - ref) <= tol).all(), (what, float(np.abs(got - ref).max()))

    Ax = _expand_compact(Ac, P, fc)
    for k in range(T):
        close(Ax[k], A[k], "A step %d" % k)
        close(Bc[k], Bm[k], "Bm step %d" % k)
    for a in range(4):
        close(cc[a][live], c[a][live], "carry %d" % a)
    # the contraction: float64 A^T Bm of the plain rows, and of the exact operands it read at the documented error
    A64, Ax64 = A.reshape(T * R, KA).astype(np.float64), Ax.reshape(T * R, KA).astype(np.float64)
    B64 = Bc.reshape(T * R, KB).astype(np.float64)
    ref_plain, ref = A64.T @ Bm.reshape(T * R, KB).astype(np.float64), Ax64.T @ B64
    mag = np.abs(Ax64).T @ np.abs(B64)
    worst = 0.0
    for rs, cs in _grad_blocks(P, fc):
        ratio = float((np.abs(G[rs, cs] - ref[rs, cs]) / np.maximum(mag[rs, cs], 1e-30)).max())
        assert ratio <= 1e-6, (rs, cs, ratio)
        worst = max(worst, ratio)
        scale = float(np.abs(ref_plain[rs, cs]).max())
        assert float(np.abs(G[rs, cs] - ref_plain[rs, cs]).max()) <= 1e-4 * scale, (rs, cs)
    print("compact %s T=%d: max |G - A^T Bm| / (|A|^T |Bm|) = %.3g" % (name, T, worst))


def test_wgrad_compact_config2_length(eng):
    """l2o_cwlstm_wgrad_compact at config 2's size -- rows = 128 x 128 per step, T = 100: 1.6 M rows -- against a row-chunked
    float64 product.  Entrywise bound 1e-7 (|A|^T |Bm|): 5 x what include/l2o_abi.h states for the bf16x3 contraction."""
    cfg = ORACLE_CFGS["dm"]
    spec = spec_of(cfg)
    P, fc = cfg.in_dim, False
    T, R = 100, 128 * 128
    KAC, KB = P + 40 + 1, 161
    gen = torch.Generator(device=eng.device).manual_seed(801)
    Ac = torch.rand((T + 1, R, KAC), generator=gen, device=eng.device) * 2 - 1     # (h in (-1, 1), as the rows hold)
    Ac[..., KAC - 1] = 1.0
    Ac[0, :, :P] = 0.0
    Ac[0, :, P + 40:] = 0.0
    Bm = torch.randn((T, R, KB), generator=gen, device=eng.device) * 1e-3
    G = eng.to_numpy(eng.wgrad_compact(spec, Ac, Bm)).astype(np.float64)
    KA = P + 20 + 60 + 1
    ref, mag = np.zeros((KA, KB)), np.zeros((KA, KB))
    CH = 10                                                # steps per chunk
    for t0 in range(0, T, CH):
        t1 = min(T, t0 + CH)
        a = _expand_compact(eng.to_numpy(Ac[t0:t1 + 1]).astype(np.float64), P, fc).reshape(-1, KA)
        b = eng.to_numpy(Bm[t0:t1]).astype(np.float64).reshape(-1, KB)
        ref += a.T @ b
        mag += np.abs(a).T @ np.abs(b)
    worst = 0.0
    for rs, cs in _grad_blocks(P, fc):
        ratio = np.abs(G[rs, cs] - ref[rs, cs]) / mag[rs, cs]
        worst = max(worst, float(ratio.max()))
    print("wgrad_compact, %d rows: max |G - A^T Bm| / (|A|^T |Bm|) = %.3g" % (T * R, worst))
    assert worst <= 1e-7, worst


# ------------------------------------------------------------------------------------------------------------------
# 5. config 2's training step at full size
# ------------------------------------------------------------------------------------------------------------------
def test_config2_training_steps_vs_float64(eng):
    """The trained dm_quadratic_d128 optimizer, B = 128, D = 128, T = 20: two consecutive train steps, each against
    float64 at 5e-4 of every block's largest entry.  The float32 oracle's own error on the same gradient is printed beside
    the kernel's (conditioning vs kernel error)."""
    with open(os.path.join(TRAINED, "dm_quadratic_d128", "cw.l2l-0"), "rb") as f:
        params = {k: {v: np.asarray(a, np.float32) for v, a in m.items()} for k, m in dill.load(f).items()}
    B, D, T = 128, 128, 20
    prob, x0, _ = make_problem("quadratic", B, D, seed=901)
    api = problems.quadratic(B, D, data={"w": prob.w, "y": prob.y, "x": x0})
    prob64 = as_float64(prob)
    tr = Trainer(eng, "dm", params, api, T)
    tr.reset()
    prev = None
    for k in range(2):
        snap = tr.snapshot()
        if prev is not None:
            check_carry(snap, prev, prev32, "carry into step %d" % k)
        got = tr.train_step()
        assert tr.graph.last_path == "fused" and eng.last_unroll_form()[0] == "k_unroll_pair"
        want, prev = tr.reference(prob64, snap)
        errs = block_errors(got, want)
        g32, prev32 = tr.reference(prob, snap, np.float32)
        errs32 = block_errors(g32, want)
        print("config 2 step %d: worst block error HIP %.3g, float32 oracle %.3g" % (k, max(errs.values()), max(errs32.values())))
        worst = max(errs, key=errs.get)
        assert errs[worst] < GRAD_TOL, (k, worst, errs[worst], errs32[worst])
