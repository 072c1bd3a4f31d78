"""The meta-gradient of the MNIST optimizee (problems.mnist, the project's default training job) against a float64
reference.  Every train step's gradient (captured in front of the meta-Adam) is compared with helpers.oracle_meta_grad
over helpers.mnist_fg -- all of the MLP's variables as one flat vector through the shared coordinate-wise net -- started
from a snapshot of what that step started from, on the minibatch rows the step consumed: they are read back from the
graph's index buffer (_mlp_idx), so the default minibatches drawn on the device are the ones tested.  Bound: every
weight-gradient block within 5e-4 of its largest entry, or 3 x the float32 oracle's own distance from float64 where
that is larger; the carried state per variable as test_training_gradient.check_carry holds it.

  * consecutive unrolls (reset, 3 steps, reset, 1 step) on the 784-20-10 MLP at minibatch 64, T = 20;
  * every recording form, each asserted by its path and flags: l2o_mlp_unroll_record FAST and generic, the step plan,
    the plain steps; relu;
  * deeper MLPs: 6 and 8 panels (the limit of one multi-panel BPTT launch) and ragged widths, one launch each;
  * the random-scaling training forks (meta_dm_train / meta_rnnprop_train) with an x-scale feed, on MNIST and on the
    two-CU recording kernel;
  * the trained config-5 optimizer, two consecutive steps.
"""
import os

import dill
import numpy as np
import pytest

import oracle as O
from helpers import ORACLE_CFGS, as_float64, block_errors, make_params, make_problem, mnist_fg
from open_l2o_amd import _engine, meta, problems
from test_training_gradient import GRAD_TOL, Trainer, _carried, check_carry, split_carry, spy_bwd_unroll

pytestmark = pytest.mark.gpu

TRAINED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trained")


@pytest.fixture
def eng():
    e = _engine.HipEngine()
    old = _engine._default_engine
    _engine.set_default_engine(e)
    yield e
    _engine.set_default_engine(old)


def _shapes(layers):
    widths = [784] + list(layers) + [10]
    return [sh for l in range(len(widths) - 1) for sh in ((widths[l], widths[l + 1]), (widths[l + 1],))]


def _params(name, seed):
    """Weights of a trained-like optimizer (helpers.make_params).  The identity-input DM net takes the raw gradient: at
    that size its unroll on the MLP is chaotic from the second unroll on (the float32 oracle lands 379 x the gradient's
    largest entry away from float64), so its output layer is scaled down a further 10 x, as a net trained there would
    be."""
    p = make_params(ORACLE_CFGS[name], seed=seed, trained_like=True)
    if name == "dm":
        p["linear"] = {v: (a * 0.1).astype(np.float32) for v, a in p["linear"].items()}
    return p


class MnistCase(object):
    """A Trainer on problems.mnist with its float64 / float32 reference: step() runs one train step and compares."""

    def __init__(self, eng, name, params, T, batch=64, layers=(20,), activation="sigmoid", data=None, fork=False,
                 scales=None, seed=0):
        self.eng, self.T, self.batch = eng, T, batch
        data = problems.synthetic_mnist(1024, seed=20) if data is None else data
        self.mlp = O.MnistMLP(data["images"], data["labels"].astype(np.int32), activation)
        meta.set_random_seed(seed)
        self.tr = Trainer(eng, name, params, problems.mnist(layers=layers, activation=activation, batch_size=batch,
                                                            data=data), T, fork=fork)
        self.shapes = [tuple(v.shape) for v in self.tr.graph.x]
        assert self.shapes == _shapes(layers)                 # (graph order == the MLP's [w0, b0, w1, b1, ...])
        self.scales = scales
        if scales is not None:
            self.tr.scale_feed = [s.astype(np.float32) for s in scales]
        self.prev, self.fresh = None, True
        self.worst, self.worst32 = {}, {}

    def reset(self):
        self.tr.reset()
        self.prev, self.fresh = None, True

    def step(self, what, check=True, carry=True):
        """One train step: the carry into it (per variable), its gradient against float64.  Returns the block errors
        of the HIP gradient and of the float32 oracle's.  check=False: only the step (and nothing to carry-check the
        next one against).  carry=False: the carry's errors are printed, not asserted."""
        tr = self.tr
        fresh, self.fresh = self.fresh, False
        if not check:
            tr.train_step()
            self.prev = None
            return None
        snap = tr.snapshot()
        if fresh:
            assert snap["step0"] == 1 and not any(a.any() for p in snap["vars"] for hc in p["state"] for a in hc)
        else:
            assert any(a.any() for hc in snap["state"] for a in hc)                  # a carried, non-zero start
        if self.prev is not None:
            for j, (sv, ev, e32) in enumerate(zip(snap["vars"], split_carry(self.prev[0], self.shapes),
                                                  split_carry(self.prev[1], self.shapes))):
                if carry:
                    check_carry(sv, ev, e32, "%s: carry into variable %d" % (what, j))
                else:
                    print("  %s: carry into variable %d, of each array's largest entry: HIP / float32 oracle %s" % (
                        what, j, carry_errors(sv, ev, e32)))
        got = tr.train_step()
        idx = self.eng.to_numpy(tr.graph._mlp_idx[0])                           # the rows this step consumed
        assert idx.shape == (self.T + 1, self.batch)
        fg = mnist_fg(self.mlp, self.shapes, idx, self.scales)
        want, end = tr.reference(fg, snap)
        g32, end32 = tr.reference(fg, snap, np.float32)
        self.prev = (end, end32)
        errs, errs32 = check_grad32(got, want, g32, what)
        for k in errs:
            self.worst[k] = max(self.worst.get(k, 0.0), errs[k])
            self.worst32[k] = max(self.worst32.get(k, 0.0), errs32[k])
        return errs, errs32

    def report(self, what):
        hip, f32 = max(self.worst.values()), max(self.worst32.values())
        print("%s: worst block error HIP %.3g, float32 oracle %.3g" % (what, hip, f32))


def carry_errors(snap, end, end32):
    got, ref, r32 = _carried(snap), _carried(end), _carried(end32)
    out = []
    for nm in ref:
        scale = max(float(np.abs(ref[nm]).max()), 1e-30)
        out.append("%s %.2g / %.2g" % (nm, float(np.abs(got[nm] - ref[nm]).max()) / scale,
                                       float(np.abs(r32[nm] - ref[nm]).max()) / scale))
    return ", ".join(out)


def check_grad32(got, want, g32, what):
    """Every block within GRAD_TOL of its largest entry -- or within 3 x the float32 oracle's own error where that is
    larger (printed when it is)."""
    errs, errs32 = block_errors(got, want), block_errors(g32, want)
    for k, e in errs.items():
        bound = max(GRAD_TOL, 3 * errs32[k])
        assert e < bound, (what, k, e, errs32[k])
        if bound > GRAD_TOL:
            print("  %s %s: float32 oracle at %.3g, bound %.3g, HIP %.3g" % (what, "/".join(k), errs32[k], bound, e))
    return errs, errs32


# ------------------------------------------------------------------------------------------------------------------
# 1. consecutive unrolls: reset, 3 train steps that carry, reset, 1 more
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dm_logsign", "rnnprop"])
def test_mnist_consecutive_unrolls_vs_float64(eng, name):
    """The harness' epoch on the 784-20-10 sigmoid MLP at minibatch 64 (l2o_mlp_unroll_record's FAST form, the
    default), T = 20: every step against float64 from its own start on the rows it drew, the carry between steps,
    `reset` restarting from the zero state.  (Not the identity-input DM net: its MNIST meta-gradient is ill-conditioned
    -- the float32 oracle alone lands up to 1.7e-4 of a block's largest entry from float64, the HIP path 1.3e-3, the
    same under all three backward pipelines -- so it would measure the conditioning, not the kernels; MNIST's default
    net is LogAndSign, util.get_config("mnist").)"""
    c = MnistCase(eng, name, _params(name, seed=21), T=20, seed=22)
    for k, do_reset in enumerate((True, False, False, True)):
        if do_reset:
            c.reset()
        c.step("step %d" % k)
        assert c.tr.graph.last_path == "mlp_unroll"
    c.report("consecutive %s" % name)


# ------------------------------------------------------------------------------------------------------------------
# 2. every recording form, on the second unroll
# ------------------------------------------------------------------------------------------------------------------
# (form, minibatch, activation): "fast" / "generic" = l2o_mlp_unroll_record (FAST: minibatch 64; generic loops with
# L2O_MLP_UNROLL_RECORD_GENERIC=1), "plan" = the step plan (L2O_NO_MLP_UNROLL_RECORD=1), "steps" = plain steps
# (+ L2O_NO_STEP_PLAN=1)
# (the identity-input DM net only where its unroll is well-conditioned enough to measure the kernels: see
# test_mnist_consecutive_unrolls_vs_float64)
RECORD_FORMS = [("fast", 64, "sigmoid"), ("fast", 64, "relu"), ("generic", 16, "sigmoid"), ("generic", 50, "relu"),
                ("plan", 64, "relu"), ("plan", 50, "sigmoid"), ("steps", 64, "sigmoid")]
RECORD_CASES = [pytest.param(name, *f, id="%s-%s-%d-%s" % ((name,) + f)) for name in ("dm", "dm_logsign", "rnnprop")
                for f in RECORD_FORMS if name != "dm" or f not in (("fast", 64, "sigmoid"), ("generic", 50, "relu"))]


@pytest.mark.parametrize("name,form,batch,activation", RECORD_CASES)
def test_mnist_recording_form_vs_float64(eng, name, form, batch, activation, monkeypatch):
    """The gradient built from each recording form's history on the second unroll (from carried state); the form is
    asserted after every step: the path the graph took, which plan it built and, for l2o_mlp_unroll_record, whether the
    kernel's FAST instantiation applies."""
    for var in ("L2O_MLP_UNROLL_RECORD_GENERIC", "L2O_NO_MLP_UNROLL_RECORD", "L2O_NO_STEP_PLAN"):
        monkeypatch.delenv(var, raising=False)
    if form == "generic":
        monkeypatch.setenv("L2O_MLP_UNROLL_RECORD_GENERIC", "1")
    if form in ("plan", "steps"):
        monkeypatch.setenv("L2O_NO_MLP_UNROLL_RECORD", "1")
    if form == "steps":
        monkeypatch.setenv("L2O_NO_STEP_PLAN", "1")
    c = MnistCase(eng, name, _params(name, seed=23), T=6, batch=batch, activation=activation, seed=24)
    g = c.tr.graph
    c.reset()
    for k in range(2):
        c.step("%s step %d" % (form, k), check=k == 1)
        fast = eng.mlp_unroll_supported(g.slots[0].net.spec, g._mlp_desc(g.terms[0]))
        if form in ("fast", "generic"):
            assert g.last_path == "mlp_unroll" and "_mlp_record_plan" in g.__dict__ and "_step_plan" not in g.__dict__
            assert fast == (2 if form == "fast" else 1), fast
        else:
            assert g.last_path == "steps" and "_mlp_record_plan" not in g.__dict__
            assert ("_step_plan" in g.__dict__) == (form == "plan")
    c.report("%s %s minibatch %d %s" % (form, name, batch, activation))


# ------------------------------------------------------------------------------------------------------------------
# 3. deeper MLPs: several panels in one BPTT launch
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layers", [(20, 20), (20, 20, 20), (13, 32, 7)])
@pytest.mark.parametrize("name", ["dm", "dm_logsign", "rnnprop"])
def test_mnist_deeper_vs_float64(eng, name, layers, monkeypatch):
    """problems.mnist with two or three hidden layers (the step-granular kernels): 6 or 8 panels -- 8 is the limit of
    one multi-panel BPTT launch -- and ragged tiles ((13, 32, 7): four of its eight panels end in a part tile).  The engine is spied
    on: each train step goes through ONE l2o_cwlstm_bwd_unroll launch holding every panel."""
    launches = spy_bwd_unroll(eng, monkeypatch)
    c = MnistCase(eng, name, _params(name, seed=25), T=6, batch=32, layers=layers, seed=26)
    c.reset()
    for k in range(2):
        c.step("%r step %d" % (layers, k), check=k == 1)
        assert c.tr.graph.last_path == "steps"
        assert launches == [[(1, int(np.prod(sh))) for sh in c.shapes]] * (k + 1), launches
    c.report("deeper %s %r" % (name, layers))


# ------------------------------------------------------------------------------------------------------------------
# 4. the random-scaling training forks
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["fast", "plan"])
@pytest.mark.parametrize("name", ["dm_logsign", "rnnprop"])
def test_mnist_train_fork_with_x_scale_vs_float64(eng, name, form, monkeypatch):
    """meta_dm_train / meta_rnnprop_train.MetaOptimizer(0, ...) on MNIST with an exp(U(-1, 1)) scale feed per coordinate
    (DM/util.py:40-54; the same feed for every unroll of the epoch): the MLP is evaluated at x * s and stepped on
    s * grad f(x * s), through l2o_mlp_unroll_record and through the step plan."""
    monkeypatch.delenv("L2O_MLP_UNROLL_RECORD_GENERIC", raising=False)
    monkeypatch.delenv("L2O_NO_STEP_PLAN", raising=False)
    if form == "plan":
        monkeypatch.setenv("L2O_NO_MLP_UNROLL_RECORD", "1")
    else:
        monkeypatch.delenv("L2O_NO_MLP_UNROLL_RECORD", raising=False)
    rng = np.random.default_rng(27)
    scales = [np.exp(rng.uniform(-1, 1, sh)).astype(np.float32) for sh in _shapes((20,))]
    c = MnistCase(eng, name, _params(name, seed=28), T=20, fork=True,
                  scales=scales, seed=29)
    c.reset()
    for k in range(2):
        c.step("x-scale %s step %d" % (form, k))
        g = c.tr.graph
        assert g.last_path == ("mlp_unroll" if form == "fast" else "steps")
        assert ("_step_plan" in g.__dict__) == (form == "plan")
    c.report("x-scale %s %s" % (form, name))


@pytest.mark.parametrize("name", ["dm", "dm_logsign", "rnnprop"])
def test_quadratic_train_fork_with_x_scale_vs_float64(eng, name):
    """The same forks on the analytic quadratic 8 x 128 through the fused recording kernel (k_unroll_pair) with a scale
    feed: the reference unrolls f(x * s) with s * grad f(x * s)."""
    T, B, D = 20, 8, 128
    prob, x0, _ = make_problem("quadratic", B, D, seed=30, stddev=0.2)
    api = problems.quadratic(B, D, data={"w": prob.w, "y": prob.y, "x": x0})
    s = np.exp(np.random.default_rng(31).uniform(-1, 1, (B, D))).astype(np.float32)

    def scaled(p):
        sc = s.astype(p.w.dtype)
        return lambda x, t: (p.f(x * sc), p.grad(x * sc) * sc)
    tr = Trainer(eng, name, make_params(ORACLE_CFGS[name], seed=32, trained_like=True), api, T, fork=True)
    tr.scale_feed = [s]
    tr.reset()
    prev = None
    for k in range(2):
        snap = tr.snapshot()
        if prev is not None:
            check_carry(snap, *prev, "carry into step %d" % k)
        got = tr.train_step()
        assert tr.graph.last_path == "fused" and eng.last_unroll_form()[0] == "k_unroll_pair", eng.last_unroll_form()
        want, end = tr.reference(scaled(as_float64(prob)), snap)
        g32, end32 = tr.reference(scaled(prob), snap, np.float32)
        prev = (end, end32)
        errs, errs32 = check_grad32(got, want, g32, "step %d" % k)
        print("x-scale quadratic %s step %d: worst block error HIP %.3g, float32 oracle %.3g"
              % (name, k, max(errs.values()), max(errs32.values())))


# ------------------------------------------------------------------------------------------------------------------
# 5. the trained config-5 optimizer
# ------------------------------------------------------------------------------------------------------------------
def test_config5_training_steps_vs_float64(eng):
    """The committed RNNProp optimizer meta-trained on the 784-20-10 MLP (tests/golden/trained/rnnprop_mnist_mlp) on
    bench.py's config-5 data, minibatch 64, T = 20: two consecutive train steps against float64.  The float32 oracle's
    own error on the same gradient is printed beside the kernel's, per block.  The carry into the second step is printed,
    not asserted: after 20 steps of the trained net the HIP c2 is 1.1e-4 of its largest entry from float64, 4.4 x the
    float32 oracle's 2.5e-5 (on the sigmoid MLP the HIP forward's rounding is several times the oracle's: the gradient
    errors are the same under every backward pipeline), and the trained RNNProp amplifies it; the gradient itself is
    held to the bound from the HIP snapshot."""
    with open(os.path.join(TRAINED, "rnnprop_mnist_mlp", "rp.l2l-0"), "rb") as f:
        params = {k: {v: np.asarray(a, np.float32) for v, a in m.items()} for k, m in dill.load(f).items()}
    data = problems.synthetic_mnist(4096, seed=5, label_noise=0.1)
    c = MnistCase(eng, "rnnprop", params, T=20, data=data, seed=33)
    c.reset()
    for k in range(2):
        errs, errs32 = c.step("config 5 step %d" % k, carry=False)
        assert c.tr.graph.last_path == "mlp_unroll"
        print("config 5 step %d:" % k)
        for key in sorted(errs):
            print("   %-28s HIP %.3g  float32 oracle %.3g" % ("/".join(key), errs[key], errs32[key]))
    c.report("config 5")
