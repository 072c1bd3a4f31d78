"""What the tests of the five image-net optimizees (mnist_conv, cifar_conv, lenet, nas, vgg16) share, written once for
tests/test_<net>.py, tests/test_<net>_cpu.py and tests/test_conv_edges.py.

``NETS`` says what differs between the nets as data: the float64 torch reference, the problem factory, the engine's
descriptor and entry point, the ABI struct, the names util.get_config and the evaluation driver know the net by, and the
biases that feed a batch norm.  The fixtures (``eng``, and ``oracle_engine`` for a module's own ``engine``) and the data
makers are imported by name into the modules that use them.  The ``check_*`` functions are the bodies the modules had five
copies of: they take a net and that case's own numbers (T, minibatch, data, seeds drawn by the caller), print every figure
they compare, and hold the project's bounds (a module's docstring says where and why its net departs from one):

    the loss                    within 1e-5 relative of float64 (in an unroll: or 3 x the float32 reference's own distance)
    a gradient / variable block within GRAD_TOL of its largest float64 entry, or 3 x the float32 reference's own distance
    a bias feeding a batch norm within 1e-6 of its layer's largest weight-gradient entry (exactly 0 in exact arithmetic)
    a carried array             within CARRY_TOL of its largest entry, or ``state_factor`` x (LSTM state) / 3 x (x, m, v) the
                                float32 oracle's own distance

Each module still owns its inputs (seeds, shapes, which point in weight space), the reasoning in its docstring about why
those, every assertion that is about one net only (pool ties, decision margins, the preconditions on the float32 reference
of nas and vgg16 and their _check_fg), and the order in which it draws: a helper here never draws from a generator the
caller has not handed it.  Nothing here needs a GPU until a HipEngine is made."""
import contextlib
import ctypes as C
import functools
import math
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import conv_reference
import lenet_reference
import nas_reference
import oracle as O
import vgg16_reference
from helpers import ORACLE_CFGS, block_errors, make_params, rel_err
from oracle_engine import OracleEngine
from open_l2o_amd import _abi, _engine, meta, meta_rnnprop_eval, problems, util
from open_l2o_amd.session import Session
from test_meta_api import _net_config
from test_training_gradient import CARRY_TOL, GRAD_TOL, Trainer, _carried, split_carry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NARROW = vgg16_reference.NARROW_CHANNELS


# ---- data ---------------------------------------------------------------------------------------------------------------
def _noisy(synthetic, n, seed):
    """A synthetic data set with a little uniform noise on top, so that no two pooling candidates tie exactly (a tie broken
    differently by rounding moves a gradient to another pixel)."""
    d = synthetic(n, seed=seed)
    rng = np.random.default_rng(seed + 1000)
    flat = d["images"].reshape(n, -1)
    images = (flat + 0.05 * rng.random(flat.shape)).astype(np.float32)
    return {"images": images.reshape(d["images"].shape), "labels": d["labels"]}


def noisy_mnist(n, seed):
    """[n, 28, 28, 1]"""
    d = _noisy(problems.synthetic_mnist, n, seed)
    return {"images": d["images"].reshape(n, 28, 28, 1), "labels": d["labels"]}


def noisy_cifar(n, seed):
    """[n, 32, 32, 3]"""
    return _noisy(problems.synthetic_cifar10, n, seed)


@functools.lru_cache(maxsize=None)
def uniform_cifar(n=64, seed=0):
    """Uniform images (every pixel its own value: no two pooling candidates tie by construction) and labels; shared, so
    nothing modifies them."""
    rng = np.random.default_rng(seed)
    return {"images": rng.random((n, 32, 32, 3)).astype(np.float32), "labels": rng.integers(0, 10, n)}


# ---- the nets -----------------------------------------------------------------------------------------------------------
def _every_other_bias(batch_norm, layers):
    """(index of the bias, index of its layer's weight) of ``layers`` conv layers of (weights1, biases1, gamma, beta)."""
    return [(4 * i + 1, 4 * i) for i in range(layers)] if batch_norm else []


def _net(name, R, ref, desc, struct, problem, synthetic, data, fed, arg=True, config="batch_norm", carry_skip_fed=True):
    """One entry.  R, ref: the reference (its module, or conv_reference's names bound to a shape) and its net class,
    ref(images, labels, arg).  arg: what shapes the net, as
    the descriptor's attribute ``config`` and as R.shapes' argument (batch norm on, or VGG-16's widths); the unrolls and
    meta-gradients of every module run at this one value.  fg / stem / scratch: the engine's entry point, the library's
    prefix (<stem>_fg, <stem>_scratch_floats) and the engine's cached scratch attribute.  problem(**kw): the factory at
    ``arg``.  name is also what util.get_config and the driver's --problem call the net; options: what get_config needs on
    top to reach ``arg``.  synthetic: problems' data maker (the driver's --<its name> N), data: the maker the GPU tests
    use.  fed(batch_norm): (bias, weight) indices of the biases that feed a batch norm; carry_skip: those whose carry into
    the next meta-training step is not compared (under batch norm what feeds the optimizer for them is rounding noise)."""
    return types.SimpleNamespace(
        name=name, R=R, ref=ref, desc=desc, struct=struct, problem=problem, synthetic=synthetic, data=data, fed=fed, arg=arg,
        config=config, fg=name + "_fg", stem="l2o_" + name, floats="l2o_%s_scratch_floats" % name,
        scratch="_%s_scratch" % name, names=R.names(*([] if config == "channels" else [arg])),
        options={"channels": arg} if config == "channels" else {},
        carry_skip=frozenset(kb for kb, _ in fed(True)) if carry_skip_fed else frozenset())


def _lenet(**kw):
    kw.setdefault("conv_channels", (6, 16))
    kw.setdefault("linear_layers", (120, 84))
    return problems.LeNet("cifar10", **kw)


NETS = {n.name: n for n in (
    # (mnist_conv compares the carry of every variable, as test_training_gradient.check_carry's callers do)
    _net("mnist_conv", conv_reference.MNIST, conv_reference.MNIST.ConvNet, _engine.MnistConvDesc, _abi.MnistConv,
         problems.mnist_conv, problems.synthetic_mnist, noisy_mnist, lambda bn: _every_other_bias(bn, 2),
         carry_skip_fed=False),
    _net("cifar_conv", conv_reference.CIFAR, conv_reference.CIFAR.ConvNet, _engine.CifarConvDesc, _abi.CifarConv,
         lambda **kw: problems.cifar10("cifar10", **kw), problems.synthetic_cifar10, noisy_cifar,
         lambda bn: _every_other_bias(bn, 2)),
    _net("lenet", lenet_reference, lenet_reference.LeNet, _engine.LenetDesc, _abi.Lenet, _lenet,
         problems.synthetic_cifar10, noisy_cifar, lenet_reference.bn_fed_biases),
    _net("nas", nas_reference, nas_reference.Nas, _engine.NasDesc, _abi.Nas, lambda **kw: problems.NAS("cifar10", **kw),
         problems.synthetic_cifar10, uniform_cifar, lambda bn: _every_other_bias(bn, 4)),
    _net("vgg16", vgg16_reference, vgg16_reference.Vgg16, _engine.Vgg16Desc, _abi.Vgg16,
         lambda **kw: problems.vgg16_cifar10("cifar10", **{"channels": NARROW, **kw}), problems.synthetic_cifar10,
         uniform_cifar, lambda bn: [], arg=NARROW, config="channels"),
)}


# ---- engines ------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def as_default(engine):
    old = _engine._default_engine
    _engine.set_default_engine(engine)
    try:
        yield engine
    finally:
        _engine.set_default_engine(old)


@pytest.fixture
def eng():
    """A fresh HipEngine, the default engine for the length of one test (imported by name into the modules that use it)."""
    with as_default(_engine.HipEngine()) as e:
        yield e


def oracle_engine(net):
    """The oracle engine plus the net's loss and gradient from the float32 torch reference, under the engine's own method
    name; every call is logged in ``calls``."""
    def fg(self, d, indices, ws, loss, grads):
        self.calls.append(net.fg)
        assert isinstance(d, net.desc)
        arg = getattr(d, net.config)
        ref = net.ref(d.images.numpy(), d.labels.numpy(), arg)
        vs = [w.numpy().reshape(sh) for w, sh in zip(ws, net.R.shapes(arg))]
        f, g = ref.fg(vs, indices.numpy(), want_grad=grads is not None)
        loss.copy_(torch.from_numpy(np.array([f], np.float32)))
        if grads is not None:
            for t, a in zip(grads, g):
                t.copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32)).view_as(t))

    return type("%sOracleEngine" % net.name, (OracleEngine,), {net.fg: fg})()


# ---- one evaluation on the GPU ----------------------------------------------------------------------------------------------
def run_fg(eng, net, desc, rows, w, want_grad=True, fill=0.0):
    """One call of the net's entry point into fresh outputs (the gradients pre-filled with ``fill``): (loss, gradients or
    None) as host arrays."""
    idx = eng.int_tensor(rows)
    ws = [eng.tensor(a) for a in w]
    grads = [eng.zeros(*a.shape) + fill for a in w] if want_grad else None
    loss = eng.zeros(1)
    getattr(eng, net.fg)(desc, idx, ws, loss, grads)
    return eng.to_numpy(loss).copy(), None if grads is None else [eng.to_numpy(g).copy() for g in grads]


def bound(got, want, g32):
    """(largest error of a block, its bound): GRAD_TOL of the largest float64 entry, or 3 x the float32 reference's own
    distance from float64 where that is larger."""
    scale = float(np.abs(want).max())
    return float(np.abs(got - want).max()), max(GRAD_TOL * scale, 3 * float(np.abs(g32 - want).max()))


def check_fg_vs_float64(eng, net, ref, rows, w, f64, g64, f32, g32):
    """The entry point of a net whose biases in front of a batch norm are held to the 1e-6 rule, on the data of the
    reference net ``ref``, against what the caller has evaluated with it (and asserted its own conditions on): the loss,
    every block, then the bit contracts -- a second call gives the same bits, a forward-only call the same loss bits."""
    batch_norm = ref.batch_norm
    desc = net.desc(len(rows), batch_norm, eng.tensor(ref.images), eng.int_tensor(ref.labels))
    loss, grads = run_fg(eng, net, desc, rows, w)
    got_f = float(loss[0])
    print("loss", got_f, f64, "rel %.3e (float32 torch %.3e)" % (abs(got_f - f64) / abs(f64), abs(f32 - f64) / abs(f64)))
    failures = []
    if not abs(got_f - f64) <= 1e-5 * abs(f64):
        failures.append(("loss", got_f, f64))
    fed = dict(net.fed(batch_norm))
    for k, nm in enumerate(net.R.names(batch_norm)):
        got = grads[k].astype(np.float64).reshape(g64[k].shape)
        if k in fed:
            wscale = float(np.abs(g64[fed[k]]).max())
            ratio, ratio32 = float(np.abs(got).max()) / wscale, float(np.abs(g32[k]).max()) / wscale
            print("%-32s |g| / max|dW| %.3e (float32 torch %.3e)" % (nm, ratio, ratio32))
            if not ratio <= 1e-6:
                failures.append((nm, ratio, ratio32))
            continue
        err, bnd = bound(got, g64[k], g32[k])
        print("%-32s err %.3e bound %.3e (float32 torch %.3e) of max %.3e" %
              (nm, err, bnd, float(np.abs(g32[k] - g64[k]).max()), float(np.abs(g64[k]).max())))
        if not err <= bnd:
            failures.append((nm, err, bnd))
    assert not failures, failures
    loss2, grads2 = run_fg(eng, net, desc, rows, w)
    loss3, _ = run_fg(eng, net, desc, rows, w, want_grad=False)
    assert loss2.tobytes() == loss.tobytes() and loss3.tobytes() == loss.tobytes()
    for a, b in zip(grads, grads2):
        assert a.tobytes() == b.tobytes()


# ---- the unroll and the meta-gradient on the GPU ----------------------------------------------------------------------------
def _meta_loss(cfg, params, problem, T, steps=(1,)):
    """(optimizer, meta_loss' ops, one feed per consecutive unroll starting at ``steps``)"""
    if cfg.kind == "rnnprop":
        optimizer = meta_rnnprop_eval.MetaOptimizer(0.95, 0.95, **_net_config(cfg, params, key="rp"))
        ml, _, _, step = optimizer.meta_loss(problem, T)
        return optimizer, ml, [{step: s} for s in steps]
    optimizer = meta.MetaOptimizer(**_net_config(cfg, params))
    return optimizer, optimizer.meta_loss(problem, T), [{} for _ in steps]


def check_unroll_vs_float64(eng, net, cfg_name, T, batch, data, idx, w0=None):
    """meta_loss over the net on the graph's step path, minibatch idx[t] at evaluation t, against a float64 and a float32
    host unroll of the same optimizer (params of seed 43, graph seed 44): fx per step, x at the end per variable.  w0: the
    variables start there and not at the graph's own initialisation."""
    cfg = O.DM_LOGSIGN if cfg_name == "dm_logsign" else O.RNNPROP
    params = make_params(cfg, seed=43, trained_like=True)
    meta.set_random_seed(44)
    problem = net.problem(batch_size=batch, data=data, sampler=lambda ne, b, nd: idx[:ne])
    optimizer, ml, (feed,) = _meta_loss(cfg, params, problem, T)
    with Session() as sess:
        sess.run(ml.reset)
        for v, a in zip(optimizer.graph.x, w0 or ()):
            v.load(a)
        v0 = [np.asarray(v.eval()) for v in optimizer.graph.x]
        res = optimizer.graph.execute(feed, True)
    assert optimizer.graph.last_path == "steps"
    for a, b in zip(v0, w0 or ()):
        assert np.array_equal(a.reshape(b.shape), b)
    fx = np.asarray(res["fx_array"], np.float64)
    xT = [np.asarray(a, np.float64) for a in res["x"]]
    ref = net.ref(data["images"], data["labels"], net.arg)
    outs = {}
    for dt in (np.float64, np.float32):
        p = {m: {v: a.astype(dt) for v, a in d.items()} for m, d in params.items()}
        states = [tuple((h.astype(dt), c.astype(dt)) for h, c in O.net_initial_state(cfg, a.size)) for a in v0]
        fx_r, x_r, _ = O.unroll_multi(lambda vs, t, wg: ref.fg(vs, idx[t], wg), cfg, p, [a.astype(dt) for a in v0],
                                      states, T)
        outs[dt] = (np.asarray(fx_r, np.float64), [np.asarray(a, np.float64) for a in x_r])
    (fx64, x64), (fx32, x32) = outs[np.float64], outs[np.float32]
    assert fx.shape == fx64.shape == (T + 1,)
    for t in range(T + 1):
        print("fx", t, fx[t], fx64[t], fx32[t])
        assert abs(fx[t] - fx64[t]) <= max(1e-5 * abs(fx64[t]), 3 * abs(fx32[t] - fx64[t])), (t, fx[t], fx64[t], fx32[t])
    for nm, g, w64, w32 in zip(net.names, xT, x64, x32):
        err, bnd = bound(g.reshape(w64.shape), w64, w32)
        print("x", nm, "err %.3e bound %.3e" % (err, bnd))
        assert err <= bnd, (nm, err, bnd)


def check_carry(snap, end, end32, what, state_factor=3):
    """The state the graph carried into the next unroll == the reference's end state of the unroll that produced it: within
    CARRY_TOL of each array's largest entry, or of the float32 oracle's own distance 3 x for x, m, v and ``state_factor``
    x for the LSTM state (test_training_gradient.check_carry's rule at 3)."""
    got, ref, r32 = _carried(snap), _carried(end), _carried(end32)
    for nm in ref:
        scale = max(float(np.abs(ref[nm]).max()), 1e-30)
        err = float(np.abs(got[nm] - ref[nm]).max()) / scale
        own = float(np.abs(r32[nm] - ref[nm]).max()) / scale
        print("carry", what, nm, "err %.3e own %.3e" % (err, own))
        factor = state_factor if nm in ("h1", "c1", "h2", "c2") else 3
        assert err < max(CARRY_TOL, factor * own), (what, nm, err, own)


def check_meta_gradient_vs_float64(eng, net, name, T, batch, data, state_factor=3):
    """Two consecutive first-order train steps (params of seed 52, graph seed 53) against helpers.oracle_meta_grad over the
    minibatches the graph drew: every block of the meta-gradient, and what the first step carried into the second."""
    params = make_params(ORACLE_CFGS[name], seed=52, trained_like=True)
    meta.set_random_seed(53)
    tr = Trainer(eng, name, params, net.problem(batch_size=batch, data=data), T)
    shapes = [tuple(v.shape) for v in tr.graph.x]
    assert shapes == net.R.shapes(net.arg)
    ref = net.ref(data["images"], data["labels"], net.arg)
    tr.reset()
    prev = None
    for k in range(2):
        snap = tr.snapshot()
        if prev is not None:
            for j, (sv, ev, e32) in enumerate(zip(snap["vars"], split_carry(prev[0], shapes), split_carry(prev[1], shapes))):
                if j not in net.carry_skip:
                    check_carry(sv, ev, e32, "step %d: carry into variable %d" % (k, j), state_factor)
        got = tr.train_step()
        assert tr.graph.last_path == "steps"
        idx = eng.to_numpy(tr.graph._mlp_idx[0])
        assert idx.shape == (T + 1, batch)
        fg = ref.flat_fg(shapes, idx)
        want, end = tr.reference(fg, snap)
        g32, end32 = tr.reference(fg, snap, np.float32)
        prev = (end, end32)
        errs, errs32 = block_errors(got, want), block_errors(g32, want)
        for blk, e in errs.items():
            print("meta-gradient step", k, blk, "err %.3e float32 oracle %.3e" % (e, errs32[blk]))
            assert e < max(GRAD_TOL, 3 * errs32[blk]), (k, blk, e, errs32[blk])


def check_driver(net, n_synthetic, num_steps, timeout):
    """scripts/evaluate_rnnprop.py with the shipped MLP-trained optimizer, pointed at the net: it ends with a finite figure."""
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "evaluate_rnnprop.py"), "--problem", net.name,
           "--" + net.synthetic.__name__, str(n_synthetic), "--num_steps", str(num_steps),
           "--path", os.path.join(ROOT, "tests", "golden", "trained", "rnnprop_mnist_mlp", "rp.l2l-0")]
    if net.config == "channels":
        cmd += ["--vgg16_channels", ",".join(str(c) for c in net.arg)]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr[-3000:]
    m = re.search(r"Log Mean Final Error: (\S+)", out.stdout)
    assert m and math.isfinite(float(m.group(1))), out.stdout[-2000:]


# ---- without a GPU: the host wiring on the oracle engine --------------------------------------------------------------------
def sampler(idx):
    """A problem's sampler that hands out the rows of idx in order, n_evals at a call."""
    calls = {"n": 0}

    def sample(n_evals, b, n_data):
        out = idx[calls["n"]:calls["n"] + n_evals]
        calls["n"] += n_evals
        return out
    return sample


def check_meta_loss_wiring(engine, net, cfg_name, n_data, T, batch, check_v0=None):
    """meta_loss over util.get_config(<net>) on the step-granular path == the oracle's multi-variable unroll over the same
    float32 evaluations, two chained unrolls; one evaluation per step and unroll went through the engine's entry point."""
    data = net.synthetic(n_data, seed=7)
    idx = np.random.default_rng(8).integers(0, n_data, size=(2 * (T + 1), batch))
    cfg = O.DM_LOGSIGN if cfg_name == "dm_logsign" else O.RNNPROP
    params = make_params(cfg, seed=9, trained_like=True)
    meta.set_random_seed(10)
    problem = util.get_config(net.name, problem_options={"data": data, "batch_size": batch, "sampler": sampler(idx),
                                                         **net.options})[0]
    optimizer, ml, feeds = _meta_loss(cfg, params, problem, T, steps=(1, 1 + T))
    with Session() as sess:
        sess.run(ml.reset)
        v0 = [v.eval() for v in optimizer.graph.x]
        assert [tuple(a.shape) for a in v0] == net.R.shapes(net.arg)
        if check_v0 is not None:
            check_v0(v0)
        loss1, fx1, _ = sess.run([ml.loss, ml.fx, ml.update], feed_dict=feeds[0])
        loss2, fx2, x2, _ = sess.run([ml.loss, ml.fx, ml.x, ml.update], feed_dict=feeds[1])
    assert optimizer.graph.last_path == "steps"
    assert engine.calls.count(net.fg) == 2 * (T + 1)
    ref = net.ref(data["images"], data["labels"], net.arg)
    states = [O.net_initial_state(cfg, a.size) for a in v0]
    if cfg.kind == "rnnprop":
        fx_a, va, sa, ma, va2 = O.unroll_multi(lambda vs, t, wg: ref.fg(vs, idx[t], wg), cfg, params, v0, states, T,
                                               return_moments=True)
        fx_b, vb, _ = O.unroll_multi(lambda vs, t, wg: ref.fg(vs, idx[T + 1 + t], wg), cfg, params, va, sa, T, ms=ma,
                                     vs=va2, step0=1 + T)
    else:
        fx_a, va, sa = O.unroll_multi(lambda vs, t, wg: ref.fg(vs, idx[t], wg), cfg, params, v0, states, T)
        fx_b, vb, _ = O.unroll_multi(lambda vs, t, wg: ref.fg(vs, idx[T + 1 + t], wg), cfg, params, va, sa, T)
    assert rel_err(fx1, fx_a[-1]) < 1e-5 and rel_err(loss1, fx_a.sum()) < 1e-5
    assert rel_err(fx2, fx_b[-1]) < 1e-5 and rel_err(loss2, fx_b.sum()) < 1e-5
    for got, want in zip(x2, vb):
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-7)


def check_meta_minimize_and_refusals(engine, net, n_data, batch, refusal="second_derivatives", replicas=True):
    """One first-order training step on the net runs on the recording step path; second derivatives refuse it with a
    message matching ``refusal``, and (``replicas``) so does the replicas' training step."""
    data = net.synthetic(n_data, seed=11)
    meta.set_random_seed(12)
    opt = meta.MetaOptimizer(**_net_config(O.DM_LOGSIGN, make_params(O.DM_LOGSIGN, seed=13, trained_like=True)))
    problem = net.problem(batch_size=batch, data=data)
    ms = opt.meta_minimize(problem, 2, learning_rate=1e-3)
    w0 = {m: {v: np.array(a) for v, a in d.items()} for m, d in opt._nets["cw"].variables.items()}
    with Session() as sess:
        sess.run(ms.reset)
        c1 = sess.run([ms.fx, ms.update, ms.step])[0]
    assert np.isfinite(c1) and opt.graph.last_path == "steps"
    assert net.fg in engine.calls
    w1 = opt._nets["cw"].variables
    assert any(not np.array_equal(w0[m][v], np.asarray(w1[m][v])) for m in w0 for v in w0[m])
    opt2 = meta.MetaOptimizer(**_net_config(O.DM_LOGSIGN, make_params(O.DM_LOGSIGN, seed=13, trained_like=True)))
    with pytest.raises(NotImplementedError, match=refusal):
        opt2.meta_minimize(problem, 2, learning_rate=1e-3, second_derivatives=True)
    if replicas:
        from open_l2o_amd.replicas import Replicas
        reps = Replicas(opt, [problem, problem], 2)
        with pytest.raises(ValueError, match="problems.mnist"):
            reps.train_step({}, 1e-3)


def check_replicas_one_at_a_time(engine, net):
    """Replicas.run over instances of the net: no multi-instance kernel applies, so they run one after the other ("chip")."""
    from open_l2o_amd.replicas import Replicas
    meta.set_random_seed(14)
    opt = meta.MetaOptimizer(**_net_config(O.DM_LOGSIGN, make_params(O.DM_LOGSIGN, seed=15, trained_like=True)))
    problem = net.problem(batch_size=4, data=net.synthetic(32, seed=16))
    reps = Replicas(opt, [problem, problem], 2)
    reps.reset()
    fx = reps.run({})
    assert reps.last_form == "chip" and fx.shape == (2,) and np.isfinite(fx).all()
    assert engine.calls.count(net.fg) >= 2 * 3


def check_central_differences(ref_net, w, rows, names, g, rng, coords, rtol):
    """The float64 reference's gradient ``g`` at ``w`` against central differences on ``coords`` coordinates of every
    variable, drawn from ``rng``: within rtol of the block's largest entry (of 1e-3 where that is smaller)."""
    h = 1e-6
    for k, a in enumerate(w):
        for j in rng.choice(a.size, size=min(coords, a.size), replace=False):
            wp = [b.copy() for b in w]
            wm = [b.copy() for b in w]
            wp[k].reshape(-1)[j] += h
            wm[k].reshape(-1)[j] -= h
            num = (ref_net.fg(wp, rows, want_grad=False)[0] - ref_net.fg(wm, rows, want_grad=False)[0]) / (2 * h)
            scale = max(np.abs(g[k]).max(), 1e-3)
            assert abs(num - g[k].reshape(-1)[j]) < rtol * scale + 1e-8, (names[k], j, num, g[k].reshape(-1)[j])


def check_batch_bounds(lib, net):
    """<stem>_scratch_floats answers 0 outside minibatches 2 .. 1024; <stem>_fg refuses those, and NULL arguments inside."""
    floats, fg = getattr(lib, net.floats), getattr(lib, net.stem + "_fg")
    m = net.struct()
    m.n_data, m.batch_norm = 100, 1
    for batch, ok in ((1, False), (2, True), (128, True), (1024, True), (1025, False)):
        m.batch = batch
        assert (floats(C.byref(m)) > 0) == ok, batch
        assert fg(C.byref(m), None, None, None, None, None, None) == (_abi.L2O_ERR_ARG if ok else _abi.L2O_ERR_UNSUPPORTED)
