"""problems.LeNet on the MI355X: l2o_lenet_fg (csrc/l2o_lenet.h) against the float64 torch reference (lenet_reference.py),
the unroll of meta_loss over the net against a float64 host unroll, the first-order meta-gradient against
helpers.oracle_meta_grad, and the RNNProp evaluation driver on it.

Bounds (the project's, as test_cifar_conv.py): a gradient block within 5e-4 of its largest entry, or 3 x the float32
reference's own distance from float64 where that is larger (test_training_gradient's rule); the loss within 1e-5 relative;
the four biases that feed a batch norm (exactly 0 in exact arithmetic) within 1e-6 of the largest entry of their layer's
weight gradient.  The images carry a little uniform noise on top of problems.synthetic_cifar10, and the test asserts on
the float64 and float32 reference activations that no two pooling candidates tie exactly (a tie broken differently by
rounding moves a gradient to another pixel): a condition on the inputs that excludes nothing.  Kernel and reference both
pool the normalised pre-activation and apply the sigmoid after (lenet_reference.py says why that is the same net).

The carry of the four batch-norm-fed biases into the second meta-training step is not compared: their gradient is 0 in
exact arithmetic, so what any implementation feeds the optimizer for them is its own rounding noise (test_fg_vs_float64
bounds it), and under RNNProp's g / sqrt(v) that noise steers their trajectories.  Every other carried quantity, the
RNNProp LSTM state included, and every meta-gradient block keeps the 3 x rule (of the float32 oracle's own distance from
float64): the 5 x that test_cifar_conv.py needed for the RNNProp state is not needed here.  Measured on one MI355X, over
both optimizers and the ten compared variables: wherever a carried array was further than CARRY_TOL from float64 (up to
3.2e-4 of its largest entry, the LSTM state of linear_1/w under RNNProp), it was at most 1.65 x the float32 oracle's own
distance; the larger multiples (up to 4.6 x) all belong to arrays within 3e-6, inside CARRY_TOL."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import lenet_reference as R
import oracle as O
from helpers import ORACLE_CFGS, block_errors, make_params
from open_l2o_amd import _engine, meta, meta_rnnprop_eval, problems
from open_l2o_amd.session import Session
from test_meta_api import _net_config
from test_training_gradient import CARRY_TOL, GRAD_TOL, Trainer, _carried, split_carry

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BN_BIASES = {kb for kb, _ in R.bn_fed_biases(True)}


@pytest.fixture
def eng():
    e = _engine.HipEngine()
    old = _engine._default_engine
    _engine.set_default_engine(e)
    yield e
    _engine.set_default_engine(old)


def _data(n, seed):
    d = problems.synthetic_cifar10(n, seed=seed)
    rng = np.random.default_rng(seed + 1000)
    images = (d["images"].reshape(n, -1) + 0.05 * rng.random((n, 3072))).astype(np.float32)
    return {"images": images.reshape(n, 32, 32, 3), "labels": d["labels"]}


def _lenet(**kw):
    return problems.LeNet("cifar10", conv_channels=(6, 16), linear_layers=(120, 84), **kw)


def _check_carry(snap, end, end32, what):
    """test_training_gradient.check_carry's rule (3 x the float32 oracle's own distance, or CARRY_TOL), every figure
    printed."""
    got, ref, r32 = _carried(snap), _carried(end), _carried(end32)
    for nm in ref:
        scale = max(float(np.abs(ref[nm]).max()), 1e-30)
        err = float(np.abs(got[nm] - ref[nm]).max()) / scale
        own = float(np.abs(r32[nm] - ref[nm]).max()) / scale
        print("carry", what, nm, "err %.3e own %.3e" % (err, own))
        assert err < max(CARRY_TOL, 3 * own), (what, nm, err, own)


def _bound(got, want, g32):
    scale = float(np.abs(want).max())
    return float(np.abs(got - want).max()), max(GRAD_TOL * scale, 3 * float(np.abs(g32 - want).max()))


# ------------------------------------------------------------------------------------------------------------------
# 1. one evaluation: l2o_lenet_fg against float64
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("point", ["sample", "init"])
@pytest.mark.parametrize("batch_norm", [True, False])
@pytest.mark.parametrize("batch", [128, 37])
def test_fg_vs_float64(eng, batch, batch_norm, point):
    """``sample``: O(1) activations, non-zero beta and biases; ``init``: the reference's own initialisation scale (all w,
    b ~ N(0, 0.01^2), beta 0), where the normalised signal comes from 1e-2-scale pre-activations.

    Measured on one MI355X: every block within 3e-7 of its largest float64 entry (float32 torch on the CPU: 4e-7), the
    loss within 3.2e-7 relative.  The batch-norm-fed biases, as a fraction of their layer's largest weight-gradient entry,
    over the four batch-norm cases (float32 torch autograd's own ratio on the same inputs in brackets): conv_2d_0/b
    0.8-4.4e-7 (0.6-1.5e-6), conv_2d_1/b 1.2-5.5e-7 (0.4-1.5e-6), linear_0/b 1.5-3.9e-8 (3.6-8.6e-7), linear_1/b
    0.1-1.9e-7 (1.8-4.9e-7): all inside the 1e-6.  With a single float for the linear layers' batch mean linear_0/b was
    at 2.6e-6 at [128-True-sample], which is why k_ln_fc keeps that mean as two floats."""
    n = 300
    data = _data(n, seed=batch + batch_norm)
    net = R.LeNet(data["images"], data["labels"], batch_norm)
    w = R.sample_weights(batch_norm, seed=batch) if point == "sample" else R.init_weights(batch_norm, seed=batch)
    rows = np.random.default_rng(batch).integers(0, n, batch)
    f64, g64 = net.fg([a.astype(np.float64) for a in w], rows)
    # no pooling window ties: in float64 neither among the pre-activations nor among their sigmoids (so the reference's
    # order, pool after the sigmoid, routes the same gradient), in float32 among the pre-activations both the kernel and
    # the float32 reference rank.  The float32 SIGMOIDS are not asserted on: at [init, no batch norm] 29 (minibatch 128)
    # and 3 (minibatch 37) windows tie there, so "no ties in either precision" does not hold for the post-sigmoid values
    # (lenet_reference.py)
    assert R.pool_ties(net.last_pre_pool) == 0 and R.pool_ties(net.last_pool_inputs) == 0
    f32, g32 = net.fg(w, rows)
    assert R.pool_ties(net.last_pre_pool) == 0
    d = _engine.LenetDesc(batch, batch_norm, eng.tensor(net.images), eng.int_tensor(data["labels"]))
    idx = eng.int_tensor(rows)
    ws = [eng.tensor(a) for a in w]
    grads = [eng.zeros(*a.shape) for a in w]
    loss = eng.zeros(1)
    eng.lenet_fg(d, idx, ws, loss, grads)
    got_f = float(eng.to_numpy(loss)[0])
    got = [eng.to_numpy(g).astype(np.float64).reshape(a.shape) for g, a in zip(grads, g64)]
    print("loss", got_f, f64, "rel %.3e (float32 torch %.3e)" % (abs(got_f - f64) / abs(f64), abs(f32 - f64) / abs(f64)))
    assert abs(got_f - f64) <= 1e-5 * abs(f64), (got_f, f64)
    names = R.names(batch_norm)
    fed = dict(R.bn_fed_biases(batch_norm))
    failures = []
    for k, nm in enumerate(names):
        if k in fed:
            wscale = float(np.abs(g64[fed[k]]).max())
            ratio, ratio32 = float(np.abs(got[k]).max()) / wscale, float(np.abs(g32[k]).max()) / wscale
            print("%-32s |g| / max|dW| %.3e (float32 torch %.3e)" % (nm, ratio, ratio32))
            if ratio > 1e-6:
                failures.append((nm, ratio, ratio32))
            continue
        err, bound = _bound(got[k], g64[k], g32[k])
        scale = float(np.abs(g64[k]).max())
        print("%-32s err %.3e bound %.3e (float32 torch %.3e) of max %.3e" % (nm, err, bound,
                                                                               float(np.abs(g32[k] - g64[k]).max()), scale))
        if not err <= bound:
            failures.append((nm, err, bound))
    assert not failures, failures
    # bit-reproducible; forward only gives the same loss
    grads2 = [eng.zeros(*a.shape) for a in w]
    loss2, loss3 = eng.zeros(1), eng.zeros(1)
    eng.lenet_fg(d, idx, ws, loss2, grads2)
    eng.lenet_fg(d, idx, ws, loss3, None)
    assert eng.to_numpy(loss2)[0] == got_f and eng.to_numpy(loss3)[0] == got_f
    for a, b in zip(grads, grads2):
        assert np.array_equal(eng.to_numpy(a), eng.to_numpy(b))


# ------------------------------------------------------------------------------------------------------------------
# 2. the unroll: meta_loss over the net, T = 20, against a float64 host unroll
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", ["dm_logsign", "rnnprop"])
def test_unroll_vs_float64(eng, net):
    T, batch, n = 20, 128, 512
    data = _data(n, seed=41)
    idx = np.random.default_rng(42).integers(0, n, size=(T + 1, batch))
    cfg = O.DM_LOGSIGN if net == "dm_logsign" else O.RNNPROP
    params = make_params(cfg, seed=43, trained_like=True)
    meta.set_random_seed(44)
    problem = _lenet(batch_size=batch, data=data, sampler=lambda ne, b, nd: idx[:ne])
    feed = {}
    if cfg.kind == "rnnprop":
        optimizer = meta_rnnprop_eval.MetaOptimizer(0.95, 0.95, **_net_config(cfg, params, key="rp"))
        ml, _, _, step = optimizer.meta_loss(problem, T)
        feed = {step: 1}
    else:
        optimizer = meta.MetaOptimizer(**_net_config(cfg, params))
        ml = optimizer.meta_loss(problem, T)
    with Session() as sess:
        sess.run(ml.reset)
        v0 = [v.eval() for v in optimizer.graph.x]
        res = optimizer.graph.execute(feed, True)
    assert optimizer.graph.last_path == "steps"
    fx = np.asarray(res["fx_array"], np.float64)
    xT = [np.asarray(a, np.float64) for a in res["x"]]
    ref = R.LeNet(data["images"], data["labels"], True)
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
    for k, (g, w64, w32) in enumerate(zip(xT, x64, x32)):
        err, bound = _bound(g.reshape(w64.shape), w64, w32)
        print("x", R.names(True)[k], "err %.3e bound %.3e" % (err, bound))
        assert err <= bound, (R.names(True)[k], err, bound)


# ------------------------------------------------------------------------------------------------------------------
# 3. the meta-gradient: two consecutive train steps against helpers.oracle_meta_grad
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dm_logsign", "rnnprop"])
def test_meta_gradient_vs_float64(eng, name):
    T, batch = 10, 128
    data = _data(1024, seed=51)
    params = make_params(ORACLE_CFGS[name], seed=52, trained_like=True)
    meta.set_random_seed(53)
    tr = Trainer(eng, name, params, _lenet(batch_size=batch, data=data), T)
    shapes = [tuple(v.shape) for v in tr.graph.x]
    assert shapes == R.shapes(True)
    ref = R.LeNet(data["images"], data["labels"], True)
    tr.reset()
    prev = None
    for k in range(2):
        snap = tr.snapshot()
        if prev is not None:
            for j, (sv, ev, e32) in enumerate(zip(snap["vars"], split_carry(prev[0], shapes), split_carry(prev[1], shapes))):
                if j in BN_BIASES:
                    continue
                _check_carry(sv, ev, e32, "step %d: carry into variable %d" % (k, j))
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


# ------------------------------------------------------------------------------------------------------------------
# 4. the RNNProp evaluation driver with the shipped MLP-trained optimizer, pointed at LeNet
# ------------------------------------------------------------------------------------------------------------------
def test_evaluate_rnnprop_driver():
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "evaluate_rnnprop.py"), "--problem", "lenet",
           "--synthetic_cifar10", "1024", "--num_steps", "40",
           "--path", os.path.join(ROOT, "tests", "golden", "trained", "rnnprop_mnist_mlp", "rp.l2l-0")]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    m = re.search(r"Log Mean Final Error: (\S+)", out.stdout)
    assert m and math.isfinite(float(m.group(1))), out.stdout[-2000:]
