"""Replicas.train_step -- one meta-training step on N MNIST replicas that share one optimizer -- on the oracle engine
(the whole-chip recording path, graph by graph): the gradient handed to the meta-Adam is the MEAN of the N single-replica
meta-gradients (each what UnrollGraph.train_step's launch + _backward computes for that replica alone, from the same
start on the same minibatches), it is within GRAD_TOL of the float64 mean of helpers.oracle_meta_grad, and the weights
after the step are one Adam step on it.  A world-size-2 gloo run with two replicas per rank averages over all four
replicas and keeps the ranks' weights identical, from ranks that start from different weights."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import oracle as O  # noqa: E402
from helpers import ORACLE_CFGS, block_errors, make_params, mnist_fg, oracle_meta_grad  # noqa: E402
from open_l2o_amd import _engine, meta, meta_rnnprop_eval, problems  # noqa: E402
from open_l2o_amd.replicas import Replicas  # noqa: E402
from test_meta_api import _net_config  # noqa: E402
from test_training_gradient import GRAD_TOL  # noqa: E402

REL_MEAN = 1e-6          # pooled BPTT vs the mean of the single-replica gradients: only the summation order differs


def sampler_of(idx):
    calls = {"n": 0}

    def sampler(n_evals, b, n_data):
        out = idx[calls["n"]:calls["n"] + n_evals]
        calls["n"] += n_evals
        return out
    return sampler


def make_replicas(name, params, data, idxs, T, seed):
    """N problems.mnist replicas (minibatch 64) of one optimizer; replica j draws its minibatches from idxs[j]."""
    cfg = ORACLE_CFGS[name]
    meta.set_random_seed(seed)
    probs = [problems.mnist(layers=(20,), batch_size=64, data=data, sampler=sampler_of(ix)) for ix in idxs]
    if cfg.kind == "rnnprop":
        opt = meta_rnnprop_eval.MetaOptimizer(0.95, 0.95, **_net_config(cfg, params, key="rp"))
    else:
        opt = meta.MetaOptimizer(**_net_config(cfg, params))
    return Replicas(opt, probs, T)


def net_key(reps):
    return "rp" if reps.graphs[0].rnnprop else "cw"


def capture_adam(reps):
    """The gradients every meta-step of the replicas hands to the Adam of graphs[0] (float64 copies)."""
    g0, key, caps = reps.graphs[0], net_key(reps), []
    orig = g0._adam_apply
    g0._adam_apply = lambda grads, lr_, **kw: (
        caps.append({k: np.array(v, np.float64) for k, v in grads[key].items()}), orig(grads, lr_, **kw))[1]
    return caps


def live_buffers(g):
    out = [v.value for v in g.x]
    for s in g.slots:
        out.append(s.state.packed)
        if s.m is not None:
            out += [s.m, s.v]
    return out


def snapshot(eng, g, key, step0):
    """What graph g's next unroll starts from, as test_training_gradient.Trainer.snapshot holds it (all variables
    concatenated in the graph's order: they go through the same coordinate-wise net)."""
    w = {m: {v: np.asarray(a, np.float64).copy() for v, a in d.items()} for m, d in g.nets[key].variables.items()}
    slot_of = {s.var_index: s for s in g.slots}
    xs, st, ms, vs = [], [[], [], [], []], [], []
    for j, var in enumerate(g.x):
        s = slot_of[j]
        for l, a in enumerate(eng.state_unpack(s.state.packed, s.state.B, s.state.D)):
            st[l].append(eng.to_numpy(a).astype(np.float64))
        xs.append(var.eval().astype(np.float64).reshape(-1))
        if g.rnnprop:
            ms.append(eng.to_numpy(s.m).astype(np.float64).reshape(-1))
            vs.append(eng.to_numpy(s.v).astype(np.float64).reshape(-1))
    state = ((np.concatenate(st[0]), np.concatenate(st[1])), (np.concatenate(st[2]), np.concatenate(st[3])))
    return dict(w=w, step0=step0, x=np.concatenate(xs), state=state,
                m=np.concatenate(ms) if g.rnnprop else None, v=np.concatenate(vs) if g.rnnprop else None)


def single_gradients(reps, feed):
    """Every replica's own meta-gradient from where it stands (its launch + _backward, as UnrollGraph.train_step does in
    front of Adam), then its inputs back and its minibatches kept for the replicas' step.  Returns (grads, snapshots,
    minibatch rows) per replica."""
    eng, key, T = reps.graphs[0].engine, net_key(reps), reps.len_unroll
    step0 = int(feed[reps.step]) if feed else 1
    grads, snaps, idxs = [], [], []
    for g in reps.graphs:
        snaps.append(snapshot(eng, g, key, step0))
        live = live_buffers(g)
        bak = [t.clone() for t in live]
        rec = {}
        g.launch(reps._feed(g, feed), True, record=rec)
        gr = g._backward(T, rec)
        grads.append({k: np.array(v, np.float64) for k, v in gr[key].items()})
        idxs.append(eng.to_numpy(g._mlp_idx[0]).copy())
        for t, b in zip(live, bak):
            t.copy_(b)
        g._reuse_minibatches = True                      # (the replicas' step consumes the same rows)
    return grads, snaps, idxs


def replica_step(reps, feed, lr, caps):
    n = len(caps)
    try:
        out = reps.train_step(feed, lr)
    finally:
        for g in reps.graphs:
            g._reuse_minibatches = False
    assert len(caps) == n + 1
    return out, caps[-1]


def mean_of(grads):
    return {k: np.mean([g[k] for g in grads], axis=0) for k in grads[0]}


def check_rel(got, want, tol, what):
    for k, w in want.items():
        err = float(np.abs(np.asarray(got[k], np.float64).reshape(w.shape) - w).max()) / max(float(np.abs(w).max()), 1e-30)
        assert err < tol, (what, k, err)


def adam_first_step(w0, g, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    """TF-1.x Adam's first update (t = 1, zero moments), float32 as _adam_apply does it."""
    f = np.float32
    lr_t = f(lr * np.sqrt(1.0 - beta2) / (1.0 - beta1))
    g = g.astype(np.float32)
    m = f(1.0 - beta1) * g
    v = f(1.0 - beta2) * g * g
    return w0.astype(np.float32) - lr_t * m / (np.sqrt(v) + f(eps))


@pytest.fixture
def oracle_engine():
    from oracle_engine import OracleEngine
    old = _engine._default_engine
    _engine.set_default_engine(OracleEngine())
    yield
    _engine.set_default_engine(old)


@pytest.mark.parametrize("name", ["rnnprop", "dm_logsign"])
def test_train_step_is_the_mean_of_three_replicas(oracle_engine, name):
    T, n, lr = 4, 3, 1e-3
    data = problems.synthetic_mnist(300, seed=21)
    idxs = [np.random.default_rng(40 + j).integers(0, 300, size=(4 * (T + 1), 64)) for j in range(n)]
    params = make_params(ORACLE_CFGS[name], seed=41, trained_like=True)
    reps = make_replicas(name, params, data, idxs, T, seed=5)
    caps = capture_adam(reps)
    key = net_key(reps)
    mlp = O.MnistMLP(data["images"], data["labels"].astype(np.int32), "sigmoid")
    shapes = [tuple(v.shape) for v in reps.graphs[0].x]
    reps.reset()
    feed = {reps.step: 1} if reps.graphs[0].rnnprop else {}
    singles, snaps, rows = single_gradients(reps, feed)
    w0 = {m: {v: np.asarray(a, np.float32).copy() for v, a in d.items()} for m, d in reps.graphs[0].nets[key].variables.items()}
    out, got = replica_step(reps, feed, lr, caps)
    assert reps.last_form == "chip"
    assert out["fx"].shape == (n,) and np.all(np.isfinite(out["fx"])) and len(reps.fx_arrays) == n
    np.testing.assert_allclose(out["loss"], np.mean([f.sum() for f in reps.fx_arrays]), rtol=1e-6)
    # == the mean of the three single-replica gradients (same starts, same minibatches)
    check_rel(got, mean_of(singles), REL_MEAN, "mean of the single-replica gradients")
    assert not np.allclose(singles[0][("lstm_1", "w_gates")], singles[1][("lstm_1", "w_gates")])   # (three different replicas)
    # == the float64 mean of the reference meta-gradients, within the suite's bound
    want = {}
    cfg = ORACLE_CFGS[name]
    for snap, ix in zip(snaps, rows):
        st = tuple((h, c) for h, c in snap["state"])
        g64, _ = oracle_meta_grad(cfg, snap["w"], mnist_fg(mlp, shapes, ix), snap["x"], st, T, m0=snap["m"], v0=snap["v"],
                                  step0=snap["step0"])
        for mod, d in g64.items():
            for var, a in d.items():
                want.setdefault(mod, {}).setdefault(var, []).append(a)
    want = {mod: {var: np.mean(a, axis=0) for var, a in d.items()} for mod, d in want.items()}
    errs = block_errors(got, want)
    assert max(errs.values()) < GRAD_TOL, errs
    # the weights after the step: one Adam step on that mean
    w1 = reps.graphs[0].nets[key].variables
    for (mod, var), g in got.items():
        np.testing.assert_allclose(w1[mod][var], adam_first_step(w0[mod][var], g.reshape(w0[mod][var].shape), lr),
                                   rtol=1e-6, atol=1e-9)


def test_refusals(oracle_engine):
    T = 2
    data = problems.synthetic_mnist(100, seed=22)
    params = make_params(O.DM_LOGSIGN, seed=42, trained_like=True)
    reps = make_replicas("dm_logsign", params, data, [np.zeros((9, 64), np.int64)] * 2, T, seed=6)
    reps.reset()
    g = reps.graphs[0]
    if g.scale:
        with pytest.raises(ValueError):
            reps.train_step({g.scale[0]: np.ones(g.x[0].shape, np.float32)}, 1e-3)
    other = problems.synthetic_mnist(100, seed=23)
    reps2 = make_replicas("dm_logsign", params, data, [np.zeros((9, 64), np.int64)] * 2, T, seed=6)
    meta.set_random_seed(6)
    extra = reps2.optimizer._build_graph(problems.mnist(layers=(20,), batch_size=64, data=other), T, None, False)
    extra.nets = reps2.graphs[0].nets
    for s in extra.slots:
        s.net = reps2.graphs[0].nets[s.key]
    reps2.graphs.append(extra)                           # a replica over ANOTHER data set
    reps2.reset()
    with pytest.raises(ValueError):
        reps2.train_step({}, 1e-3)
    with pytest.raises(ValueError):
        reps.train_step({}, 1e-3, form="wide")


# ------------------------------------------------------------------------------------------------------------------
# two ranks (gloo), two replicas each
# ------------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _rank_run(rank, T, nsteps):
    from oracle_engine import OracleEngine
    _engine.set_default_engine(OracleEngine())
    name = "rnnprop"
    data = problems.synthetic_mnist(256, seed=24)
    idxs = [np.random.default_rng(60 + 10 * rank + j).integers(0, 256, size=(2 * nsteps * (T + 1), 64)) for j in range(2)]
    params = make_params(ORACLE_CFGS[name], seed=43 + rank, trained_like=True)     # ranks start from DIFFERENT weights
    reps = make_replicas(name, params, data, idxs, T, seed=7 + rank)
    caps = capture_adam(reps)
    reps.reset()
    checks = []
    for i in range(nsteps):
        feed = {reps.step: 1 + i * T}
        singles = None
        if i > 0:                                        # (from step 2 on every rank holds rank 0's weights)
            singles, _, _ = single_gradients(reps, feed)
            out, got = replica_step(reps, feed, 1e-3, caps)
        else:
            out = reps.train_step(feed, 1e-3)
            got = caps[-1]
        assert np.isfinite(out["loss"])
        checks.append((singles, got))
    w = {m: {v: np.asarray(a, np.float32).copy() for v, a in d.items()} for m, d in reps.graphs[0].nets["rp"].variables.items()}
    return w, checks


def _worker(rank, world, port, T, nsteps, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.set_num_threads(2)
        q.put((rank,) + _rank_run(rank, T, nsteps))
    finally:
        dist.destroy_process_group()


def test_two_ranks_two_replicas_each():
    T, nsteps = 3, 3
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, T, nsteps, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(2):
        rank, w, checks = q.get(timeout=600)
        res[rank] = (w, checks)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    # identical weights on both ranks after 3 steps
    for mod, d in res[0][0].items():
        for var, a in d.items():
            np.testing.assert_array_equal(a, res[1][0][mod][var], err_msg="%s/%s" % (mod, var))
    # the applied gradient == the mean of the four replicas' gradients (two per rank), the same on both ranks
    for i in range(1, nsteps):
        four = res[0][1][i][0] + res[1][1][i][0]
        want = mean_of(four)
        for rank in (0, 1):
            check_rel(res[rank][1][i][1], want, REL_MEAN, "step %d, rank %d" % (i, rank))
