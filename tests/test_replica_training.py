"""Meta-training on MNIST replicas with the recording one-instance-per-XCD kernel (l2o_mlp_unroll_multi_record /
k_mlp_xcd<PRE, WV, true>), both wave forms:

  * the history it writes for n instances (8: every XCD; 3: five XCDs exit; 11: two launches) against what
    l2o_mlp_unroll_record writes for the same instances on the same minibatches, one after the other on the whole chip:
    gradients (slot T included, also against the host's gradient at x_T), moments, LSTM states.  The history buffers
    are filled with NaN first, so a slot the kernel does not write fails.  Bound: 2e-4 of each array's largest entry (the
    two kernels sum the hidden pre-activations in different orders; measured worst: the LSTM state, 1.3e-4, at the
    first step of an RNNProp instance, where m / sqrt(v) = g / |g|);
  * Replicas.train_step at BASELINE config 5's shape (RNNProp, 8 replicas, minibatch 64, T = 20), two consecutive steps
    from carried state: the gradient handed to Adam against the float64 mean of the eight reference meta-gradients, on
    the rows each replica consumed (read back from its _mlp_idx); four fused BPTT launches of two replicas each;
  * a forced partner timeout of the recording kernel: no update, the Adam step count taken back, L2OPartnerTimeout;
  * scripts/train_rnnprop.py --replicas 8 end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle as O
from helpers import ORACLE_CFGS, block_errors, lib_option, make_params, mnist_fg, oracle_meta_grad
from open_l2o_amd import _abi, _engine
from open_l2o_amd import problems
from test_replica_training_cpu import capture_adam, make_replicas, net_key, snapshot
from test_training_gradient import GRAD_TOL, spy_bwd_unroll

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def hip():
    eng = _engine.HipEngine()
    old = _engine._default_engine
    _engine.set_default_engine(eng)
    yield eng
    _engine.set_default_engine(old)


@pytest.fixture(params=[1, 2], ids=["eight_waves", "four_waves_tile_pairs"])
def waves(request):
    """L2O_OPT_MLP_XCD_WAVES: both forms of k_mlp_xcd run every kernel test of this file."""
    with lib_option(_abi.OPT_MLP_XCD_WAVES, request.param):
        yield request.param


def _feed(reps, step0):
    return {reps.step: step0} if reps.graphs[0].rnnprop else {}


def _plans(reps):
    """Every replica's record plan (the buffers the recording launch writes), created ahead and filled with NaN."""
    out = []
    for g in reps.graphs:
        g._ensure_init()
        slots = g.slots
        panels = [v.value.view(*g._panel_shape(v)) for v in g.x]
        plan = g._mlp_hist_plan(reps.len_unroll, panels, slots, [s.state for s in slots], [s.m for s in slots],
                                  [s.v for s in slots])
        for k in ("st", "g", "m", "v"):
            for t in plan["hist"][k] or ():
                t.fill_(float("nan"))
        out.append(plan)
    return out


def _host_hist(eng, plan):
    return {k: [eng.to_numpy(t) for t in plan["hist"][k]] for k in ("st", "g", "m", "v") if plan["hist"][k] is not None}


def _max_rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max()) / max(float(np.abs(b).max()), 1e-30)


@pytest.mark.parametrize("name,n", [("rnnprop", 8), ("dm_logsign", 8), ("dm", 8), ("rnnprop", 3), ("rnnprop", 11)])
def test_history_equals_the_whole_chip_record(hip, waves, name, n):
    T = 20
    data = problems.synthetic_mnist(400, seed=31)
    idxs = [np.random.default_rng(100 + j).integers(0, 400, size=(T + 1, 64)) for j in range(n)]
    params = make_params(ORACLE_CFGS[name], seed=32, trained_like=True)
    res = {}
    for form in ("xcd", "chip"):
        reps = make_replicas(name, params, data, idxs, T, seed=14)
        reps.reset()
        plans = _plans(reps)
        if form == "xcd":
            runs = reps._record_xcd(_feed(reps, 1), 1)
            fx = [hip.to_numpy(f) for _, f in runs]
            hip.check_unroll_status()
            assert hip.last_unroll_form()[0].startswith("k_mlp_xcd")
        else:
            fx = []
            for g in reps.graphs:
                out, _ = g.launch(reps._feed(g, _feed(reps, 1)), True, record={})
                assert g.last_path == "mlp_unroll"
                fx.append(hip.to_numpy(out))
            hip.check_unroll_status()
        xs = [[v.eval() for v in g.x] for g in reps.graphs]
        res[form] = (np.array(fx, np.float64), [_host_hist(hip, p) for p in plans], xs, reps)
    fx_x, h_x, xs_x, reps = res["xcd"]
    fx_c, h_c, xs_c, _ = res["chip"]
    np.testing.assert_allclose(fx_x, fx_c, rtol=2e-5)
    assert not np.allclose(fx_x[0], fx_x[1])                                   # (different instances)
    mlp = O.MnistMLP(data["images"], data["labels"].astype(np.int32), "sigmoid")
    shapes = [tuple(v.shape) for v in reps.graphs[0].x]
    worst = {}
    for j in range(n):
        hx, hc = h_x[j], h_c[j]
        for k in range(4):                                                     # w1, b1, w2, b2
            what = "instance %d variable %d" % (j, k)
            assert np.all(np.isfinite(hx["g"][k])), what + ": gradient slot not written"
            e = _max_rel(hx["g"][k], hc["g"][k])
            assert e < 2e-4, (what, "g", e)
            worst["g"] = max(worst.get("g", 0.0), e)
            assert np.all(np.isfinite(hx["st"][k])), what + ": state slot not written"
            for t in range(T):                                                 # the state BEFORE step t
                e = _max_rel(hx["st"][k][t], hc["st"][k][t])
                assert e < 2e-4, (what, "st", t, e)
                worst["st"] = max(worst.get("st", 0.0), e)
            if "m" in hx:                                                      # slots 1..T: the moments after step t - 1
                for mv in ("m", "v"):
                    e = _max_rel(hx[mv][k][1:], hc[mv][k][1:])
                    assert np.all(np.isfinite(hx[mv][k][1:])) and e < 2e-4, (what, mv, e)
                    worst[mv] = max(worst.get(mv, 0.0), e)
        # slot T: the gradient at x_T, on minibatch row T (independently, on the host)
        _, g_T = mlp.fg([np.asarray(a, np.float64).reshape(sh) for a, sh in zip(xs_x[j], shapes)], idxs[j][T])
        for k in range(4):
            e = _max_rel(hx["g"][k][T].reshape(-1), g_T[k].reshape(-1))
            assert e < 2e-4, ("instance %d slot T" % j, k, e)
            worst["g_T vs host"] = max(worst.get("g_T vs host", 0.0), e)
    print("%s x %d: worst error of each array's largest entry, xcd vs chip: %s" % (
        name, n, ", ".join("%s %.2g" % kv for kv in sorted(worst.items()))))


def test_config5_train_steps_vs_float64(hip, waves, monkeypatch):
    """Eight RNNProp replicas at minibatch 64, T = 20: two consecutive train steps (the second from carried state);
    each step's gradient in front of Adam against the float64 mean of the eight replicas' reference meta-gradients."""
    T, n, name = 20, 8, "rnnprop"
    cfg = ORACLE_CFGS[name]
    data = problems.synthetic_mnist(1024, seed=33)
    mlp = O.MnistMLP(data["images"], data["labels"].astype(np.int32), "sigmoid")
    params = make_params(cfg, seed=34, trained_like=True)
    from open_l2o_amd import meta, meta_rnnprop_eval
    from open_l2o_amd.replicas import Replicas
    from test_meta_api import _net_config
    meta.set_random_seed(15)
    probs = [problems.mnist(layers=(20,), batch_size=64, data=data) for _ in range(n)]    # minibatches drawn on the device
    reps = Replicas(meta_rnnprop_eval.MetaOptimizer(0.95, 0.95, **_net_config(cfg, params, key="rp")), probs, T)
    caps = capture_adam(reps)
    launches = spy_bwd_unroll(hip, monkeypatch)
    key = net_key(reps)
    shapes = [tuple(v.shape) for v in reps.graphs[0].x]
    reps.reset()
    for i in range(2):
        step0 = 1 + i * T
        snaps = [snapshot(hip, g, key, step0) for g in reps.graphs]
        if i:
            assert any(np.abs(s["state"][0][0]).max() > 0 for s in snaps)      # a carried, non-zero start
        del launches[:]
        out = reps.train_step({reps.step: step0}, 1e-3)
        assert reps.last_form == "xcd" and hip.last_unroll_form()[0].startswith("k_mlp_xcd")
        assert len(launches) == 4 and all(len(p) == 8 for p in launches), launches
        assert np.isfinite(out["loss"]) and out["fx"].shape == (n,)
        got = caps[-1]
        want, want32 = {}, {}
        for g, snap in zip(reps.graphs, snaps):
            rows = hip.to_numpy(g._mlp_idx[0])
            assert rows.shape == (T + 1, 64)
            fg = mnist_fg(mlp, shapes, rows)
            st = tuple((h, c) for h, c in snap["state"])
            g64, _ = oracle_meta_grad(cfg, snap["w"], fg, snap["x"], st, T, m0=snap["m"], v0=snap["v"], step0=step0)
            for mod, d in g64.items():
                for var, a in d.items():
                    want.setdefault(mod, {}).setdefault(var, []).append(a / n)
        want = {mod: {var: np.sum(a, axis=0) for var, a in d.items()} for mod, d in want.items()}
        errs = block_errors(got, want)
        bad = {k: e for k, e in errs.items() if e >= GRAD_TOL}
        if bad:                                                                # only then: the float32 oracle's own distance
            for g, snap in zip(reps.graphs, snaps):
                fg = mnist_fg(mlp, shapes, hip.to_numpy(g._mlp_idx[0]))
                w32 = {m: {v: a.astype(np.float32) for v, a in d.items()} for m, d in snap["w"].items()}
                st32 = tuple((h.astype(np.float32), c.astype(np.float32)) for h, c in snap["state"])
                g32, _ = oracle_meta_grad(cfg, w32, fg, snap["x"].astype(np.float32), st32, T, m0=snap["m"].astype(np.float32),
                                          v0=snap["v"].astype(np.float32), step0=step0)
                for mod, d in g32.items():
                    for var, a in d.items():
                        want32.setdefault(mod, {}).setdefault(var, []).append(a.astype(np.float64) / n)
            want32 = {mod: {var: np.sum(a, axis=0) for var, a in d.items()} for mod, d in want32.items()}
            errs32 = block_errors(want32, want)
            for k, e in bad.items():
                assert e < 3 * errs32[k], ("step %d" % i, k, e, errs32[k])
        print("config 5, 8 replicas, step %d: worst block error %.3g" % (i, max(errs.values())))


def test_timeout_skips_the_update_and_raises(hip, waves):
    T, n = 8, 4
    data = problems.synthetic_mnist(256, seed=35)
    idxs = [np.random.default_rng(110 + j).integers(0, 256, size=(3 * (T + 1), 64)) for j in range(n)]
    params = make_params(O.RNNPROP, seed=36, trained_like=True)
    reps = make_replicas("rnnprop", params, data, idxs, T, seed=16)
    reps.reset()
    reps.train_step({reps.step: 1}, 1e-3)                                      # (allocates the workspace)
    assert reps.last_form == "xcd"
    g0 = reps.graphs[0]
    before = reps.optimizer.save()
    t_before = g0._adam["t"]
    hip.inject_unroll_fault()
    with pytest.raises(_abi.L2OPartnerTimeout):
        reps.train_step({reps.step: 1 + T}, 1e-3)
    after = reps.optimizer.save()
    assert g0._adam["t"] == t_before
    for net in before:
        for mod in before[net]:
            for var in before[net][mod]:
                np.testing.assert_array_equal(np.asarray(after[net][mod][var]), np.asarray(before[net][mod][var]))
    reps.reset()                                                               # (the failed unroll's iterates are garbage)
    out = reps.train_step({reps.step: 1}, 1e-3)                                # the status word was cleared: steps go on
    assert np.isfinite(out["loss"]) and g0._adam["t"] == t_before + 1


def test_train_rnnprop_driver_with_replicas(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "train_rnnprop.py"), "--problem", "mnist", "--replicas", "8",
           "--synthetic_mnist", "512", "--batch_size", "64", "--num_epochs", "2", "--evaluation_period", "1",
           "--evaluation_epochs", "1", "--num_steps", "40", "--unroll_length", "20", "--seed", "3",
           "--save_path", str(tmp_path / "out")]
    r = subprocess.run(["timeout", "-k", "10", "240"] + cmd, capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "replicas=8, form=xcd" in r.stdout, r.stdout[-2000:]
    losses = [float(l.split("=")[1]) for l in r.stdout.splitlines() if l.startswith("training_loss=")]
    assert len(losses) == 2 and all(np.isfinite(losses)), r.stdout[-2000:]
    assert os.path.exists(str(tmp_path / "out" / "rp.l2l-0"))
