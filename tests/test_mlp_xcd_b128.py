"""k_mlp_xcd at the reference's minibatch of 128 (problems.mnist / get_config("mnist") draw batch_size=128, the default
--problem of train_rnnprop.py): eight optimizee instances per launch, one per XCD, in the eight-wave form, plain and
recording, through the existing entry points (l2o_mlp_unroll_multi / _record) and open_l2o_amd.replicas.Replicas:

  * parity of two instances in one launch against the oracle's multi-variable unroll (T = 200, the DM nets);
  * RNNProp instances (8: every XCD; 3: five XCDs exit; 11: two launches) equal to the same instances on the whole-chip
    kernel k_mlp_unroll (its generic loops at this batch), two chained unrolls;
  * the recorded history against the whole-chip recording kernel's generic instantiation;
  * Replicas.train_step at batch 128: the gradient in front of Adam against the float64 mean of the reference meta-gradients;
  * determinism, the drivers, and the four-wave form (which serves batch 64 only) falling back to the whole chip."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle as O
from helpers import ORACLE_CFGS, block_errors, lib_option, make_params, mnist_fg, oracle_meta_grad, rel_err
from open_l2o_amd import _abi, _engine, meta, meta_rnnprop_eval, problems
from open_l2o_amd.replicas import Replicas
from test_meta_api import _net_config
from test_replica_training import _host_hist, _max_rel, _plans
from test_replica_training_cpu import capture_adam, net_key, snapshot
from test_training_gradient import GRAD_TOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 128


@pytest.fixture()
def hip():
    eng = _engine.HipEngine()
    old = _engine._default_engine
    _engine.set_default_engine(eng)
    yield eng
    _engine.set_default_engine(old)


def _sampler(idx):
    calls = {"n": 0}

    def sampler(n_evals, b, n_data):
        out = idx[calls["n"]:calls["n"] + n_evals]
        calls["n"] += n_evals
        return out
    return sampler


def _step0_input_gap(hx, hc):
    """RNNProp's first input is m^ / (sqrt(v^) + 1e-8) = g / (|g| + 1e-8): where a coordinate's gradient is ~1e-8 (five orders
    below the largest), a last-ulp difference of g -- two kernels summing the samples in different orders -- moves that
    input by ~1e-4, and the state after step 0 with it (by ~0.85 of it, then decaying; batch 64 shows the same, smaller:
    128 samples average to more gradients near 1e-8).  The largest such gap over the four variables, from the two
    recorded gradients at x_0."""
    gap = 0.0
    for k in range(4):
        a, b = (np.asarray(h["g"][k][0], np.float64).reshape(-1) for h in (hx, hc))
        gap = max(gap, float(np.abs(a / (np.abs(a) + 1e-8) - b / (np.abs(b) + 1e-8)).max()))
    return gap


def _replicas(cfg, params, data, idxs, T, activation="sigmoid", seed=9):
    meta.set_random_seed(seed)
    probs = [problems.mnist(layers=(20,), activation=activation, batch_size=B, data=data, sampler=_sampler(ix)) for ix in idxs]
    if cfg.kind == "rnnprop":
        opt = meta_rnnprop_eval.MetaOptimizer(0.95, 0.95, **_net_config(cfg, params, key="rp"))
    else:
        opt = meta.MetaOptimizer(**_net_config(cfg, params))
    return Replicas(opt, probs, T)


@pytest.mark.parametrize("netname", ["dm_logsign", "dm"])
def test_batch128_vs_oracle_T200(hip, netname):
    """Minibatch 128, T = 200: TWO instances in one launch (XCDs 0 and 1), each against O.unroll_multi on its own minibatch
    sequence and its own initial weights: the whole loss trajectory and x_T (bounds of the batch-64 test)."""
    data = problems.synthetic_mnist(512, seed=3)
    T = 200
    idxs = [np.random.default_rng(270 + j).integers(0, 512, size=(T + 1, B)) for j in range(2)]
    cfg = O.DM_LOGSIGN if netname == "dm_logsign" else O.DM_IDENTITY
    params = make_params(cfg, seed=71, trained_like=True)
    reps = _replicas(cfg, params, data, idxs, T)
    reps.reset()
    assert reps.xcd_supported()
    v0 = [[v.eval() for v in g.x] for g in reps.graphs]
    fx = reps.run(form="xcd")
    assert reps.last_form == "xcd" and hip.last_unroll_form()[0].startswith("k_mlp_xcd")
    ref = O.MnistMLP(data["images"], data["labels"].astype(np.int32), "sigmoid")
    for j, g in enumerate(reps.graphs):
        states = [O.net_initial_state(cfg, a.size) for a in v0[j]]
        fx_ref, v_ref, _ = O.unroll_multi(lambda vs, t, wg: ref.fg(vs, idxs[j][t], wg), cfg, params, v0[j], states, T)
        e = rel_err(reps.fx_arrays[j], fx_ref)
        print("k_mlp_xcd B=128 %s instance %d T=200 vs oracle: rel fx=%.3g fx0=%.5g fx200=%.5g" % (netname, j, e, fx_ref[0], fx_ref[-1]))
        assert e < 1e-5 and rel_err(fx[j], fx_ref[-1]) < 1e-5
        for got, want in zip([v.eval() for v in g.x], v_ref):
            np.testing.assert_allclose(got, want, rtol=1e-4, atol=2e-6)
    assert not np.allclose(reps.fx_arrays[0], reps.fx_arrays[1])            # (two different instances)


@pytest.mark.parametrize("activation,n", [("sigmoid", 8), ("relu", 3), ("sigmoid", 11)])
def test_rnnprop_batch128_equals_the_whole_chip_kernel(hip, activation, n):
    """RNNProp, n instances through k_mlp_xcd<.., 128> against the same n instances stepped one after the other by
    k_mlp_unroll on the same minibatches; two chained unrolls (step0 = 1 and 1 + T)."""
    data = problems.synthetic_mnist(300, seed=4)
    T = 12
    idxs = [np.random.default_rng(280 + j).integers(0, 300, size=(2 * (T + 1), B)) for j in range(n)]
    cfg = O.RNNPROP
    params = make_params(cfg, seed=81, trained_like=True)
    res = {}
    for form in ("xcd", "chip"):
        reps = _replicas(cfg, params, data, idxs, T, activation=activation, seed=11)
        reps.reset()
        out = []
        for i in range(2):
            fx = reps.run({reps.step: 1 + i * T}, form=form)
            out.append(np.array(reps.fx_arrays, np.float64))
            assert fx.shape == (n,) and np.all(np.isfinite(fx))
        assert reps.last_form == form
        if form == "xcd":
            assert hip.last_unroll_form()[0].startswith("k_mlp_xcd")
        res[form] = (np.array(out), [[v.eval() for v in g.x] for g in reps.graphs])
    np.testing.assert_allclose(res["xcd"][0], res["chip"][0], rtol=2e-5)
    for xa, xb in zip(res["xcd"][1], res["chip"][1]):
        for a, b in zip(xa, xb):
            np.testing.assert_allclose(a, b, rtol=2e-4, atol=2e-6)
    assert not np.allclose(res["xcd"][0][0][0], res["xcd"][0][0][1])       # (different instances)


@pytest.mark.parametrize("name,n", [("rnnprop", 8), ("dm_logsign", 8), ("rnnprop", 3)])
def test_batch128_history_equals_the_whole_chip_record(hip, monkeypatch, name, n):
    """The recording form at batch 128: history buffers pre-filled with NaN, against what the whole-chip recording kernel
    (l2o_mlp_unroll_record, its generic instantiation at this batch) writes for the same instances on the same
    minibatches; slot T (the gradient at x_T) also against the host.  Bound: 2e-4 of each array's largest entry; RNNProp's
    LSTM states from step 1 on: plus the gap of the step-0 inputs the two gradients give (_step0_input_gap), itself < 1e-3."""
    monkeypatch.setenv("L2O_MLP_UNROLL_RECORD_GENERIC", "1")
    T = 20
    data = problems.synthetic_mnist(400, seed=31)
    idxs = [np.random.default_rng(300 + j).integers(0, 400, size=(T + 1, B)) for j in range(n)]
    cfg = ORACLE_CFGS[name]
    params = make_params(cfg, seed=32, trained_like=True)
    feed = (lambda reps: {reps.step: 1}) if cfg.kind == "rnnprop" else (lambda reps: {})
    res = {}
    for form in ("xcd", "chip"):
        reps = _replicas(cfg, params, data, idxs, T, seed=14)
        reps.reset()
        plans = _plans(reps)
        if form == "xcd":
            runs = reps._record_xcd(feed(reps), 1)
            fx = [hip.to_numpy(f) for _, f in runs]
            hip.check_unroll_status()
            assert hip.last_unroll_form()[0].startswith("k_mlp_xcd")
        else:
            fx = []
            for g in reps.graphs:
                out, _ = g.launch(reps._feed(g, feed(reps)), True, record={})
                assert g.last_path == "mlp_unroll"
                fx.append(hip.to_numpy(out))
            hip.check_unroll_status()
        xs = [[v.eval() for v in g.x] for g in reps.graphs]
        res[form] = (np.array(fx, np.float64), [_host_hist(hip, p) for p in plans], xs, reps)
    fx_x, h_x, xs_x, reps = res["xcd"]
    fx_c, h_c, _, _ = res["chip"]
    np.testing.assert_allclose(fx_x, fx_c, rtol=2e-5)
    assert not np.allclose(fx_x[0], fx_x[1])
    mlp = O.MnistMLP(data["images"], data["labels"].astype(np.int32), "sigmoid")
    shapes = [tuple(v.shape) for v in reps.graphs[0].x]
    worst = {}
    for j in range(n):
        hx, hc = h_x[j], h_c[j]
        gap = _step0_input_gap(hx, hc) if "m" in hx else 0.0
        assert gap < 1e-3, ("instance %d: step-0 input gap" % j, gap)
        worst["step-0 input gap"] = max(worst.get("step-0 input gap", 0.0), gap)
        for k in range(4):
            what = "instance %d variable %d" % (j, k)
            assert np.all(np.isfinite(hx["g"][k])), what + ": gradient slot not written"
            e = _max_rel(hx["g"][k], hc["g"][k])
            assert e < 2e-4, (what, "g", e)
            worst["g"] = max(worst.get("g", 0.0), e)
            assert np.all(np.isfinite(hx["st"][k])), what + ": state slot not written"
            for t in range(T):
                e = _max_rel(hx["st"][k][t], hc["st"][k][t])
                assert e < 2e-4 + (gap if t else 0.0), (what, "st", t, e, gap)
                worst["st"] = max(worst.get("st", 0.0), e)
            if "m" in hx:
                for mv in ("m", "v"):
                    e = _max_rel(hx[mv][k][1:], hc[mv][k][1:])
                    assert np.all(np.isfinite(hx[mv][k][1:])) and e < 2e-4, (what, mv, e)
                    worst[mv] = max(worst.get(mv, 0.0), e)
        _, g_T = mlp.fg([np.asarray(a, np.float64).reshape(sh) for a, sh in zip(xs_x[j], shapes)], idxs[j][T])
        for k in range(4):
            e = _max_rel(hx["g"][k][T].reshape(-1), g_T[k].reshape(-1))
            assert e < 2e-4, ("instance %d slot T" % j, k, e)
            worst["g_T vs host"] = max(worst.get("g_T vs host", 0.0), e)
    print("B=128 %s x %d: worst error of each array's largest entry, xcd vs chip: %s" % (
        name, n, ", ".join("%s %.2g" % kv for kv in sorted(worst.items()))))


def test_batch128_train_steps_vs_float64(hip):
    """Eight RNNProp replicas at minibatch 128, T = 20: two consecutive train steps (the second from carried state) on the
    recording k_mlp_xcd; each step's gradient in front of Adam against the float64 mean of the eight reference
    meta-gradients, on the rows each replica consumed."""
    T, n, name = 20, 8, "rnnprop"
    cfg = ORACLE_CFGS[name]
    data = problems.synthetic_mnist(1024, seed=33)
    mlp = O.MnistMLP(data["images"], data["labels"].astype(np.int32), "sigmoid")
    params = make_params(cfg, seed=34, trained_like=True)
    meta.set_random_seed(15)
    probs = [problems.mnist(layers=(20,), batch_size=B, data=data) for _ in range(n)]    # minibatches drawn on the device
    reps = Replicas(meta_rnnprop_eval.MetaOptimizer(0.95, 0.95, **_net_config(cfg, params, key="rp")), probs, T)
    assert reps.xcd_supported()
    caps = capture_adam(reps)
    key = net_key(reps)
    shapes = [tuple(v.shape) for v in reps.graphs[0].x]
    reps.reset()
    for i in range(2):
        step0 = 1 + i * T
        snaps = [snapshot(hip, g, key, step0) for g in reps.graphs]
        if i:
            assert any(np.abs(s["state"][0][0]).max() > 0 for s in snaps)
        out = reps.train_step({reps.step: step0}, 1e-3)
        assert reps.last_form == "xcd" and hip.last_unroll_form()[0].startswith("k_mlp_xcd")
        assert np.isfinite(out["loss"]) and out["fx"].shape == (n,)
        got = caps[-1]
        want, want32 = {}, {}
        for g, snap in zip(reps.graphs, snaps):
            rows = hip.to_numpy(g._mlp_idx[0])
            assert rows.shape == (T + 1, B)
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
        print("B=128, 8 replicas, step %d: worst block error %.3g" % (i, max(errs.values())))


def test_batch128_launches_are_deterministic(hip):
    """Two launches of eight RNNProp instances on identical inputs (weights, minibatches, step) give bit-identical losses
    and x_T: every sum in the kernel runs in a fixed order."""
    data = problems.synthetic_mnist(300, seed=8)
    T, n = 20, 8
    idxs = [np.random.default_rng(320 + j).integers(0, 300, size=(T + 1, B)) for j in range(n)]
    cfg = O.RNNPROP
    params = make_params(cfg, seed=83, trained_like=True)
    outs = []
    for _ in range(2):
        reps = _replicas(cfg, params, data, idxs, T, seed=21)
        reps.reset()
        reps.run({reps.step: 1}, form="xcd")
        assert reps.last_form == "xcd"
        outs.append((np.array(reps.fx_arrays), [[v.eval() for v in g.x] for g in reps.graphs]))
    np.testing.assert_array_equal(outs[0][0], outs[1][0])
    for xa, xb in zip(outs[0][1], outs[1][1]):
        for a, b in zip(xa, xb):
            np.testing.assert_array_equal(a, b)


def test_four_wave_form_has_no_batch128(hip):
    """L2O_OPT_MLP_XCD_WAVES = 2 forces the four-wave form, which has no batch-128 instantiation: the support predicate
    says no, form="xcd" raises, and form="auto" runs on the whole chip."""
    data = problems.synthetic_mnist(256, seed=9)
    T, n = 4, 3
    idxs = [np.random.default_rng(330 + j).integers(0, 256, size=(T + 1, B)) for j in range(n)]
    params = make_params(O.RNNPROP, seed=84, trained_like=True)
    with lib_option(_abi.OPT_MLP_XCD_WAVES, 2):
        reps = _replicas(O.RNNPROP, params, data, idxs, T, seed=22)
        reps.reset()
        assert not reps.xcd_supported()
        with pytest.raises(_abi.L2OUnsupported):
            reps.run({reps.step: 1}, form="xcd")
        fx = reps.run({reps.step: 1})
        assert reps.last_form == "chip" and fx.shape == (n,) and np.all(np.isfinite(fx))
    reps = _replicas(O.RNNPROP, params, data, idxs, T, seed=22)
    assert reps.xcd_supported()                                              # (the default: eight waves)


def _run_driver(cmd, seconds):
    r = subprocess.run(["timeout", "-k", "10", str(seconds)] + cmd, capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_train_rnnprop_driver_default_batch_is_xcd(tmp_path):
    """train_rnnprop.py --problem mnist --replicas 8 with the reference's minibatch (no --batch_size: 128)."""
    out = _run_driver([sys.executable, os.path.join(ROOT, "scripts", "train_rnnprop.py"), "--problem", "mnist", "--replicas", "8",
                       "--synthetic_mnist", "512", "--num_epochs", "2", "--evaluation_period", "1",
                       "--evaluation_epochs", "1", "--num_steps", "40", "--unroll_length", "20", "--seed", "3",
                       "--save_path", str(tmp_path / "out")], 300)
    assert "replicas=8, form=xcd" in out, out[-2000:]
    losses = [float(l.split("=")[1]) for l in out.splitlines() if l.startswith("training_loss=")]
    assert len(losses) == 2 and all(np.isfinite(losses)), out[-2000:]


def test_evaluate_rnnprop_driver_batch128_is_xcd(tmp_path):
    out = _run_driver([sys.executable, os.path.join(ROOT, "scripts", "evaluate_rnnprop.py"), "--problem", "mnist",
                       "--synthetic_mnist", "512", "--replicas", "8", "--batch_size", "128", "--num_steps", "40",
                       "--unroll_len", "20", "--seed", "4", "--output_path", str(tmp_path / "eval")], 300)
    assert "kernel form: xcd" in out, out[-2000:]
    import pickle
    path = tmp_path / "eval" / "L2L_eval_loss_record.pickle-mnist"
    with open(str(path), "rb") as f:
        records = pickle.load(f)
    assert len(records) == 8 and all(len(r) == 2 and np.all(np.isfinite(r)) for r in records)
    assert len({tuple(r) for r in records}) == 8                             # (eight distinct instances)
