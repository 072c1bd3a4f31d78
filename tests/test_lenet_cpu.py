"""problems.LeNet (DM/problems.py:461-537, util.get_config("lenet")) without a GPU: the variables the factory declares, the
unsupported shapes and the missing-data error, the float64 reference's own correctness (central differences), the
library's new symbols, and the host wiring -- meta_loss / meta_minimize over the net on an oracle engine whose lenet_fg is
the float32 torch reference (lenet_reference.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import lenet_reference as R
import oracle as O
from helpers import make_params, rel_err, spec_of
from oracle_engine import OracleEngine
from open_l2o_amd import _abi, _engine, meta, meta_rnnprop_eval, problems, util
from open_l2o_amd.session import Session
from test_meta_api import _net_config


class LenetOracleEngine(OracleEngine):
    """The oracle engine plus LeNet's loss and gradient from the float32 torch reference."""

    def lenet_fg(self, d, indices, ws, loss, grads):
        self.calls.append("lenet_fg")
        net = R.LeNet(d.images.numpy(), d.labels.numpy(), d.batch_norm)
        vs = [w.numpy().reshape(sh) for w, sh in zip(ws, R.shapes(d.batch_norm))]
        f, g = net.fg(vs, indices.numpy(), want_grad=grads is not None)
        loss.copy_(torch.from_numpy(np.array([f], np.float32)))
        if grads is not None:
            for t, a in zip(grads, g):
                t.copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32)).view_as(t))


@pytest.fixture
def engine():
    eng = LenetOracleEngine()
    old = _engine._default_engine
    _engine.set_default_engine(eng)
    yield eng
    _engine.set_default_engine(old)


def _data(n=64, seed=0):
    return problems.synthetic_cifar10(n, seed=seed)


def _lenet(**kw):
    kw.setdefault("conv_channels", (6, 16))
    kw.setdefault("linear_layers", (120, 84))
    return problems.LeNet("cifar10", **kw)


# 1. the factory
@pytest.mark.parametrize("batch_norm", [True, False])
def test_variables_names_shapes_order(batch_norm):
    loss = _lenet(batch_norm=batch_norm, data=_data())()
    assert [v.name for v in loss.variables] == R.names(batch_norm)
    assert [v.shape for v in loss.variables] == R.shapes(batch_norm)
    assert len(loss.variables) == (14 if batch_norm else 10)
    assert all(v.trainable for v in loss.variables)
    assert sum(int(np.prod(v.shape)) for v in loss.variables) == (62232 if batch_norm else 62006)
    (term,) = loss.terms
    assert term.kind == _abi.PROB_LENET == 8 and term.hyper["batch_size"] == 128
    assert term.hyper["batch_norm"] is batch_norm and term.hyper["images"].shape == (64, 3072)
    for v in loss.variables:                       # every w AND b from N(0, 0.01^2), every beta zero
        assert v.initializer == (("zeros",) if v.name.endswith("beta") else ("normal", 0.0, 0.01)), v.name
    if batch_norm:
        assert [v.name for v in loss.variables][:3] == ["conv_net_2d/conv_2d_0/w", "conv_net_2d/conv_2d_0/b",
                                                        "conv_net_2d/batch_norm_0/beta"]
        assert loss.variables[8].name == "mlp/batch_norm/beta" and loss.variables[11].name == "mlp/batch_norm_1/beta"
        assert loss.variables[6].shape == (400, 120) and loss.variables[13].shape == (10,)


def test_unsupported_shapes_and_batches():
    for kw in ({"conv_channels": None, "linear_layers": None}, {"conv_channels": (6, 8)}, {"linear_layers": (120,)},
               {"conv_channels": (6, 16, 32)}, {"linear_layers": (100, 84)}):
        with pytest.raises(NotImplementedError, match=r"\(6, 16\).*\(120, 84\)"):
            _lenet(data=_data(), **kw)
    with pytest.raises(NotImplementedError):
        problems.LeNet("cifar10", data=_data())          # the reference's None defaults
    for batch in (1, 1025):
        with pytest.raises(NotImplementedError):
            _lenet(batch_size=batch, data=_data())
    _lenet(batch_size=2, data=_data())
    _lenet(conv_channels=[6, 16], linear_layers=[120, 84], batch_size=1024, data=_data())


def test_missing_data_error(tmp_path, monkeypatch):
    monkeypatch.delenv("L2O_CIFAR10_DIR", raising=False)
    monkeypatch.chdir(tmp_path)
    for make in (lambda: util.get_config("lenet"), lambda: _lenet()):
        with pytest.raises(FileNotFoundError) as ei:
            make()
        assert isinstance(ei.value, NotImplementedError) and isinstance(ei.value, problems.Cifar10DataMissing)
        assert "L2O_CIFAR10_DIR" in str(ei.value)


# 2. util.get_config
def test_get_config():
    problem, net_config, na = util.get_config("lenet", problem_options={"data": _data()})
    loss = problem()
    assert [v.name for v in loss.variables] == R.names(True) and loss.terms[0].hyper["batch_size"] == 128
    assert loss.terms[0].kind == _abi.PROB_LENET
    assert net_config["cw"]["net_options"]["preprocess_name"] == "LogAndSign" and na is None
    problem, net_config, _ = util.get_config("lenet", net_name="RNNprop",
                                             problem_options={"data": _data(), "batch_size": 16, "batch_norm": False})
    assert "rp" in net_config and problem().terms[0].hyper["batch_size"] == 16
    assert [v.name for v in problem().variables] == R.names(False)


# 3. the float64 reference itself
@pytest.mark.parametrize("batch_norm", [True, False])
def test_reference_central_differences(batch_norm):
    """The float64 reference's gradient against central differences on a handful of coordinates of every variable; the
    biases that feed a batch norm have gradient 0."""
    d = _data(64, seed=3)
    rng = np.random.default_rng(4)
    images = d["images"].reshape(64, -1) + 0.05 * rng.random((64, 3072))
    net = R.LeNet(images, d["labels"], batch_norm)
    w = [a.astype(np.float64) for a in R.sample_weights(batch_norm, 5)]
    rows = rng.integers(0, 64, 12)
    f, g = net.fg(w, rows)
    assert np.isfinite(f) and (net.last_logits > 0).any() and (net.last_logits < 0).any()
    assert R.pool_ties(net.last_pre_pool) == 0 and R.pool_ties(net.last_pool_inputs) == 0
    h = 1e-6
    for k, a in enumerate(w):
        for j in rng.choice(a.size, size=min(4, a.size), replace=False):
            wp = [b.copy() for b in w]
            wm = [b.copy() for b in w]
            wp[k].reshape(-1)[j] += h
            wm[k].reshape(-1)[j] -= h
            num = (net.fg(wp, rows, want_grad=False)[0] - net.fg(wm, rows, want_grad=False)[0]) / (2 * h)
            scale = max(np.abs(g[k]).max(), 1e-3)
            assert abs(num - g[k].reshape(-1)[j]) < 1e-6 * scale + 1e-8, (R.names(batch_norm)[k], j, num, g[k].reshape(-1)[j])
    assert len(R.bn_fed_biases(batch_norm)) == (4 if batch_norm else 0)
    for kb, kw in R.bn_fed_biases(batch_norm):
        assert R.names(batch_norm)[kb].endswith("/b") and R.names(batch_norm)[kw].endswith("/w")
        assert np.abs(g[kb]).max() < 1e-12 * np.abs(g[kw]).max(), R.names(batch_norm)[kb]


def test_reference_pools_like_the_kernel():
    """max-pool(sigmoid(x)) == sigmoid(max-pool(x)) with the same argmax: the order the kernels and lenet_reference.py use
    is the reference's net."""
    d = _data(32, seed=5)
    net = R.LeNet(d["images"], d["labels"], True)
    w = [a.astype(np.float64) for a in R.sample_weights(True, 6)]
    net.fg(w, np.arange(16), want_grad=False)
    pool = torch.nn.functional.max_pool2d
    for pre, post in zip(net.last_pre_pool, net.last_pool_inputs):
        a, ia = pool(torch.tensor(pre), 2, 2, return_indices=True)
        b, ib = pool(torch.tensor(post), 2, 2, return_indices=True)
        assert torch.equal(torch.sigmoid(a), b) and torch.equal(ia, ib)


# 4. the library
def test_library_symbols_and_unroll_support():
    import __graft_entry__  # noqa: F401
    lib = _abi.lib()
    for name in ("l2o_lenet_fg", "l2o_lenet_scratch_floats"):
        assert name in _abi.SYMBOLS
        getattr(lib, name)
    assert lib.l2o_abi_version() == 15
    cc = spec_of(O.DM_LOGSIGN).to_c()
    p = _abi.Problem()
    p.kind, p.B_local, p.B_global, p.D, p.M = _abi.PROB_LENET, 1, 1, 62232, 62232
    assert lib.l2o_unroll_supported(C.byref(cc), C.byref(p)) == 0
    assert lib.l2o_unroll_record_supported(C.byref(cc), C.byref(p)) == 0
    m = _abi.Lenet()
    m.n_data, m.batch_norm = 100, 1
    for batch, ok in ((1, False), (2, True), (128, True), (1024, True), (1025, False)):
        m.batch = batch
        assert (lib.l2o_lenet_scratch_floats(C.byref(m)) > 0) == ok, batch
    m.batch = 128
    assert lib.l2o_lenet_fg(C.byref(m), None, None, None, None, None, None) == _abi.L2O_ERR_ARG
    m.batch = 1
    assert lib.l2o_lenet_fg(C.byref(m), None, None, None, None, None, None) == _abi.L2O_ERR_UNSUPPORTED
    m.batch = 1025
    assert lib.l2o_lenet_fg(C.byref(m), None, None, None, None, None, None) == _abi.L2O_ERR_UNSUPPORTED


# 5. host wiring
def _sampler(idx):
    calls = {"n": 0}

    def sampler(n_evals, b, n_data):
        out = idx[calls["n"]:calls["n"] + n_evals]
        calls["n"] += n_evals
        return out
    return sampler


@pytest.mark.parametrize("net", ["dm_logsign", "rnnprop"])
def test_meta_loss_wiring(engine, net):
    """meta_loss over util.get_config("lenet") on the step-granular path == the oracle's multi-variable unroll over the same
    float32 evaluations, two chained unrolls."""
    data = _data(96, seed=7)
    T, batch = 3, 8
    idx = np.random.default_rng(8).integers(0, 96, size=(2 * (T + 1), batch))
    cfg = O.DM_LOGSIGN if net == "dm_logsign" else O.RNNPROP
    params = make_params(cfg, seed=9, trained_like=True)
    meta.set_random_seed(10)
    problem = util.get_config("lenet", problem_options={"data": data, "batch_size": batch, "sampler": _sampler(idx)})[0]
    feeds = [{}, {}]
    if cfg.kind == "rnnprop":
        optimizer = meta_rnnprop_eval.MetaOptimizer(0.95, 0.95, **_net_config(cfg, params, key="rp"))
        ml, _, _, step = optimizer.meta_loss(problem, T)
        feeds = [{step: 1}, {step: 1 + T}]
    else:
        optimizer = meta.MetaOptimizer(**_net_config(cfg, params))
        ml = optimizer.meta_loss(problem, T)
    with Session() as sess:
        sess.run(ml.reset)
        v0 = [v.eval() for v in optimizer.graph.x]
        assert [a.shape for a in v0] == R.shapes(True)
        loss1, fx1, _ = sess.run([ml.loss, ml.fx, ml.update], feed_dict=feeds[0])
        loss2, fx2, x2, _ = sess.run([ml.loss, ml.fx, ml.x, ml.update], feed_dict=feeds[1])
    assert optimizer.graph.last_path == "steps"
    assert engine.calls.count("lenet_fg") == 2 * (T + 1)
    ref = R.LeNet(data["images"], data["labels"], True)
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


def test_meta_minimize_and_refusals(engine):
    """One first-order training step on LeNet runs on the recording step path; second derivatives and the replicas' training
    step refuse it."""
    data = _data(64, seed=11)
    meta.set_random_seed(12)
    opt = meta.MetaOptimizer(**_net_config(O.DM_LOGSIGN, make_params(O.DM_LOGSIGN, seed=13, trained_like=True)))
    problem = _lenet(batch_size=8, data=data)
    ms = opt.meta_minimize(problem, 2, learning_rate=1e-3)
    w0 = {m: {v: np.array(a) for v, a in d.items()} for m, d in opt._nets["cw"].variables.items()}
    with Session() as sess:
        sess.run(ms.reset)
        c1 = sess.run([ms.fx, ms.update, ms.step])[0]
    assert np.isfinite(c1) and opt.graph.last_path == "steps"
    assert "lenet_fg" in engine.calls
    w1 = opt._nets["cw"].variables
    assert any(not np.array_equal(w0[m][v], np.asarray(w1[m][v])) for m in w0 for v in w0[m])
    opt2 = meta.MetaOptimizer(**_net_config(O.DM_LOGSIGN, make_params(O.DM_LOGSIGN, seed=13, trained_like=True)))
    with pytest.raises(NotImplementedError, match=r"second_derivatives.*problems\.LeNet"):
        opt2.meta_minimize(problem, 2, learning_rate=1e-3, second_derivatives=True)
    from open_l2o_amd.replicas import Replicas
    reps = Replicas(opt, [problem, problem], 2)
    with pytest.raises(ValueError, match="problems.mnist"):
        reps.train_step({}, 1e-3)


def test_replicas_run_one_at_a_time(engine):
    """Replicas.run over LeNet instances: no multi-instance kernel applies, so they run one after the other ("chip")."""
    from open_l2o_amd.replicas import Replicas
    meta.set_random_seed(14)
    opt = meta.MetaOptimizer(**_net_config(O.DM_LOGSIGN, make_params(O.DM_LOGSIGN, seed=15, trained_like=True)))
    problem = _lenet(batch_size=4, data=_data(32, seed=16))
    reps = Replicas(opt, [problem, problem], 2)
    reps.reset()
    fx = reps.run({})
    assert reps.last_form == "chip" and fx.shape == (2,) and np.isfinite(fx).all()
    assert engine.calls.count("lenet_fg") >= 2 * 3
