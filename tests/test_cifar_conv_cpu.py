"""problems.cifar10 (DM/problems.py:369-458, util.get_config("cifar_conv")) without a GPU: the variables the factory
declares, the binary-file loader and the missing-data error, the float64 reference's own correctness (central
differences), the library's new symbols, and the host wiring -- meta_loss / meta_minimize over the conv net on an oracle
engine whose cifar_conv_fg is the float32 torch reference (cifar_conv_reference.py)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cifar_conv_reference as R
import oracle as O
from helpers import make_params, rel_err, spec_of
from oracle_engine import OracleEngine
from open_l2o_amd import _abi, _engine, meta, meta_rnnprop_eval, problems, util
from open_l2o_amd.session import Session
from test_meta_api import _net_config


class CifarOracleEngine(OracleEngine):
    """The oracle engine plus the CIFAR-10 conv net's loss and gradient from the float32 torch reference."""

    def cifar_conv_fg(self, d, indices, ws, loss, grads):
        self.calls.append("cifar_conv_fg")
        net = R.ConvNet(d.images.numpy(), d.labels.numpy(), d.batch_norm)
        vs = [w.numpy().reshape(sh) for w, sh in zip(ws, R.shapes(d.batch_norm))]
        f, g = net.fg(vs, indices.numpy(), want_grad=grads is not None)
        loss.copy_(torch.from_numpy(np.array([f], np.float32)))
        if grads is not None:
            for t, a in zip(grads, g):
                t.copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32)).view_as(t))


@pytest.fixture
def engine():
    eng = CifarOracleEngine()
    old = _engine._default_engine
    _engine.set_default_engine(eng)
    yield eng
    _engine.set_default_engine(old)


def _data(n=64, seed=0):
    return problems.synthetic_cifar10(n, seed=seed)


@pytest.mark.parametrize("batch_norm", [True, False])
def test_variables_names_shapes_order(batch_norm):
    loss = problems.cifar10("cifar10", batch_norm=batch_norm, data=_data())()
    assert [v.name for v in loss.variables] == R.names(batch_norm)
    assert [v.shape for v in loss.variables] == R.shapes(batch_norm)
    assert all(v.trainable for v in loss.variables)
    assert sum(int(np.prod(v.shape)) for v in loss.variables) == (13706 if batch_norm else 13610)
    (term,) = loss.terms
    assert term.kind == _abi.PROB_CIFAR_CONV == 7 and term.hyper["batch_size"] == 128
    assert term.hyper["images"].shape == (64, 3072)
    inits = [v.initializer for v in loss.variables]
    k2 = 4 if batch_norm else 2
    assert inits[0] == inits[k2] == inits[-2] == ("normal", 0.0, 0.01)
    assert inits[1] == inits[k2 + 1] == inits[-1] == ("zeros",)
    if batch_norm:
        assert inits[2] == inits[6] == ("ones",) and inits[3] == inits[7] == ("zeros",)


def test_synthetic_cifar10():
    a, b = problems.synthetic_cifar10(200, seed=3), problems.synthetic_cifar10(200, seed=3)
    assert a["images"].shape == (200, 32, 32, 3) and a["images"].dtype == np.float32 and a["labels"].shape == (200,)
    assert np.array_equal(a["images"], b["images"]) and np.array_equal(a["labels"], b["labels"])
    assert a["images"].min() >= 0.0 and a["images"].max() <= 1.0 and set(a["labels"]) <= set(range(10))
    # class-separable: every image is nearer its own class mean than any other
    x = a["images"].reshape(200, -1)
    means = np.stack([x[a["labels"] == c].mean(0) for c in range(10)])
    d = ((x[:, None, :] - means[None]) ** 2).sum(-1)
    assert (d.argmin(1) == a["labels"]).all()
    noisy = problems.synthetic_cifar10(200, seed=3, label_noise=0.5)
    assert np.array_equal(noisy["images"], a["images"]) and not np.array_equal(noisy["labels"], a["labels"])


def test_get_config():
    problem, net_config, na = util.get_config("cifar_conv", problem_options={"data": _data()})
    loss = problem()
    assert [v.name for v in loss.variables] == R.names(True) and loss.terms[0].hyper["batch_size"] == 128
    assert net_config["cw"]["net_options"]["preprocess_name"] == "LogAndSign" and na is None
    problem, net_config, _ = util.get_config("cifar_conv", net_name="RNNprop",
                                             problem_options={"data": _data(), "batch_size": 16})
    assert "rp" in net_config and problem().terms[0].hyper["batch_size"] == 16


def test_others_still_unimplemented():
    for name in ("lenet", "nas", "vgg16", "cifar-multi"):
        with pytest.raises(NotImplementedError) as ei:
            util.get_config(name)
    # cifar-multi has its own stub: the reference calls cifar10 with arguments its own cifar10 does not take
    assert "conv_channels" in str(ei.value)


def _write_batches(root, counts, seed):
    """A tiny cifar-10-batches-bin under root: {file name: (labels, CHW uint8 images)}."""
    rng = np.random.default_rng(seed)
    folder = os.path.join(root, "cifar-10-batches-bin")
    os.makedirs(folder)
    out = {}
    for name, n in counts.items():
        labels = rng.integers(0, 10, n).astype(np.uint8)
        chw = rng.integers(0, 256, (n, 3, 32, 32)).astype(np.uint8)
        rec = np.concatenate([labels[:, None], chw.reshape(n, -1)], axis=1)
        rec.tofile(os.path.join(folder, name))
        out[name] = (labels, chw)
    return out


def test_binary_loader(tmp_path, monkeypatch):
    monkeypatch.delenv("L2O_CIFAR10_DIR", raising=False)
    counts = {"data_batch_%d.bin" % i: i + 1 for i in range(1, 6)}
    counts["test_batch.bin"] = 3
    files = _write_batches(str(tmp_path), counts, seed=1)
    loss = problems.cifar10(str(tmp_path), batch_size=2)()
    hyper = loss.terms[0].hyper
    labels = np.concatenate([files["data_batch_%d.bin" % i][0] for i in range(1, 6)])
    chw = np.concatenate([files["data_batch_%d.bin" % i][1] for i in range(1, 6)])
    assert hyper["images"].shape == (len(labels), 3072) and hyper["images"].dtype == np.float32
    np.testing.assert_array_equal(hyper["labels"], labels)
    want = chw.transpose(0, 2, 3, 1).astype(np.float32) / 255.0             # CHW -> HWC, / 255
    np.testing.assert_array_equal(hyper["images"].reshape(-1, 32, 32, 3), want)
    assert hyper["images"].reshape(-1, 32, 32, 3)[0, 1, 2, 0] == chw[0, 0, 1, 2] / np.float32(255.0)
    # mode="test" reads test_batch.bin only; L2O_CIFAR10_DIR replaces the path
    monkeypatch.setenv("L2O_CIFAR10_DIR", str(tmp_path))
    hyper = problems.cifar10("nowhere", mode="test", batch_size=2)().terms[0].hyper
    np.testing.assert_array_equal(hyper["labels"], files["test_batch.bin"][0])
    np.testing.assert_array_equal(hyper["images"].reshape(-1, 32, 32, 3),
                                  files["test_batch.bin"][1].transpose(0, 2, 3, 1).astype(np.float32) / 255.0)
    with pytest.raises(ValueError):
        problems.cifar10("nowhere", mode="validation")


def test_missing_data_error(tmp_path, monkeypatch):
    monkeypatch.delenv("L2O_CIFAR10_DIR", raising=False)
    monkeypatch.chdir(tmp_path)
    for make in (lambda: util.get_config("cifar_conv"), lambda: problems.cifar10("cifar10")):
        with pytest.raises(FileNotFoundError) as ei:
            make()
        assert isinstance(ei.value, NotImplementedError) and isinstance(ei.value, problems.Cifar10DataMissing)
        msg = str(ei.value)
        assert "L2O_CIFAR10_DIR" in msg and "synthetic_cifar10" in msg
        assert os.path.join("cifar10", "cifar-10-batches-bin", "data_batch_1.bin") in msg


def test_unsupported_batch():
    with pytest.raises(NotImplementedError):
        problems.cifar10("cifar10", batch_size=1, data=_data())
    with pytest.raises(NotImplementedError):
        problems.cifar10("cifar10", batch_size=1025, data=_data())


@pytest.mark.parametrize("batch_norm", [True, False])
def test_reference_central_differences(batch_norm):
    """The float64 reference's gradient against central differences on a handful of coordinates of every variable; the
    conv biases under batch norm have gradient 0."""
    d = _data(64, seed=3)
    rng = np.random.default_rng(4)
    images = d["images"].reshape(64, -1) + 0.05 * rng.random((64, 3072))
    net = R.ConvNet(images, d["labels"], batch_norm)
    w = [a.astype(np.float64) for a in R.sample_weights(batch_norm, 5, logit_scale=3.0)]
    rows = rng.integers(0, 64, 12)
    f, g = net.fg(w, rows)
    assert np.isfinite(f) and (net.last_logits > 0).any() and (net.last_logits < 0).any()
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
    if batch_norm:
        assert np.abs(g[1]).max() < 1e-12 * np.abs(g[0]).max()
        assert np.abs(g[5]).max() < 1e-12 * np.abs(g[4]).max()


def test_library_symbols_and_unroll_support():
    import __graft_entry__  # noqa: F401
    lib = _abi.lib()
    for name in ("l2o_cifar_conv_fg", "l2o_cifar_conv_scratch_floats"):
        assert name in _abi.SYMBOLS
        getattr(lib, name)
    assert lib.l2o_abi_version() == 15
    cc = spec_of(O.DM_LOGSIGN).to_c()
    p = _abi.Problem()
    p.kind, p.B_local, p.B_global, p.D, p.M = _abi.PROB_CIFAR_CONV, 1, 1, 13706, 13706
    assert lib.l2o_unroll_supported(C.byref(cc), C.byref(p)) == 0
    assert lib.l2o_unroll_record_supported(C.byref(cc), C.byref(p)) == 0
    m = _abi.CifarConv()
    m.n_data, m.batch_norm = 100, 1
    for batch, ok in ((1, False), (2, True), (128, True), (1024, True), (1025, False)):
        m.batch = batch
        assert (lib.l2o_cifar_conv_scratch_floats(C.byref(m)) > 0) == ok, batch
    m.batch = 128
    assert lib.l2o_cifar_conv_fg(C.byref(m), None, None, None, None, None, None) == _abi.L2O_ERR_ARG
    m.batch = 1
    assert lib.l2o_cifar_conv_fg(C.byref(m), None, None, None, None, None, None) == _abi.L2O_ERR_UNSUPPORTED
    m.batch = 1025
    assert lib.l2o_cifar_conv_fg(C.byref(m), None, None, None, None, None, None) == _abi.L2O_ERR_UNSUPPORTED


def _sampler(idx):
    calls = {"n": 0}

    def sampler(n_evals, b, n_data):
        out = idx[calls["n"]:calls["n"] + n_evals]
        calls["n"] += n_evals
        return out
    return sampler


@pytest.mark.parametrize("net", ["dm_logsign", "rnnprop"])
def test_meta_loss_wiring(engine, net):
    """meta_loss over util.get_config("cifar_conv") on the step-granular path == the oracle's multi-variable unroll over
    the same float32 evaluations, two chained unrolls."""
    data = _data(96, seed=7)
    T, batch = 3, 8
    idx = np.random.default_rng(8).integers(0, 96, size=(2 * (T + 1), batch))
    cfg = O.DM_LOGSIGN if net == "dm_logsign" else O.RNNPROP
    params = make_params(cfg, seed=9, trained_like=True)
    meta.set_random_seed(10)
    problem = util.get_config("cifar_conv", problem_options={"data": data, "batch_size": batch,
                                                             "sampler": _sampler(idx)})[0]
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
    assert engine.calls.count("cifar_conv_fg") == 2 * (T + 1)
    ref = R.ConvNet(data["images"], data["labels"], True)
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
    """One first-order training step on the conv net runs on the recording step path; second derivatives and the
    replicas' training step refuse it."""
    data = _data(64, seed=11)
    meta.set_random_seed(12)
    opt = meta.MetaOptimizer(**_net_config(O.DM_LOGSIGN, make_params(O.DM_LOGSIGN, seed=13, trained_like=True)))
    problem = problems.cifar10("cifar10", batch_size=8, data=data)
    ms = opt.meta_minimize(problem, 2, learning_rate=1e-3)
    w0 = {m: {v: np.array(a) for v, a in d.items()} for m, d in opt._nets["cw"].variables.items()}
    with Session() as sess:
        sess.run(ms.reset)
        c1 = sess.run([ms.fx, ms.update, ms.step])[0]
    assert np.isfinite(c1) and opt.graph.last_path == "steps"
    assert "cifar_conv_fg" in engine.calls
    w1 = opt._nets["cw"].variables
    assert any(not np.array_equal(w0[m][v], np.asarray(w1[m][v])) for m in w0 for v in w0[m])
    opt2 = meta.MetaOptimizer(**_net_config(O.DM_LOGSIGN, make_params(O.DM_LOGSIGN, seed=13, trained_like=True)))
    with pytest.raises(NotImplementedError, match="second_derivatives"):
        opt2.meta_minimize(problem, 2, learning_rate=1e-3, second_derivatives=True)
    from open_l2o_amd.replicas import Replicas
    reps = Replicas(opt, [problem, problem], 2)
    with pytest.raises(ValueError, match="problems.mnist"):
        reps.train_step({}, 1e-3)


def test_replicas_run_one_at_a_time(engine):
    """Replicas.run over conv-net instances: no multi-instance kernel applies, so they run one after the other ("chip")."""
    from open_l2o_amd.replicas import Replicas
    meta.set_random_seed(14)
    opt = meta.MetaOptimizer(**_net_config(O.DM_LOGSIGN, make_params(O.DM_LOGSIGN, seed=15, trained_like=True)))
    problem = problems.cifar10("cifar10", batch_size=4, data=_data(32, seed=16))
    reps = Replicas(opt, [problem, problem], 2)
    reps.reset()
    fx = reps.run({})
    assert reps.last_form == "chip" and fx.shape == (2,) and np.isfinite(fx).all()
    assert engine.calls.count("cifar_conv_fg") >= 2 * 3
