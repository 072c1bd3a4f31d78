"""problems.confocal_microscopy_3d (DM/problems.py:701-956, util.get_config("confocal_microscopy_3d")) without a GPU: the
variables the factory declares, the rejected shapes and the missing-image error, get_config, the float64 reference's own
correctness (central differences), the library's new symbols, and the host wiring -- meta_loss / meta_minimize over the
problem on an oracle engine whose confocal_fg is the float32 torch reference (confocal_reference.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import confocal_reference as R
import oracle as O
from helpers import make_params, rel_err, spec_of
from oracle_engine import OracleEngine
from open_l2o_amd import _abi, _engine, meta, meta_dm_train, meta_rnnprop_eval, problems, util
from open_l2o_amd.session import Session
from test_meta_api import _net_config


class ConfocalOracleEngine(OracleEngine):
    """The oracle engine plus the confocal loss and gradient from the float32 torch reference; keeps what it was given."""

    def lstm_step_multi(self, spec, wpack, segs, pow1, pow2):
        self.multi = getattr(self, "multi", []) + [len(segs)]
        super().lstm_step_multi(spec, wpack, segs, pow1, pow2)

    def confocal_fg(self, d, theta, sim, loss, grads):
        self.calls.append("confocal_fg")
        self.seen = dict(theta=[t.numpy().copy().reshape(-1) for t in theta],
                         sim=None if sim is None else [t.numpy().copy().reshape(-1) for t in sim])
        ref = R.Confocal(d.roi, d.num_points, None if d.img is None else d.img.numpy())
        f, g = ref.fg(self.seen["theta"], self.seen["sim"], want_grad=grads is not None)
        loss.copy_(torch.from_numpy(np.array([f], np.float32)))
        if grads is not None:
            self.seen["g"] = [a.copy() for a in g]
            for t, a in zip(grads, g):
                t.copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32)).view_as(t))


@pytest.fixture
def engine():
    eng = ConfocalOracleEngine()
    old = _engine._default_engine
    _engine.set_default_engine(eng)
    yield eng
    _engine.set_default_engine(old)


# 1. the factory
@pytest.mark.parametrize("points", [1, 3])
def test_variables_names_shapes_order(points):
    loss = problems.confocal_microscopy_3d(batch_size=4, num_points=points, ROI=[5, 7, 6])()
    names = [v.name for v in loss.variables]
    assert names == R.declared_names(points)
    assert "y_sim0" in names and "y_sim_0" not in names and "x_sim_0" in names
    assert names[-2:] == ["bg_var", "bg_sim"] and names.index("bg_var") > names.index("sigmaz_sim_%d" % (points - 1))
    assert names[:6] == ["I_var_0", "x_var_0", "y_var_0", "z_var_0", "sigmaxy_var_0", "sigmaz_var_0"]
    assert all(v.shape == (4, 1) for v in loss.variables)
    trainable = [v.name for v in loss.variables if v.trainable]
    assert trainable == R.trainable_names(points) and len(trainable) == 6 * points + 1
    for v in loss.variables:
        assert v.trainable == ("_var" in v.name), v.name
        assert v.initializer == (("normal", 0.0, 0.01) if v.name == "bg_var" else ("uniform", 0.0, 1.0)), v.name
    (term,) = loss.terms
    assert term.kind == _abi.PROB_CONFOCAL == 9 and term.weight == 1.0
    assert [v.name for v in term.var] == trainable
    assert [v.name for v in term.consts["sim"]] == R.sim_names(points)
    assert term.hyper["roi"] == (5, 7, 6) and term.hyper["num_points"] == points and term.hyper["batch_size"] == 4


def test_defaults_stddev_and_data():
    loss = problems.confocal_microscopy_3d()()
    assert len(loss.variables) == 62 and loss.variables[0].shape == (128, 1) and loss.terms[0].hyper["roi"] == (28, 28, 28)
    fixed = np.linspace(0, 1, 4, dtype=np.float32)
    loss = problems.confocal_microscopy_3d(batch_size=4, num_points=1, stddev=0.5, data={"y_sim0": fixed, "bg_var": fixed})()
    by = {v.name: v for v in loss.variables}
    assert by["bg_var"].initializer[0] == "constant" and np.array_equal(by["bg_var"].initializer[1].reshape(-1), fixed)
    assert by["y_sim0"].initializer[0] == "constant" and by["x_sim_0"].initializer == ("uniform", 0.0, 1.0)
    assert problems.confocal_microscopy_3d(stddev=0.5)().variables[-2].initializer == ("normal", 0.0, 0.5)


def test_inference_variables_and_missing_image():
    img = np.ones((3, 5 * 7 * 6), np.float32)
    loss = problems.confocal_microscopy_3d(batch_size=3, num_points=2, ROI=[5, 7, 6], inference=True, data={"img": img})()
    assert [v.name for v in loss.variables] == R.trainable_names(2) and all(v.trainable for v in loss.variables)
    assert loss.terms[0].consts["sim"] == () and loss.terms[0].hyper["img"].shape == (3, 210)
    for data in (None, {}, {"I_var_0": np.zeros(3)}):
        with pytest.raises(ValueError, match="img"):
            problems.confocal_microscopy_3d(batch_size=3, inference=True, data=data)


def test_out_of_range_shapes():
    for kw in ({"batch_size": 0}, {"batch_size": 1025}, {"num_points": 0}, {"num_points": 9}, {"ROI": [28, 28, 33]},
               {"ROI": [1, 28, 28]}, {"ROI": [28, 28]}):
        with pytest.raises(NotImplementedError, match=r"\[1, 1024\].*\[1, 8\].*\[2, 32\]"):
            problems.confocal_microscopy_3d(**kw)
    problems.confocal_microscopy_3d(batch_size=1024, num_points=8, ROI=[32, 2, 32])
    problems.confocal_microscopy_3d(batch_size=1, num_points=1, ROI=(2, 2, 2))


# 2. util.get_config
def test_get_config():
    problem, net_config, na = util.get_config("confocal_microscopy_3d")
    loss = problem()
    assert loss.terms[0].kind == _abi.PROB_CONFOCAL and na is None
    assert loss.terms[0].hyper["batch_size"] == 32 and loss.terms[0].hyper["num_points"] == 5
    assert loss.terms[0].hyper["roi"] == (28, 28, 28) and loss.variables[0].shape == (32, 1)
    opts = net_config["cw"]["net_options"]
    assert opts == {"layers": (20, 20)} and "preprocess_name" not in opts and net_config["cw"]["net_path"] is None
    problem, net_config, _ = util.get_config("confocal_microscopy_3d", path="p", net_name="RNNprop",
                                             problem_options={"batch_size": 6, "num_points": 2, "ROI": [4, 5, 6]})
    assert list(net_config) == ["rp"] and net_config["rp"]["net"] == "RNNprop" and net_config["rp"]["net_path"] == "p"
    hyper = problem().terms[0].hyper
    assert (hyper["batch_size"], hyper["num_points"], hyper["roi"]) == (6, 2, (4, 5, 6))


# 3. the float64 reference itself
@pytest.mark.parametrize("inference", [False, True])
def test_reference_central_differences(inference):
    roi, batch, points = (5, 7, 6), 3, 2
    theta, sim = R.sample(batch, points, seed=3)
    theta = [a.astype(np.float64) for a in theta]
    sim = None if inference else [a.astype(np.float64) for a in sim]
    img = np.random.default_rng(4).random((batch, 5 * 7 * 6)) if inference else None
    ref = R.Confocal(roi, points, img)
    f, g = ref.fg(theta, sim)
    assert np.isfinite(f) and f > 0 and all(a.shape == (batch,) and np.abs(a).max() > 0 for a in g)
    h = 1e-6
    for k in range(len(theta)):
        for b in range(batch):
            tp, tm = [a.copy() for a in theta], [a.copy() for a in theta]
            tp[k][b] += h
            tm[k][b] -= h
            num = (ref.fg(tp, sim, want_grad=False)[0] - ref.fg(tm, sim, want_grad=False)[0]) / (2 * h)
            scale = max(np.abs(g[k]).max(), 1e-3)
            assert abs(num - g[k][b]) < 1e-6 * scale + 1e-9, (R.trainable_names(points)[k], b, num, g[k][b])


def test_reference_voxel_order_and_axes():
    """One narrow-ish point far towards +x, low y, middle z: the brightest voxel of the [batch, Ry, Rx, Rz] volume sits there,
    and each axis uses its own ROI edge for the centre."""
    roi = (9, 5, 7)
    ref = R.Confocal(roi, 1)
    theta = [np.array([v], np.float64) for v in (1.0, 0.9, 0.1, 0.5, -0.4, -0.4, 0.0)]
    vol = ref.volume([torch.tensor(a) for a in theta], torch.float64)[0].numpy()
    assert vol.shape == (5, 9, 7)
    iy, ix, iz = np.unravel_index(np.argmax(vol), vol.shape)
    cx, cy, cz = 0.5 + 7.5 * 0.9, 0.5 + 3.5 * 0.1, 0.5 + 5.5 * 0.5
    assert (ix, iy, iz) == (round(cx), round(cy), round(cz))
    assert abs(vol.sum() - 2.0) < 0.3 * 2.0            # I0 = 2: most of the integrated intensity lies inside the volume


# 4. the library
def test_library_symbols_and_unroll_support():
    import __graft_entry__  # noqa: F401
    lib = _abi.lib()
    for name in ("l2o_confocal_fg", "l2o_confocal_scratch_floats"):
        assert name in _abi.PROTOTYPES["l2o_abi.h"]
        getattr(lib, name)
    assert lib.l2o_abi_version() == 15
    cc = spec_of(O.DM_IDENTITY).to_c()
    p = _abi.Problem()
    p.kind, p.B_local, p.B_global, p.D, p.M = _abi.PROB_CONFOCAL, 1, 1, 32, 32
    assert lib.l2o_unroll_supported(C.byref(cc), C.byref(p)) == 0
    assert lib.l2o_unroll_record_supported(C.byref(cc), C.byref(p)) == 0
    m = _abi.Confocal()
    for batch, points, roi, ok in ((32, 5, (28, 28, 28), True), (1, 1, (2, 2, 2), True), (1024, 8, (32, 32, 32), True),
                                   (0, 5, (28, 28, 28), False), (1025, 5, (28, 28, 28), False), (32, 0, (28, 28, 28), False),
                                   (32, 9, (28, 28, 28), False), (32, 5, (28, 33, 28), False), (32, 5, (28, 28, 1), False)):
        m.batch, m.num_points = batch, points
        m.roi[0], m.roi[1], m.roi[2] = roi
        assert (lib.l2o_confocal_scratch_floats(C.byref(m)) > 0) == ok, (batch, points, roi)
        want = _abi.L2O_ERR_ARG if ok else _abi.L2O_ERR_UNSUPPORTED      # (NULL arguments: refused before any launch)
        assert lib.l2o_confocal_fg(C.byref(m), None, None, None, None, None, None) == want, (batch, points, roi)


# 5. host wiring
def _fixed(batch, points, seed, inference=False, roi=(5, 4, 6)):
    theta, sim = R.sample(batch, points, seed)
    data = dict(zip(R.trainable_names(points), theta))
    if inference:
        data["img"] = np.random.default_rng(seed + 1).random((batch, int(np.prod(roi)))).astype(np.float32)
    else:
        data.update(zip(R.sim_names(points), sim))
    return theta, (None if inference else sim), data


@pytest.mark.parametrize("net,inference", [("dm_identity", False), ("rnnprop", False), ("dm_identity", True)])
def test_meta_loss_wiring(engine, net, inference):
    """meta_loss over util.get_config("confocal_microscopy_3d") on the step-granular path == the oracle's multi-variable
    unroll over the same float32 evaluations, two chained unrolls."""
    T, batch, points, roi = 3, 4, 2, (5, 4, 6)
    theta, sim, data = _fixed(batch, points, 8, inference, roi)
    cfg = O.DM_IDENTITY if net == "dm_identity" else O.RNNPROP
    params = make_params(cfg, seed=9, trained_like=True)
    meta.set_random_seed(10)
    problem = util.get_config("confocal_microscopy_3d", problem_options={
        "data": data, "batch_size": batch, "num_points": points, "ROI": list(roi), "inference": inference})[0]
    feeds = [{}, {}]
    if cfg.kind == "rnnprop":
        optimizer = meta_rnnprop_eval.MetaOptimizer(0.95, 0.95, **_net_config(cfg, params, key="rp"))
        ml, _, _, step = optimizer.meta_loss(problem, T)
        feeds = [{step: 1}, {step: 1 + T}]
    else:
        optimizer = meta.MetaOptimizer(**_net_config(cfg, params))
        ml = optimizer.meta_loss(problem, T)
    graph = optimizer.graph
    assert len(graph.x) == 6 * points + 1 and all(graph._panel_shape(v) == (1, batch) for v in graph.x)
    with Session() as sess:
        sess.run(ml.reset)
        v0 = [v.eval() for v in graph.x]
        assert all(a.shape == (batch, 1) for a in v0)
        for a, want in zip(v0, theta):
            assert np.array_equal(a.reshape(-1), want)
        loss1, fx1, _ = sess.run([ml.loss, ml.fx, ml.update], feed_dict=feeds[0])
        loss2, fx2, x2, _ = sess.run([ml.loss, ml.fx, ml.x, ml.update], feed_dict=feeds[1])
    assert graph.last_path == "steps"
    assert engine.calls.count("confocal_fg") == 2 * (T + 1)
    # one multi-segment LSTM launch per group of variables that share the net, not one per variable
    assert engine.multi == [6 * points + 1] * (2 * T)
    if sim is not None:
        for a, want in zip(engine.seen["sim"], sim):
            assert np.array_equal(a, want)
    ref = R.Confocal(roi, points, data.get("img"))
    fg = lambda vs, t, wg: ref.fg([np.asarray(a).reshape(-1) for a in vs], sim, wg)      # noqa: E731
    flat = [a.reshape(-1) for a in v0]
    states = [O.net_initial_state(cfg, a.size) for a in flat]
    if cfg.kind == "rnnprop":
        fx_a, va, sa, ma, va2 = O.unroll_multi(fg, cfg, params, flat, states, T, return_moments=True)
        fx_b, vb, _ = O.unroll_multi(fg, cfg, params, va, sa, T, ms=ma, vs=va2, step0=1 + T)
    else:
        fx_a, va, sa = O.unroll_multi(fg, cfg, params, flat, states, T)
        fx_b, vb, _ = O.unroll_multi(fg, cfg, params, va, sa, T)
    assert rel_err(fx1, fx_a[-1]) < 1e-5 and rel_err(loss1, fx_a.sum()) < 1e-5
    assert rel_err(fx2, fx_b[-1]) < 1e-5 and rel_err(loss2, fx_b.sum()) < 1e-5
    for got, want in zip(x2, vb):
        assert got.shape == (batch, 1)
        np.testing.assert_allclose(got.reshape(-1), want, rtol=1e-5, atol=1e-7)


def test_constants_redrawn_on_reset(engine):
    meta.set_random_seed(20)
    opt = meta.MetaOptimizer(**_net_config(O.DM_IDENTITY, make_params(O.DM_IDENTITY, seed=21, trained_like=True)))
    ml = opt.meta_loss(problems.confocal_microscopy_3d(batch_size=3, num_points=1, ROI=[4, 4, 4]), 1)
    with Session() as sess:
        sess.run(ml.reset)
        sess.run([ml.fx, ml.update])
        first = [a.copy() for a in engine.seen["sim"]]
        sess.run(ml.reset)
        sess.run([ml.fx, ml.update])
    assert len(first) == 7 and all(a.shape == (3,) for a in first)
    assert all(not np.array_equal(a, b) for a, b in zip(first, engine.seen["sim"]))
    assert all((a >= 0).all() and (a < 1).all() for a in engine.seen["sim"])


def test_x_scaling_reaches_the_kernel(engine):
    """The training fork's random x-scaling: the kernel is given x * s and its gradients are multiplied by s before the
    optimizer sees them (one step of the identity-preprocessing DM net is checked against the oracle's update)."""
    T, batch, points, roi = 1, 3, 1, (4, 5, 3)
    theta, sim, data = _fixed(batch, points, 30, roi=roi)
    cfg = O.DM_IDENTITY
    params = make_params(cfg, seed=31, trained_like=True)
    meta.set_random_seed(32)
    opt = meta_dm_train.MetaOptimizer(0, **_net_config(cfg, params))
    problem = problems.confocal_microscopy_3d(batch_size=batch, num_points=points, ROI=list(roi), data=data)
    out = opt.meta_loss(problem, T)
    ml, scale_ph = out[0], out[1]
    nv = 6 * points + 1
    assert len(scale_ph) == nv
    scales = [np.exp(np.random.default_rng(33 + k).uniform(-1, 1, (batch, 1))).astype(np.float32) for k in range(nv)]
    with Session() as sess:
        sess.run(ml.reset)
        # commit=False evaluations see x_0 * s first: run ONE unroll and look at what the last evaluation (x_1 * s) saw
        fx, x1, _ = sess.run([ml.fx, ml.x, ml.update], feed_dict=dict(zip(scale_ph, scales)))
    ref = R.Confocal(roi, points)
    fg = ref.flat_fg(batch, sim, scales)
    x0 = np.concatenate(theta)
    f0, g0 = fg(x0, 0)
    st = O.net_initial_state(cfg, x0.size)
    delta, _ = O.net_apply(cfg, params, g0.astype(np.float32), st)
    want_x1 = x0 + np.asarray(delta).reshape(-1)
    got_x1 = np.concatenate([a.reshape(-1) for a in x1])
    np.testing.assert_allclose(got_x1, want_x1, rtol=1e-5, atol=1e-7)
    s_flat = np.concatenate([s.reshape(-1) for s in scales])
    np.testing.assert_allclose(np.concatenate(engine.seen["theta"]), (want_x1 * s_flat).astype(np.float32), rtol=1e-5,
                               atol=1e-7)
    assert rel_err(fx, fg(want_x1.astype(np.float32), 1)[0]) < 1e-5


def test_meta_minimize_and_refusals(engine, monkeypatch):
    """One first-order training step runs on the recording step path; second derivatives and a sharded graph refuse the
    problem."""
    meta.set_random_seed(12)
    opt = meta.MetaOptimizer(**_net_config(O.DM_IDENTITY, make_params(O.DM_IDENTITY, seed=13, trained_like=True)))
    problem = problems.confocal_microscopy_3d(batch_size=4, num_points=2, ROI=[5, 4, 6])
    ms = opt.meta_minimize(problem, 2, learning_rate=1e-3)
    w0 = {m: {v: np.array(a) for v, a in d.items()} for m, d in opt._nets["cw"].variables.items()}
    with Session() as sess:
        sess.run(ms.reset)
        c1 = sess.run([ms.fx, ms.update, ms.step])[0]
    assert np.isfinite(c1) and opt.graph.last_path == "steps"
    assert engine.calls.count("confocal_fg") == 3          # the gradient at x_T as well
    w1 = opt._nets["cw"].variables
    assert any(not np.array_equal(w0[m][v], np.asarray(w1[m][v])) for m in w0 for v in w0[m])
    opt2 = meta.MetaOptimizer(**_net_config(O.DM_IDENTITY, make_params(O.DM_IDENTITY, seed=13, trained_like=True)))
    with pytest.raises(NotImplementedError, match=r"second_derivatives.*confocal_microscopy_3d"):
        opt2.meta_minimize(problem, 2, learning_rate=1e-3, second_derivatives=True)
    from open_l2o_amd import _graph_core
    monkeypatch.setattr(_graph_core, "_EMULATED_WORLD", (0, 2))
    with pytest.raises(NotImplementedError, match=r"confocal_microscopy_3d.*sharded"):
        opt2.meta_loss(problem, 2)


def test_meta_gradient_matches_host_unroll(engine):
    """The first-order meta-gradient of one training step against helpers.oracle_meta_grad over the same float32
    evaluations."""
    from helpers import block_errors, oracle_meta_grad
    T, batch, points, roi = 3, 3, 1, (4, 5, 3)
    theta, sim, data = _fixed(batch, points, 40, roi=roi)
    cfg = O.DM_IDENTITY
    params = make_params(cfg, seed=41, trained_like=True)
    meta.set_random_seed(42)
    opt = meta.MetaOptimizer(**_net_config(cfg, params))
    problem = problems.confocal_microscopy_3d(batch_size=batch, num_points=points, ROI=list(roi), data=data)
    ms = opt.meta_minimize(problem, T, learning_rate=1e-3)
    caps = []
    orig = opt.graph._adam_apply
    opt.graph._adam_apply = lambda grads, lr_, **kw: (caps.append({k: np.array(v, np.float64) for k, v in grads["cw"].items()}),
                                                      orig(grads, lr_, **kw))[1]
    with Session() as sess:
        sess.run(ms.reset)
        sess.run([ms.fx, ms.update, ms.step])
    x0 = np.concatenate(theta).astype(np.float64)
    w = {m: {v: np.asarray(a, np.float64) for v, a in d.items()} for m, d in params.items()}
    fg64 = R.Confocal(roi, points).flat_fg(batch, sim)
    st = tuple((h.astype(np.float64), c.astype(np.float64)) for h, c in O.net_initial_state(cfg, x0.size))
    want, _ = oracle_meta_grad(cfg, w, fg64, x0, st, T)
    errs = block_errors(caps[0], want)
    assert max(errs.values()) < 5e-4, errs
