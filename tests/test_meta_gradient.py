"""The meta-gradient path: MetaOptimizer.meta_minimize (DM/meta.py:398-414).

 * the reference's golden test (L2O-Swarm/src/meta_test.py:50-69) run for real: Adam(0.01) on
   the all-zero Linear net over two 5-step unrolls of f(x) = x^2 -> cost 0.7325327, x 0.8559;
 * the hand-derived BPTT step of the oracle (oracle.net_bwd_step) against torch autograd of the
   restated unroll with stop-gradient on the optimizee gradient (float64);
 * the HIP kernel l2o_cwlstm_bwd_step and the whole train step against those (GPU).
"""
import numpy as np
import pytest
import torch

import oracle as O
from helpers import (ORACLE_CFGS, block_errors, lib_option, make_params, make_problem, max_abs, mnist_fg,
                     oracle_meta_grad, random_state, rel_err, spec_of)
from open_l2o_amd import _abi, _engine, meta, meta_rnnprop_eval, problems
from open_l2o_amd.session import Session
from test_meta_api import _net_config, engine  # noqa: F401  (fixture)
from test_oracle_kat import _torch_lstm_from_sonnet  # noqa: F401


def train(sess, minimize_ops, num_epochs, num_unrolls):
    """L2L training, verbatim from meta_test.py:34-44."""
    step, update, reset, loss_last, x_last = minimize_ops
    for _ in range(num_epochs):
        sess.run(reset)
        for _ in range(num_unrolls):
            cost, final_x, unused_1, unused_2 = sess.run([loss_last, x_last, update, step])
    return cost, final_x


def test_results_reference_golden_through_meta_minimize(engine):
    """meta_test.py:50-69 testResults: 'Tests reproducibility of Torch results'."""
    problem = problems.simple()
    optimizer = meta.MetaOptimizer(net=dict(net="CoordinateWiseDeepLSTM",
                                            net_options={"layers": (), "initializer": "zeros"}))
    minimize_ops = optimizer.meta_minimize(problem, 5)
    with Session() as sess:
        cost, final_x = train(sess, minimize_ops, 1, 2)
    torch_cost = 0.7325327
    torch_final_x = 0.8559
    assert abs(float(cost) - torch_cost) < 5e-5                  # assertAlmostEqual(places=4)
    assert abs(float(final_x[0]) - torch_final_x) < 5e-5
    w = optimizer._nets["net"].variables["linear"]
    # two Adam steps of ~-lr each (the cost above was produced with the weights after the FIRST)
    np.testing.assert_allclose([w["w"][0, 0], w["b"][0]], [-0.02, -0.02], rtol=1e-2)


# ------------------------------------------------------------------ autograd reference
def _torch_meta_grad(cfg, params, prob_kind, prob, x0, state0, T, step0=1, m0=None, v0=None):
    """dL/dtheta of loss = sum_t f(x_t) by torch autograd (float64) with g detached, from the LSTM state state0 and
    (RNNProp) the carried moments m0 / v0 (zeros: None) with exponent step0 + t."""
    W, y = torch.tensor(prob.w.astype(np.float64)), torch.tensor(prob.y.astype(np.float64))

    def f(xx, t):
        r = torch.matmul(W, xx.unsqueeze(-1)).squeeze(-1) - y
        return torch.mean(torch.sum(r * r, 1))
    return _torch_meta_grad_of(cfg, params, f, x0, state0, T, step0, m0, v0)


def _torch_meta_grad_of(cfg, params, f, x0, state0, T, step0=1, m0=None, v0=None):
    """The same for any optimizee ``f(x, t)`` (a torch function of x that may change with the evaluation t = 0..T)."""
    tp = {k: {v: torch.tensor(np.asarray(a, np.float64), requires_grad=True) for v, a in d.items()}
          for k, d in params.items()}
    x = torch.tensor(x0.astype(np.float64))
    st = [[torch.tensor(a.astype(np.float64)) for a in hc] for hc in state0]
    m = torch.zeros_like(x) if m0 is None else torch.tensor(np.asarray(m0, np.float64).reshape(x.shape))
    v = torch.zeros_like(x) if v0 is None else torch.tensor(np.asarray(v0, np.float64).reshape(x.shape))
    H = 20

    def cell(inp, h, c, p):
        z = torch.cat([inp, h], 1) @ p["w_gates"] + p["b_gates"]
        i, j, fg, o = torch.sigmoid(z[:, :H]), torch.tanh(z[:, H:2 * H]), torch.sigmoid(z[:, 2 * H:3 * H] + 1), \
            torch.sigmoid(z[:, 3 * H:])
        cn = fg * c + i * j
        return torch.tanh(cn) * o, cn

    loss = 0
    for t in range(T):
        xr = x.detach().clone().requires_grad_(True)
        fx = f(xr, t)
        g = torch.autograd.grad(fx, xr)[0].detach()
        loss = loss + f(x, t)
        if cfg.kind == "rnnprop":
            k = float(step0 + t)
            m = 0.95 * m + (1 - 0.95) * g
            v = 0.95 * v + (1 - 0.95) * g * g
            mh, vh = m / (1 - 0.95 ** k), v / (1 - 0.95 ** k)
            feats = torch.stack([(mh / (vh.sqrt() + 1e-8)).reshape(-1), (g / (vh.sqrt() + 1e-8)).reshape(-1)], -1)
            a = torch.nn.functional.elu(feats @ tp["input_projection"]["w"] + tp["input_projection"]["b"])
        elif cfg.preprocess_name == "LogAndSign":
            gf = g.reshape(-1, 1)
            eps = float(np.finfo(np.float64).eps)
            a = torch.cat([torch.clamp(torch.log(gf.abs() + eps) / 5, min=-1.0),
                           torch.clamp(gf * float(np.exp(5)), -1.0, 1.0)], 1)
        else:
            a = g.reshape(-1, 1)
        h1, c1 = cell(a, st[0][0], st[0][1], tp["lstm_1"])
        h2, c2 = cell(h1, st[1][0], st[1][1], tp["lstm_2"])
        st = [[h1, c1], [h2, c2]]
        d = h2 @ tp["linear"]["w"] + tp["linear"]["b"]
        d = (torch.tanh(d) if cfg.tanh_output else d) * cfg.scale
        x = x + d.reshape(x.shape)
    loss = loss + f(x, T)
    loss.backward()
    return {k: {v: t.grad.numpy() for v, t in d.items()} for k, d in tp.items()}, float(loss.detach())


@pytest.mark.parametrize("name", ["dm", "dm_logsign", "rnnprop"])
def test_oracle_bptt_matches_torch_autograd(name):
    cfg = ORACLE_CFGS[name]
    rng = np.random.default_rng(100)
    params = {k: {v: a.astype(np.float64) for v, a in d.items()} for k, d in make_params(cfg, 101).items()}
    B, D, T = 3, 4, 5
    prob, x0 = O.Quadratic.sample(rng, B, D, stddev=0.5, dtype=np.float64)
    state0 = random_state(cfg, B * D, 102)
    state0 = tuple((h.astype(np.float64), c.astype(np.float64)) for h, c in state0)
    # a carried start (the 2nd..5th unroll of a training epoch): non-zero state, moments and step0 > 1
    m0 = rng.standard_normal((B, D)) * 0.3
    v0 = rng.random((B, D)) * 0.5 + 0.05
    step0 = 41
    want, loss = _torch_meta_grad(cfg, params, "quadratic", prob, x0, state0, T, step0=step0, m0=m0, v0=v0)
    got, end = oracle_meta_grad(cfg, params, prob, x0, state0, T, m0=m0, v0=v0, step0=step0)
    assert abs(end["loss"] - loss) <= 1e-12 * abs(loss)
    res = O.unroll(prob, cfg, params, x0, state0, T, m0=m0 if cfg.kind == "rnnprop" else None,
                   v0=v0 if cfg.kind == "rnnprop" else None, step0=step0)
    np.testing.assert_array_equal(end["x"], res.x)
    if cfg.kind == "rnnprop":
        np.testing.assert_array_equal(end["m"], res.m)
        np.testing.assert_array_equal(end["v"], res.v)
    for mod in want:
        for var in want[mod]:
            np.testing.assert_allclose(got[mod][var].reshape(want[mod][var].shape), want[mod][var],
                                       rtol=1e-8, atol=1e-11, err_msg="%s/%s" % (mod, var))


# ------------------------------------------------------------------ the MLP optimizee (problems.mnist)
def _torch_mlp_loss(images, labels, shapes, idx, activation, scales=None):
    """f(x, t) of _torch_meta_grad_of for the MLP optimizee, written in torch: the flat x split by ``shapes`` into
    [w0, b0, w1, b1, ...], the mean softmax cross-entropy of minibatch row idx[t]; with x-scale s evaluated at x * s
    (autograd then gives s * grad f(x * s) by itself)."""
    X, Y = torch.tensor(images.astype(np.float64)), torch.tensor(labels.astype(np.int64))
    sizes = [int(np.prod(sh)) for sh in shapes]
    s = None if scales is None else torch.tensor(np.concatenate([a.reshape(-1) for a in scales]).astype(np.float64))
    nl = len(shapes) // 2

    def f(x, t):
        parts = torch.split(x if s is None else x * s, sizes)
        ix = torch.tensor(np.asarray(idx[t], np.int64))
        a = X[ix]
        for l in range(nl):
            a = a @ parts[2 * l].reshape(shapes[2 * l]) + parts[2 * l + 1]
            if l < nl - 1:
                a = torch.sigmoid(a) if activation == "sigmoid" else torch.relu(a)
        return torch.nn.functional.cross_entropy(a, Y[ix])
    return f


MLP_CASES = [pytest.param((20,), "sigmoid", False, id="20-sigmoid"),
             pytest.param((20,), "relu", True, id="20-relu-xscale"),
             pytest.param((20, 20), "sigmoid", False, id="20x20-sigmoid"),
             pytest.param((20, 20), "relu", False, id="20x20-relu")]


@pytest.mark.parametrize("layers,activation,scaled", MLP_CASES)
@pytest.mark.parametrize("name", ["dm", "dm_logsign", "rnnprop"])
def test_oracle_mlp_meta_grad_matches_torch_autograd(name, layers, activation, scaled):
    """The float64 reference of the MNIST meta-gradient (helpers.oracle_meta_grad over helpers.mnist_fg: all the MLP's
    variables as one flat vector through the shared coordinate-wise net, minibatch row t at evaluation t) == torch
    autograd of the restated unroll, on a small MLP (36-pixel images), a different minibatch every evaluation, g
    detached, from a carried start (non-zero state, m0 / v0, step0 = 41) and once with the train forks' x-scale."""
    cfg = ORACLE_CFGS[name]
    rng = np.random.default_rng(110)
    params = {k: {v: a.astype(np.float64) for v, a in d.items()} for k, d in make_params(cfg, 111).items()}
    n_in, n_data, batch, T = 36, 40, 8, 5
    images = rng.random((n_data, n_in)).astype(np.float32)
    labels = rng.integers(0, 10, n_data).astype(np.int32)
    mlp = O.MnistMLP(images, labels, activation)
    widths = [n_in] + list(layers) + [10]
    shapes = [sh for l in range(len(widths) - 1) for sh in ((widths[l], widths[l + 1]), (widths[l + 1],))]
    v0 = [rng.standard_normal(sh) * 0.3 for sh in shapes]       # (large enough that every activation bends)
    x0 = np.concatenate([a.reshape(-1) for a in v0])
    N = x0.size
    idx = rng.integers(0, n_data, size=(T + 1, batch))
    assert len({tuple(r) for r in idx}) == T + 1                 # a different minibatch at every evaluation
    state0 = tuple((h.astype(np.float64), c.astype(np.float64)) for h, c in random_state(cfg, N, 112))
    m0 = rng.standard_normal(N) * 0.3
    v0m = rng.random(N) * 0.5 + 0.05
    step0 = 41
    scales = [np.exp(rng.uniform(-1, 1, sh)) for sh in shapes] if scaled else None
    want, loss = _torch_meta_grad_of(cfg, params, _torch_mlp_loss(images, labels, shapes, idx, activation, scales),
                                     x0, state0, T, step0=step0, m0=m0, v0=v0m)
    got, end = oracle_meta_grad(cfg, params, mnist_fg(mlp, shapes, idx, scales), x0, state0, T, m0=m0, v0=v0m,
                                step0=step0)
    assert abs(end["loss"] - loss) <= 1e-12 * abs(loss)
    for mod in want:
        for var in want[mod]:
            np.testing.assert_allclose(got[mod][var].reshape(want[mod][var].shape), want[mod][var],
                                       rtol=1e-8, atol=1e-11, err_msg="%s/%s" % (mod, var))
    # the concatenation steps exactly as one net state / pair of moments per variable does (O.unroll_multi)
    sizes = np.cumsum([0] + [a.size for a in v0])
    rows = lambda a, i: a[sizes[i]:sizes[i + 1]]
    sts = [tuple((rows(h, i), rows(c, i)) for h, c in state0) for i in range(len(v0))]
    rn = cfg.kind == "rnnprop"

    def fg_multi(vs, t, wg):
        f, g = mnist_fg(mlp, shapes, idx, scales)(np.concatenate([a.reshape(-1) for a in vs]), t)
        return f, [rows(g, i).reshape(shapes[i]) for i in range(len(vs))]
    res = O.unroll_multi(fg_multi, cfg, params, v0, sts, T, step0=step0, return_moments=True,
                         ms=[rows(m0, i).reshape(shapes[i]) for i in range(len(v0))] if rn else None,
                         vs=[rows(v0m, i).reshape(shapes[i]) for i in range(len(v0))] if rn else None)
    np.testing.assert_allclose(end["x"], np.concatenate([a.reshape(-1) for a in res[1]]), rtol=1e-12, atol=1e-15)
    assert abs(end["loss"] - res[0].sum()) <= 1e-12 * abs(loss)


@pytest.mark.parametrize("layers", [(20,), (20, 20, 20)])
@pytest.mark.parametrize("name", ["dm", "dm_logsign", "rnnprop"])
def test_mnist_train_steps_on_the_oracle_engine(name, layers, monkeypatch):
    """Two MNIST meta_minimize steps (reset, then one from carried state) on the OracleEngine: the gradient handed to the
    meta-Adam == the float64 reference from the step's own start, on the minibatch rows the graph drew (read back from
    its index buffer), every block at 5e-4 of its largest entry; the carry per variable.  That holds the host's part of
    the MNIST meta-gradient -- which row feeds g_t and g_final, the moment history, step0, the four (784-20-10) or eight
    ((20, 20, 20): the limit of one multi-panel launch) panels in ONE BPTT launch, the gather into the meta-Adam --
    without a GPU."""
    from oracle_engine import OracleEngine
    from test_training_gradient import Trainer, check_carry, check_grad, split_carry, spy_bwd_unroll
    eng = OracleEngine()
    old = _engine._default_engine
    _engine.set_default_engine(eng)
    try:
        cfg = ORACLE_CFGS[name]
        T, batch = 4, 16
        data = problems.synthetic_mnist(100, seed=12)
        mlp = O.MnistMLP(data["images"], data["labels"].astype(np.int32), "sigmoid")
        meta.set_random_seed(13)
        tr = Trainer(eng, name, make_params(cfg, seed=14, trained_like=True),
                     problems.mnist(layers=layers, batch_size=batch, data=data), T)
        shapes = [tuple(v.shape) for v in tr.graph.x]
        widths = [784] + list(layers) + [10]
        assert shapes == [sh for l in range(len(widths) - 1) for sh in ((widths[l], widths[l + 1]), (widths[l + 1],))]
        launches = spy_bwd_unroll(eng, monkeypatch)
        tr.reset()
        prev = None
        for k in range(2):
            snap = tr.snapshot()
            if prev is not None:
                for j, (sv, ev, e32) in enumerate(zip(snap["vars"], split_carry(prev, shapes), split_carry(prev32, shapes))):
                    check_carry(sv, ev, e32, "carry into step %d, variable %d" % (k, j))
            got = tr.train_step()
            assert tr.graph.last_path == "steps" and launches == [[(1, int(np.prod(sh))) for sh in shapes]] * (k + 1)
            idx = eng.to_numpy(tr.graph._mlp_idx[0])
            assert idx.shape == (T + 1, batch)
            want, prev = tr.reference(mnist_fg(mlp, shapes, idx), snap)
            prev32 = tr.reference(mnist_fg(mlp, shapes, idx), snap, np.float32)[1]
            check_grad(got, want, "step %d" % k)
    finally:
        _engine.set_default_engine(old)


@pytest.mark.parametrize("name", ["dm", "dm_logsign", "rnnprop"])
def test_train_step_gradient_and_adam(engine, name):
    """One sess.run([fx, update, step]) == forward + BPTT + Adam: the gradient handed to Adam is the autograd gradient
    (every block at 5e-4 of its largest entry), and the weights move exactly as tf.train.AdamOptimizer would move them
    given it."""
    cfg = ORACLE_CFGS[name]
    params = make_params(cfg, seed=103, trained_like=True)
    B, D, T = 4, 6, 7
    prob, x0, _ = make_problem("quadratic", B, D, seed=104)
    problem = problems.quadratic(B, D, data={"w": prob.w, "y": prob.y, "x": x0})
    key = "rp" if cfg.kind == "rnnprop" else "cw"
    feed = {}
    if cfg.kind == "rnnprop":
        optimizer = meta_rnnprop_eval.MetaOptimizer(0.95, 0.95, **_net_config(cfg, params, key=key))
        ms, _, _, step_ph = optimizer.meta_minimize(problem, T, learning_rate=0.01)
        feed = {step_ph: 1}
    else:
        optimizer = meta.MetaOptimizer(**_net_config(cfg, params, key=key))
        ms = optimizer.meta_minimize(problem, T, learning_rate=0.01)
    cap = {}
    graph = optimizer.graph
    orig = graph._adam_apply
    graph._adam_apply = lambda grads, lr, **kw: (cap.update(grads={k: np.array(v) for k, v in grads[key].items()}),
                                                 orig(grads, lr, **kw))[1]
    with Session() as sess:
        sess.run(ms.reset)
        cost = sess.run([ms.fx, ms.update, ms.step], feed_dict=feed)[0]
    st0 = O.net_initial_state(cfg, B * D)
    want, loss = _torch_meta_grad(cfg, params, "quadratic", prob, x0, st0, T)
    for k, err in block_errors(cap["grads"], want).items():
        assert err < 5e-4, (k, err)
    res = O.unroll(prob, cfg, params, x0, st0, T)
    assert rel_err(cost, res.fx[-1]) < 1e-5 and rel_err(res.loss, loss) < 1e-5
    new = optimizer._nets[key].variables
    for mod in want:
        for var in want[mod]:
            g = want[mod][var].astype(np.float32).reshape(params[mod][var].shape)
            expect, _, _ = O.tf_adam_step(params[mod][var], g, np.zeros_like(g), np.zeros_like(g), 1, lr=0.01)
            # Adam's first step is -lr * sign(g) wherever |g| >> eps: compare where the sign is unambiguous
            mask = np.abs(g) > 1e-5 * np.abs(g).max()
            np.testing.assert_allclose(new[mod][var][mask], expect[mask], rtol=2e-4, atol=1e-7,
                                       err_msg="%s/%s" % (mod, var))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["dm", "dm_logsign", "rnnprop"])
@pytest.mark.parametrize("B,D", [(3, 10), (2, 37)])
def test_bwd_step_kernel_vs_oracle(name, B, D):
    """l2o_cwlstm_bwd_step (teacher-forced, random state / carries) == oracle.net_bwd_step."""
    eng = _engine.HipEngine()
    cfg = ORACLE_CFGS[name]
    spec = spec_of(cfg)
    params = make_params(cfg, seed=105)
    rng = np.random.default_rng(106)
    N = B * D
    g = rng.standard_normal((B, D)).astype(np.float32)
    state = random_state(cfg, N, 107)
    dx = rng.standard_normal(N).astype(np.float32)
    carry = tuple((rng.standard_normal((N, 20)) * 0.3).astype(np.float32) for _ in range(4))
    m = (rng.standard_normal((B, D)) * 0.1).astype(np.float32)
    v = (rng.random((B, D)) * 0.1 + 0.01).astype(np.float32)
    k = 5
    pw = float(np.float32(0.95)) ** k
    if cfg.kind == "rnnprop":
        dt = np.float32
        mh, vh = m / (dt(1) - dt(pw)), v / (dt(1) - dt(pw))
        inputs = ((mh / (np.sqrt(vh) + dt(1e-8))).reshape(-1), (g / (np.sqrt(vh) + dt(1e-8))).reshape(-1))
    else:
        inputs = g.reshape(-1)
    cout, rows = O.net_bwd_step(cfg, params, inputs, state, dx, carry)
    P = cfg.in_dim
    t = eng.tensor
    io = dict(g=t(g), m=t(m), v=t(v), st_prev=eng.state_pack(*[t(a) for hc in state for a in hc], B, D),
              dx_next=t(dx), carry_in=t(np.stack(carry)), carry_out=eng.zeros(4, N, 20),
              act1=eng.zeros(N, P + 20), dz1=eng.zeros(N, 80), act2=eng.zeros(N, 40), dz2=eng.zeros(N, 80),
              h2=eng.zeros(N, 20), dd=eng.zeros(N), feats=eng.zeros(N, 2), du=eng.zeros(N, 20))
    names = {"w_gates1": ("lstm_1", "w_gates"), "b_gates1": ("lstm_1", "b_gates"), "w_gates2": ("lstm_2", "w_gates"),
             "b_gates2": ("lstm_2", "b_gates"), "w_lin": ("linear", "w"), "b_lin": ("linear", "b"),
             "w_fc": ("input_projection", "w"), "b_fc": ("input_projection", "b")}
    wdev = {kk: t(params[mm][nn]) for kk, (mm, nn) in names.items() if mm in params}
    da = rows.pop("da")
    if cfg.kind != "rnnprop":                  # u = dL/dg of the DM nets (second_derivatives): the preprocess adjoint
        io["dg"] = eng.zeros(N)
        rows["dg"] = O.preprocess_bwd(cfg, g, da)
    eng.bwd_step(spec, wdev, io, pw, pw, B, D)
    for kk, ref in rows.items():
        got = eng.to_numpy(io[kk]).reshape(ref.shape)
        assert max_abs(got, ref) < 2e-5 * max(1.0, float(np.abs(ref).max())), kk
    got = eng.to_numpy(io["carry_out"])
    for i in range(4):
        assert max_abs(got[i], cout[i]) < 2e-5 * max(1.0, float(np.abs(cout[i]).max()))


def test_training_harness_learns(engine, tmp_path):
    """scripts/train_dm.py's schedule (DM/train_dm.py: epochs of truncated-BPTT segments, periodic
    evaluation, best-model .l2l checkpoints) runs and the meta-loss goes down."""
    import argparse
    import sys
    import os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
    import _train_common as TC
    flags = argparse.Namespace(save_path=str(tmp_path), num_epochs=12, evaluation_period=4, evaluation_epochs=2,
                               num_steps=20, unroll_length=5, learning_rate=0.01, second_derivatives=False,
                               problem="quadratic", if_scale=True, rd_scale_bound=1.0, if_cl=False, min_num_eval=3,
                               if_mt=False, num_mt=1, seed=11, batch_size=4, num_dims=3)
    tr = TC.Trainer(flags, rnnprop=False)
    w0 = {k: v.copy() for k, v in tr.optimizer._nets["cw"].variables["linear"].items()}
    tr.run()
    w1 = tr.optimizer._nets["cw"].variables["linear"]
    assert not np.array_equal(w0["w"], w1["w"])                      # the meta-step moved the weights
    saved = sorted(os.listdir(str(tmp_path)))
    assert "cw.l2l-0" in saved and any(s.startswith("cw.l2l-") and s != "cw.l2l-0" for s in saved)


@pytest.mark.parametrize("name,B,D", [("dm", 5, 24), ("rnnprop", 5, 24), ("dm", 3, 256), ("rnnprop", 2, 384)])
def test_recording_fused_unroll_equals_step_path(engine, name, B, D, monkeypatch):
    """meta_minimize on a fused-size problem takes the recording unroll (l2o_unroll_record: one
    launch that stores the per-step history) -- the LDS-resident forms for D <= 128, the streaming form
    beyond (config-3 sizes: <= 3 launches per training segment); its meta-gradient == the step-granular path's."""
    cfg = ORACLE_CFGS[name]
    rn = cfg.kind == "rnnprop"
    params = make_params(cfg, seed=71, trained_like=True)
    T = 6
    if D > 128 and engine.name != "hip":
        pytest.skip("the streaming sizes are a property of the HIP kernels")
    prob, x0, _ = make_problem("quadratic", B, D, seed=72)
    got = {}
    for mode in ("fused", "steps"):
        if mode == "steps":
            monkeypatch.setenv("L2O_DISABLE_FUSED", "1")
            monkeypatch.setenv("L2O_BWD_ALIGNED_ONLY", "1")             # (D = 24: the per-step BPTT kernels as reference)
        else:
            monkeypatch.delenv("L2O_DISABLE_FUSED", raising=False)
            monkeypatch.delenv("L2O_BWD_ALIGNED_ONLY", raising=False)
        problem = problems.quadratic(B, D, data={"w": prob.w, "y": prob.y, "x": x0})
        if rn:
            opt = meta_rnnprop_eval.MetaOptimizer(0.95, 0.95, **_net_config(cfg, params, key="rp"))
            out = opt.meta_minimize(problem, T, learning_rate=1e-3)
            ms, step_ph = out[0], out[3]
        else:
            opt = meta.MetaOptimizer(**_net_config(cfg, params))
            ms, step_ph = opt.meta_minimize(problem, T, learning_rate=1e-3), None
        graph = opt.graph
        cap = {}
        orig = graph._adam_apply
        graph._adam_apply = lambda grads, lr, **kw: (cap.update(grads=grads), orig(grads, lr, **kw))[1]
        with Session() as sess:
            sess.run(ms.reset)
            feed = {step_ph: 3} if rn else {}
            cost = sess.run([ms.fx, ms.update, ms.step], feed_dict=feed)[0]
            x_after = graph.x[0].eval()
        assert graph.last_path == mode
        got[mode] = (cost, x_after, cap["grads"])
    assert rel_err(got["fused"][0], got["steps"][0]) < 1e-5
    assert max_abs(got["fused"][1], got["steps"][1]) < 1e-5
    key = "rp" if rn else "cw"
    for k, gref in got["steps"][2][key].items():
        g = got["fused"][2][key][k]
        scale = max(float(np.abs(gref).max()), 1e-12)
        assert float(np.abs(np.asarray(g) - np.asarray(gref)).max()) / scale < 2e-4, k


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["dm", "dm_logsign", "rnnprop"])
def test_bwd_tile_kernel_equals_generic_kernel(name, monkeypatch):
    """L2O_OPT_BWD_KERNEL: the matrix-core BPTT (0, the default) and k_cwlstm_bwd_tile (1: tile-aligned panels, LDS-tiled
    I/O, four lanes per coordinate) against the generic one-thread-per-coordinate kernel (2): same meta-gradient."""
    eng = _engine.HipEngine()
    old = _engine._default_engine
    _engine.set_default_engine(eng)
    try:
        cfg = ORACLE_CFGS[name]
        rn = cfg.kind == "rnnprop"
        params = make_params(cfg, seed=81, trained_like=True)
        B, D, T = 3, 32, 4                                   # D % 16 == 0 -> the tile kernel
        prob, x0, _ = make_problem("quadratic", B, D, seed=82)
        got = {}
        for mode in ("mfma", "tile", "generic"):
            _abi.set_option(_abi.OPT_BWD_KERNEL, {"mfma": 0, "tile": 1, "generic": 2}[mode])
            problem = problems.quadratic(B, D, data={"w": prob.w, "y": prob.y, "x": x0})
            if rn:
                opt = meta_rnnprop_eval.MetaOptimizer(0.95, 0.95, **_net_config(cfg, params, key="rp"))
                out = opt.meta_minimize(problem, T, learning_rate=1e-3)
                ms, step_ph = out[0], out[3]
            else:
                opt = meta.MetaOptimizer(**_net_config(cfg, params))
                ms, step_ph = opt.meta_minimize(problem, T, learning_rate=1e-3), None
            graph = opt.graph
            cap = {}
            orig = graph._adam_apply
            graph._adam_apply = lambda grads, lr, **kw: (cap.update(grads=grads), orig(grads, lr, **kw))[1]
            with Session() as sess:
                sess.run(ms.reset)
                sess.run([ms.fx, ms.update, ms.step], feed_dict={step_ph: 2} if rn else {})
            got[mode] = cap["grads"]["rp" if rn else "cw"]
        for k, gref in got["generic"].items():
            scale = max(float(np.abs(gref).max()), 1e-12)
            for mode in ("mfma", "tile"):
                assert float(np.abs(np.asarray(got[mode][k]) - np.asarray(gref)).max()) / scale < 1e-4, (mode, k)
    finally:
        _abi.set_option(_abi.OPT_BWD_KERNEL, 0)
        _engine.set_default_engine(old)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["tile", "mfma"])
@pytest.mark.parametrize("name", ["dm", "dm_logsign", "rnnprop"])
def test_bwd_multi_equals_per_panel_bwd_step(name, form):
    """l2o_cwlstm_bwd_multi (ONE launch for the panels that share a network: the five variables of the
    mnist optimizee, DM/meta.py:231-235) == l2o_cwlstm_bwd_step called once per panel, row for row
    of A / Bm and carry for carry.  Panels: tile-aligned (2 x 32), one flat ragged row (1 x 200),
    one short row (1 x 10).  form == "mfma": the multi-panel launch gets the packed weights and runs
    k_cwlstm_bwd_mfma (bf16x3 matrix-core products, csrc/l2o_bwd_mfma.h); the per-panel reference stays
    on the fp32 tile kernel -- agreement to fp32 rounding (2e-5 of the largest entry) instead of bits."""
    eng = _engine.HipEngine()
    cfg = ORACLE_CFGS[name]
    spec = spec_of(cfg)
    params = make_params(cfg, seed=91, trained_like=True)
    names = {"w_gates1": ("lstm_1", "w_gates"), "b_gates1": ("lstm_1", "b_gates"), "w_gates2": ("lstm_2", "w_gates"),
             "b_gates2": ("lstm_2", "b_gates"), "w_lin": ("linear", "w"), "b_lin": ("linear", "b"),
             "w_fc": ("input_projection", "w"), "b_fc": ("input_projection", "b")}
    t = eng.tensor
    wdev = {kk: t(params[mm][nn]) for kk, (mm, nn) in names.items() if mm in params}
    fc = cfg.kind == "rnnprop"
    P = cfg.in_dim
    K1 = P + 20
    KA = K1 + 60 + (2 if fc else 0) + 1
    KB = 161 + (20 if fc else 0)
    shapes = [(2, 32), (1, 200), (1, 10)]
    rows = [(b * d + 15) // 16 * 16 for b, d in shapes]
    R = sum(rows)
    rng = np.random.default_rng(92)
    cin_all = (rng.standard_normal((4, R, 20)) * 0.3).astype(np.float32)
    segs, ref_A, ref_B, ref_c = [], [], [], []
    row = 0
    for i, (B, D) in enumerate(shapes):
        N = B * D
        g = t(rng.standard_normal((B, D)).astype(np.float32))
        m = t((rng.standard_normal((B, D)) * 0.1).astype(np.float32))
        v = t((rng.random((B, D)) * 0.1 + 0.01).astype(np.float32))
        state = random_state(cfg, N, 93 + i)
        st = eng.state_pack(*[t(a) for hc in state for a in hc], B, D)
        dx = t(rng.standard_normal(N).astype(np.float32))
        segs.append(dict(g=g, m=m if fc else None, v=v if fc else None, st_prev=st, dx_next=dx, B=B, D=D))
        # reference: the single-panel entry point on its own buffers
        A1, B1 = eng.zeros(rows[i], KA), eng.zeros(rows[i], KB)
        co = eng.zeros(4, N, 20)
        io = dict(g=g, m=m if fc else None, v=v if fc else None, st_prev=st, dx_next=dx,
                  carry_in=t(np.ascontiguousarray(cin_all[:, row:row + N])), carry_out=co, a_stride=KA, b_stride=KB,
                  act1=A1[:N, 0:K1], act2=A1[:N, K1:K1 + 40], h2=A1[:N, K1 + 40:K1 + 60],
                  dz1=B1[:N, 0:80], dz2=B1[:N, 80:160], dd=B1[:N, 160:161])
        if fc:
            io.update(feats=A1[:N, K1 + 60:K1 + 62], du=B1[:N, 161:181])
        eng.bwd_step(spec, wdev, io, 0.9, 0.8, B, D)
        ref_A.append(eng.to_numpy(A1)[:N]); ref_B.append(eng.to_numpy(B1)[:N]); ref_c.append(eng.to_numpy(co))
        row += rows[i]
    A, Bm = eng.zeros(R, KA), eng.zeros(R, KB)
    cout = eng.zeros(4, R, 20)
    wmulti = dict(wdev, wpack=eng.pack_weights(spec, params)) if form == "mfma" else wdev
    eng.bwd_multi(spec, wmulti, segs, t(cin_all), cout, A, Bm, 0.9, 0.8)
    A, Bm, cout = eng.to_numpy(A), eng.to_numpy(Bm), eng.to_numpy(cout)

    def same(got, ref, what):
        if form == "tile":
            np.testing.assert_array_equal(got, ref, err_msg=what)
        else:
            # column-wise scale: the columns of A / Bm differ by orders of magnitude
            tol = 2e-5 * np.maximum(np.abs(ref).max(axis=0, keepdims=True), 1e-30) + 1e-9
            assert (np.abs(got - ref) <= tol).all(), (what, float(np.abs(got - ref).max()))

    row = 0
    for i, (B, D) in enumerate(shapes):
        N = B * D
        same(A[row:row + N], ref_A[i], "A panel %d" % i)
        same(Bm[row:row + N], ref_B[i], "Bm panel %d" % i)
        for a in range(4):
            same(cout[a, row:row + N], ref_c[i][a], "carry %d panel %d" % (a, i))
        assert not A[row + N:row + rows[i]].any() and not Bm[row + N:row + rows[i]].any()   # padding rows stay zero
        row += rows[i]


@pytest.mark.gpu
@pytest.mark.parametrize("dx_mode", ["g_final", "table"])
@pytest.mark.parametrize("name", ["dm", "dm_logsign", "rnnprop"])
def test_bwd_unroll_equals_stepwise_bwd_multi(name, dx_mode):
    """l2o_cwlstm_bwd_unroll (T steps in one launch, carries in registers, dL/d(delta_t) either from the
    pointer table or accumulated from g_final: loss = sum_t fx_t, DM/meta.py:376) == T calls of
    l2o_cwlstm_bwd_multi on the fp32 tile kernel with the carries going through memory."""
    eng = _engine.HipEngine()
    cfg = ORACLE_CFGS[name]
    spec = spec_of(cfg)
    params = make_params(cfg, seed=95, trained_like=True)
    names = {"w_gates1": ("lstm_1", "w_gates"), "b_gates1": ("lstm_1", "b_gates"), "w_gates2": ("lstm_2", "w_gates"),
             "b_gates2": ("lstm_2", "b_gates"), "w_lin": ("linear", "w"), "b_lin": ("linear", "b"),
             "w_fc": ("input_projection", "w"), "b_fc": ("input_projection", "b")}
    t_ = eng.tensor
    wdev = {kk: t_(params[mm][nn]) for kk, (mm, nn) in names.items() if mm in params}
    wfused = dict(wdev, wpack=eng.pack_weights(spec, params))
    fc = cfg.kind == "rnnprop"
    P = cfg.in_dim
    KA = P + 20 + 60 + (2 if fc else 0) + 1
    KB = 161 + (20 if fc else 0)
    T, step0 = 4, 3
    shapes = [(2, 32), (1, 40)]
    rows = [(b * d + 15) // 16 * 16 for b, d in shapes]
    R = sum(rows)
    rng = np.random.default_rng(96)
    panels = []
    for i, (B, D) in enumerate(shapes):
        N = B * D
        gs = [t_((rng.standard_normal((B, D)) * 0.5).astype(np.float32)) for _ in range(T)]
        ms = [t_((rng.standard_normal((B, D)) * 0.1).astype(np.float32)) for _ in range(T)] if fc else [None] * T
        vs = [t_((rng.random((B, D)) * 0.1 + 0.01).astype(np.float32)) for _ in range(T)] if fc else [None] * T
        sts = []
        for k in range(T):
            state = random_state(cfg, N, 200 + 10 * i + k)
            sts.append(eng.state_pack(*[t_(a) for hc in state for a in hc], B, D))
        g_final = t_((rng.standard_normal(N) * 0.5).astype(np.float32))
        dxs, acc = [None] * T, g_final.clone()
        for k in reversed(range(T)):
            dxs[k] = acc
            acc = acc + gs[k].reshape(N)
        panels.append(dict(B=B, D=D, gs=gs, ms=ms, vs=vs, sts=sts, dxs=dxs, g_final=g_final))
    cin0 = t_((rng.standard_normal((4, R, 20)) * 0.3).astype(np.float32))
    # reference: step by step on the fp32 tile kernel
    A0, B0 = eng.zeros(T, R, KA), eng.zeros(T, R, KB)
    cin, cout = cin0.clone(), eng.zeros(4, R, 20)
    b1, b2 = float(np.float32(spec.beta1)), float(np.float32(spec.beta2))
    for k in reversed(range(T)):
        segs = [dict(g=pn["gs"][k], m=pn["ms"][k], v=pn["vs"][k], st_prev=pn["sts"][k], dx_next=pn["dxs"][k],
                     B=pn["B"], D=pn["D"]) for pn in panels]
        eng.bwd_multi(spec, wdev, segs, cin, cout, A0[k], B0[k], b1 ** (step0 + k), b2 ** (step0 + k))
        cin, cout = cout, cin
    ref_c = eng.to_numpy(cin)
    A1, B1 = eng.zeros(T, R, KA), eng.zeros(T, R, KB)
    c1 = eng.zeros(4, R, 20)
    fused_panels = [dict(pn, dxs=None) if dx_mode == "g_final" else dict(pn, g_final=None) for pn in panels]
    eng.bwd_unroll(spec, wfused, fused_panels, T, step0, A1, B1, carry_in=cin0, carry_out=c1)

    def close(got, ref, what):
        tol = 2e-5 * np.maximum(np.abs(ref).max(axis=0, keepdims=True), 1e-30) + 1e-9
        assert (np.abs(got - ref) <= tol).all(), (what, float(np.abs(got - ref).max()))

    A0, B0, A1, B1, c1 = [eng.to_numpy(x) for x in (A0, B0, A1, B1, c1)]
    for k in range(T):
        close(A1[k], A0[k], "A step %d" % k)
        close(B1[k], B0[k], "Bm step %d" % k)
    row = 0
    for i, (B, D) in enumerate(shapes):                     # (the padding rows of a ragged last tile are not defined)
        for a in range(4):
            close(c1[a, row:row + B * D], ref_c[a, row:row + B * D], "carry %d panel %d" % (a, i))
        row += rows[i]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["dm", "dm_logsign", "rnnprop"])
def test_bwd_unroll_ragged_problem_tiles(name):
    """l2o_cwlstm_bwd_unroll on panels whose D is NOT a multiple of 16 with B > 1 (BASELINE config 4: d = 100): the
    tiles are per problem, ceil(D / 16) each with a ragged last one -- the packed-state layout the forward records --
    and the rows of A / Bm / the carries are 16 per tile (padding rows zero).  Reference: the one-thread-per-coordinate
    kernel (l2o_cwlstm_bwd_step, any shape), step by step, rows mapped coordinate -> (tile, lane)."""
    eng = _engine.HipEngine()
    cfg = ORACLE_CFGS[name]
    spec = spec_of(cfg)
    params = make_params(cfg, seed=97, trained_like=True)
    names = {"w_gates1": ("lstm_1", "w_gates"), "b_gates1": ("lstm_1", "b_gates"), "w_gates2": ("lstm_2", "w_gates"),
             "b_gates2": ("lstm_2", "b_gates"), "w_lin": ("linear", "w"), "b_lin": ("linear", "b"),
             "w_fc": ("input_projection", "w"), "b_fc": ("input_projection", "b")}
    t_ = eng.tensor
    wdev = {kk: t_(params[mm][nn]) for kk, (mm, nn) in names.items() if mm in params}
    wfused = dict(wdev, wpack=eng.pack_weights(spec, params))
    fc = cfg.kind == "rnnprop"
    P = cfg.in_dim
    K1 = P + 20
    KA = K1 + 60 + (2 if fc else 0) + 1
    KB = 161 + (20 if fc else 0)
    T, step0 = 3, 2
    shapes = [(3, 100), (2, 37), (1, 40), (4, 32)]
    rows = [b * ((d + 15) // 16) * 16 for b, d in shapes]
    R = sum(rows)
    rng = np.random.default_rng(98)
    panels, maps = [], []
    off = 0
    for i, (B, D) in enumerate(shapes):
        N = B * D
        tpp = (D + 15) // 16
        bb, jj = np.divmod(np.arange(N), D)
        maps.append(off + (bb * tpp + jj // 16) * 16 + jj % 16)         # row of coordinate n in the padded numbering
        off += rows[i]
        gs = [t_((rng.standard_normal((B, D)) * 0.5).astype(np.float32)) for _ in range(T)]
        ms = [t_((rng.standard_normal((B, D)) * 0.1).astype(np.float32)) for _ in range(T)] if fc else [None] * T
        vs = [t_((rng.random((B, D)) * 0.1 + 0.01).astype(np.float32)) for _ in range(T)] if fc else [None] * T
        sts = []
        for k in range(T):
            state = random_state(cfg, N, 300 + 10 * i + k)
            sts.append(eng.state_pack(*[t_(a) for hc in state for a in hc], B, D))
        g_final = t_((rng.standard_normal(N) * 0.5).astype(np.float32))
        dxs, acc = [None] * T, g_final.clone()
        for k in reversed(range(T)):
            dxs[k] = acc
            acc = acc + gs[k].reshape(N)
        panels.append(dict(B=B, D=D, gs=gs, ms=ms, vs=vs, sts=sts, dxs=dxs, g_final=g_final))
    cin_rows = (rng.standard_normal((4, R, 20)) * 0.3).astype(np.float32)
    live = np.zeros(R, bool)
    for mp in maps:
        live[mp] = True
    cin_rows[:, ~live] = 0.0
    # reference: per panel, per step, dense [N] rows
    b1, b2 = float(np.float32(spec.beta1)), float(np.float32(spec.beta2))
    refA, refB = np.zeros((T, R, KA), np.float32), np.zeros((T, R, KB), np.float32)
    refC = np.zeros((4, R, 20), np.float32)
    for pn, mp in zip(panels, maps):
        B, D = pn["B"], pn["D"]
        N = B * D
        cin = t_(np.ascontiguousarray(cin_rows[:, mp]))
        for k in reversed(range(T)):
            At, Bt = eng.zeros(N, KA), eng.zeros(N, KB)
            cout = eng.zeros(4, N, 20)
            io = dict(g=pn["gs"][k], dx_next=pn["dxs"][k], st_prev=pn["sts"][k], carry_in=cin, carry_out=cout,
                      m=pn["ms"][k], v=pn["vs"][k], a_stride=KA, b_stride=KB, act1=At[:, 0:K1], act2=At[:, K1:K1 + 40],
                      h2=At[:, K1 + 40:K1 + 60], dz1=Bt[:, 0:80], dz2=Bt[:, 80:160], dd=Bt[:, 160:161])
            if fc:
                io.update(feats=At[:, K1 + 60:K1 + 62], du=Bt[:, 161:181])
            with lib_option(_abi.OPT_BWD_KERNEL, 2):                     # the generic kernel
                eng.bwd_step(spec, wdev, io, b1 ** (step0 + k), b2 ** (step0 + k), B, D)
            a = eng.to_numpy(At)
            a[:, KA - 1] = 1.0
            refA[k, mp], refB[k, mp] = a, eng.to_numpy(Bt)
            cin = cout
        refC[:, mp] = eng.to_numpy(cin)
    for dx_mode in ("g_final", "table"):
        A1, B1 = eng.empty(T, R, KA), eng.empty(T, R, KB)
        A1.fill_(7.0); B1.fill_(7.0)                                     # every row is written, the padding rows as zeros
        c1 = eng.zeros(4, R, 20)
        fused_panels = [dict(pn, dxs=None) if dx_mode == "g_final" else dict(pn, g_final=None) for pn in panels]
        eng.bwd_unroll(spec, wfused, fused_panels, T, step0, A1, B1, carry_in=t_(cin_rows), carry_out=c1)
        A1n, B1n, c1n = eng.to_numpy(A1), eng.to_numpy(B1), eng.to_numpy(c1)
        for k in range(T):
            for got, ref, what in ((A1n[k], refA[k], "A"), (B1n[k], refB[k], "Bm")):
                tol = 2e-5 * np.maximum(np.abs(ref).max(axis=0, keepdims=True), 1e-30) + 1e-9
                assert (np.abs(got - ref) <= tol).all(), (dx_mode, what, k, float(np.abs(got - ref).max()))
            assert not A1n[k][~live].any() and not B1n[k][~live].any()
        for a in range(4):
            tol = 2e-5 * np.maximum(np.abs(refC[a]).max(), 1e-30) + 1e-9
            assert (np.abs(c1n[a][live] - refC[a][live]) <= tol).all(), (dx_mode, "carry", a)


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [16, 64])
@pytest.mark.parametrize("name", ["dm_logsign", "rnnprop"])
def test_planned_mlp_unroll_equals_step_path(name, batch, monkeypatch):
    """The recorded unroll of problems.mnist three ways: ONE persistent launch that also records the history
    (l2o_mlp_unroll_record, the default where the fused MLP unroll applies; batch 64 = its FAST instantiation), the
    step-granular PLAN (history buffers chained through the steps, ctypes arguments prepared once;
    L2O_NO_MLP_UNROLL_RECORD=1) and the plain step-by-step path with cloned history (+ L2O_NO_STEP_PLAN=1): same costs,
    same iterates and the same meta-gradient for two consecutive training steps (the second re-uses the buffers)."""
    eng = _engine.HipEngine()
    old = _engine._default_engine
    _engine.set_default_engine(eng)
    try:
        cfg = ORACLE_CFGS[name]
        rn = cfg.kind == "rnnprop"
        params = make_params(cfg, seed=83, trained_like=True)
        data = problems.synthetic_mnist(200, seed=4)
        T = 3
        idx = np.random.default_rng(5).integers(0, 200, size=(64, batch))

        def sampler(n_evals, b, n_data, _state={"k": 0}):
            k = _state["k"]
            _state["k"] = (k + n_evals) % 32
            return idx[k:k + n_evals, :b]

        got = {}
        for mode in ("fused", "plan", "steps"):
            monkeypatch.delenv("L2O_NO_STEP_PLAN", raising=False)
            monkeypatch.delenv("L2O_NO_MLP_UNROLL_RECORD", raising=False)
            monkeypatch.setenv("L2O_MLP_UNROLL_RECORD_GENERIC", "1")   # (minibatch 16: the kernel's generic loops -- not the default there)
            if mode != "fused":
                monkeypatch.setenv("L2O_NO_MLP_UNROLL_RECORD", "1")
            if mode == "steps":
                monkeypatch.setenv("L2O_NO_STEP_PLAN", "1")
            st = {"k": 0}
            problem = problems.mnist(layers=(20,), batch_size=batch, data=data,
                                     sampler=lambda n, b, nd, _s=st: sampler(n, b, nd, _s))
            meta.set_random_seed(11)
            if rn:
                opt = meta_rnnprop_eval.MetaOptimizer(0.95, 0.95, **_net_config(cfg, params, key="rp"))
                out = opt.meta_minimize(problem, T, learning_rate=1e-3)
                ms, step_ph = out[0], out[3]
            else:
                opt = meta.MetaOptimizer(**_net_config(cfg, params))
                ms, step_ph = opt.meta_minimize(problem, T, learning_rate=1e-3), None
            graph = opt.graph
            caps = []
            orig = graph._adam_apply
            graph._adam_apply = lambda grads, lr, **kw: (caps.append(grads), orig(grads, lr, **kw))[1]
            costs = []
            with Session() as sess:
                sess.run(ms.reset)
                for i in range(2):
                    costs.append(sess.run([ms.fx, ms.update, ms.step], feed_dict={step_ph: 1 + i * T} if rn else {})[0])
                xs = [v.eval() for v in graph.x]
            assert ("_step_plan" in graph.__dict__) == (mode == "plan")
            if mode == "fused":
                assert graph.last_path == "mlp_unroll" and "_mlp_record_plan" in graph.__dict__
            else:
                assert graph.last_path == "steps"
            got[mode] = (costs, xs, caps)
        key = "rp" if rn else "cw"
        for mode in ("fused", "plan"):
            for a, b in zip(got[mode][0], got["steps"][0]):
                assert rel_err(a, b) < 2e-6, mode
            for a, b in zip(got[mode][1], got["steps"][1]):
                assert max_abs(a, b) < 2e-6, mode
            for ga, gb in zip(got[mode][2], got["steps"][2]):
                for k, gref in gb[key].items():
                    scale = max(float(np.abs(gref).max()), 1e-12)
                    assert float(np.abs(np.asarray(ga[key][k]) - np.asarray(gref)).max()) / scale < 1e-4, (mode, k)
    finally:
        _engine.set_default_engine(old)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["dm", "dm_logsign", "rnnprop"])
def test_device_weight_pack_equals_host_pack(name):
    """l2o_wpack_device (weights that live on the device) == l2o_wpack_host, bit for bit."""
    from open_l2o_amd._engine import HipEngine, pack_weights_host
    from helpers import spec_of
    eng = HipEngine()
    cfg = ORACLE_CFGS[name]
    spec = spec_of(cfg)
    params = make_params(cfg, seed=123, trained_like=True)
    host = pack_weights_host(eng.lib, spec, params)
    names = {"w_gates1": ("lstm_1", "w_gates"), "b_gates1": ("lstm_1", "b_gates"), "w_gates2": ("lstm_2", "w_gates"),
             "b_gates2": ("lstm_2", "b_gates"), "w_lin": ("linear", "w"), "b_lin": ("linear", "b"),
             "w_fc": ("input_projection", "w"), "b_fc": ("input_projection", "b")}
    wdev = {k: eng.tensor(params[m][v]) for k, (m, v) in names.items() if m in params}
    out = eng.tensor(np.full(host.size, 7.0, np.float32))           # stale contents must be overwritten
    eng.pack_weights_device(spec, wdev, out)
    got = eng.to_numpy(out)
    assert np.array_equal(got.view(np.uint32), host.view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["dm", "rnnprop"])
def test_device_meta_step_equals_host_meta_step(name, monkeypatch):
    """Three meta_minimize steps with Adam + re-pack on the device (l2o_adam_step, l2o_wpack_device) leave the
    same weights, losses and packed copy as the NumPy meta-step (L2O_HOST_ADAM=1); the host dict is refreshed
    lazily, and a host-side assign() after device steps is honoured."""
    from open_l2o_amd import _engine
    eng = _engine.HipEngine()
    old = _engine._default_engine
    _engine.set_default_engine(eng)
    try:
        cfg = ORACLE_CFGS[name]
        rn = cfg.kind == "rnnprop"
        params = make_params(cfg, seed=77, trained_like=True)
        B, D, T = 4, 32, 5
        prob, x0, _ = make_problem("quadratic", B, D, seed=78)
        res = {}
        for mode in ("device", "host"):
            if mode == "host":
                monkeypatch.setenv("L2O_HOST_ADAM", "1")
            else:
                monkeypatch.delenv("L2O_HOST_ADAM", raising=False)
            problem = problems.quadratic(B, D, data={"w": prob.w, "y": prob.y, "x": x0})
            if rn:
                opt = meta_rnnprop_eval.MetaOptimizer(0.95, 0.95, **_net_config(cfg, params, key="rp"))
                out = opt.meta_minimize(problem, T, learning_rate=1e-2)
                ms, step_ph = out[0], out[3]
            else:
                opt = meta.MetaOptimizer(**_net_config(cfg, params))
                ms, step_ph = opt.meta_minimize(problem, T, learning_rate=1e-2), None
            net = opt.graph.nets["rp" if rn else "cw"]
            costs = []
            with Session() as sess:
                sess.run(ms.reset)
                for i in range(3):
                    feed = {step_ph: 1 + i * T} if rn else {}
                    costs.append(sess.run([ms.fx, ms.update, ms.step], feed_dict=feed)[0])
                assert net._host_stale == (mode == "device")
                w = {m: {v: a.copy() for v, a in d.items()} for m, d in net.variables.items()}
                assert not net._host_stale
                packed = eng.to_numpy(net.wpack(eng)).copy()
                # a host-side write after device steps: picked up by the next unroll
                net.assign("linear", "b", np.array([0.25], np.float32))
                feed = {step_ph: 1 + 3 * T} if rn else {}
                costs.append(sess.run([ms.fx, ms.update, ms.step], feed_dict=feed)[0])
                w2 = {m: {v: a.copy() for v, a in d.items()} for m, d in net.variables.items()}
            res[mode] = (costs, w, packed, w2)
        for a, b in zip(res["device"][0], res["host"][0]):
            assert rel_err(a, b) < 1e-6
        for key in (1, 3):
            for m, d in res["host"][key].items():
                for v, a in d.items():
                    assert max_abs(res["device"][key][m][v], a) <= 1e-7 * max(1.0, float(np.abs(a).max())), (m, v)
        assert not np.array_equal(res["host"][1]["lstm_1"]["w_gates"], params["lstm_1"]["w_gates"])
        # the packed copy the kernels read is the pack of the weights the host sees
        from open_l2o_amd._engine import pack_weights_host
        from helpers import spec_of
        assert np.array_equal(pack_weights_host(eng.lib, spec_of(cfg), res["device"][1]).view(np.uint32),
                              res["device"][2].view(np.uint32))
    finally:
        _engine.set_default_engine(old)


def test_device_meta_step_host_logic_on_cpu(monkeypatch):
    """The host logic of the device meta-step (gradient layout = flat weight buffer, in-place update, lazy
    refresh of the .l2l dict, assign() after device steps) on the oracle-backed engine: same weights as the
    NumPy meta-step, bit for bit (the engine's adam_step is the same NumPy expression)."""
    from oracle_engine import OracleEngine
    cfg = ORACLE_CFGS["rnnprop"]
    params = make_params(cfg, seed=61, trained_like=True)
    B, D, T = 3, 10, 4
    prob, x0, _ = make_problem("quadratic", B, D, seed=62)
    res = {}
    old = _engine._default_engine
    try:
        for mode in ("device", "host"):
            eng = OracleEngine()
            _engine.set_default_engine(eng)
            if mode == "host":
                monkeypatch.setenv("L2O_HOST_ADAM", "1")
            else:
                monkeypatch.delenv("L2O_HOST_ADAM", raising=False)
            opt = meta_rnnprop_eval.MetaOptimizer(0.95, 0.95, **_net_config(cfg, params, key="rp"))
            out = opt.meta_minimize(problems.quadratic(B, D, data={"w": prob.w, "y": prob.y, "x": x0}), T,
                                    learning_rate=1e-2)
            ms, step_ph = out[0], out[3]
            net = opt.graph.nets["rp"]
            with Session() as sess:
                sess.run(ms.reset)
                for i in range(2):
                    sess.run([ms.fx, ms.update, ms.step], feed_dict={step_ph: 1 + i * T})
                assert ("adam_step" in eng.calls) == (mode == "device")
                assert net._host_stale == (mode == "device")
                w = {m: {v: a.copy() for v, a in d.items()} for m, d in net.variables.items()}
                assert not net._host_stale
                net.assign("linear", "b", np.array([0.5], np.float32))
                sess.run([ms.fx, ms.update, ms.step], feed_dict={step_ph: 1 + 2 * T})
                w2 = {m: {v: a.copy() for v, a in d.items()} for m, d in net.variables.items()}
            res[mode] = (w, w2)
    finally:
        _engine.set_default_engine(old)
    for k in (0, 1):
        for m, d in res["host"][k].items():
            for v, a in d.items():
                assert np.array_equal(res["device"][k][m][v], a), (m, v)
    assert not np.array_equal(res["host"][0]["lstm_2"]["w_gates"], params["lstm_2"]["w_gates"])
    assert abs(float(res["host"][1]["linear"]["b"][0]) - 0.5) < 0.05      # the assigned value, moved by one Adam step
