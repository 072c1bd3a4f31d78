"""networks.KernelDeepLSTM without a GPU: the class (variables, .l2l round trip, refusals, the eager call, the [K, N] indexing)
and the host wiring of the unroll graph (step path, recording, BPTT, host Adam) on the oracle engine, whose klstm_step /
klstm_bwd_step are the float32 torch restatement of kernel_lstm_reference.py."""
import numpy as np
import pytest
import torch

import imagenet_harness as H
import kernel_lstm_reference as KR
from open_l2o_amd import _abi, _graph_core, meta, meta_dm_train, networks, problems
from open_l2o_amd.session import Session

NET = H.NETS["mnist_conv"]
LOGSIGN = {"preprocess_name": "LogAndSign", "preprocess_options": {"k": 5}, "scale": 0.01}
NAMES = ["conv_layer1/weights1", "conv_layer2/weights1"]


def config(l3=(20, 20), l5=(8, 12)):
    return {"k3": {"net": "KernelDeepLSTM", "net_options": dict(kernel_shape=(3, 3), layers=l3, **LOGSIGN)},
            "k5": {"net": "KernelDeepLSTM", "net_options": dict(kernel_shape=(5, 5), layers=l5, **LOGSIGN)},
            "cw": {"net": "CoordinateWiseDeepLSTM", "net_options": dict(layers=(20, 20), **LOGSIGN)}}


def assignments(batch_norm):
    rest = [n for n in NET.R.names(batch_norm) if n not in NAMES]
    return [("k3", NAMES[:1]), ("k5", NAMES[1:]), ("cw", rest)]


def engine():
    """The oracle engine with the kernel net's two entry points and mnist_conv's evaluation, all float32 torch."""
    fg = type(H.oracle_engine(NET)).__dict__[NET.fg]
    return type("KernelConvOracleEngine", (KR.KernelOracleEngine,), {NET.fg: fg})()


# 1. the class
def test_variable_shapes_defaults_and_l2l_round_trip(tmp_path):
    networks.set_random_seed(3)
    net = networks.KernelDeepLSTM((2, 3), (8, 12), preprocess_name="LogAndSign", preprocess_options={"k": 5}, scale=0.1)
    v = net.variables
    assert list(v) == ["lstm_1", "lstm_2", "linear"]
    assert {m: {n: a.shape for n, a in d.items()} for m, d in v.items()} == {
        "lstm_1": {"w_gates": (12 + 8, 32), "b_gates": (32,)}, "lstm_2": {"w_gates": (8 + 12, 48), "b_gates": (48,)},
        "linear": {"w": (12, 6), "b": (6,)}}
    assert not v["lstm_1"]["b_gates"].any() and not v["linear"]["b"].any()                # zeros
    assert np.abs(v["lstm_1"]["w_gates"]).max() <= 2.0 / np.sqrt(20) and v["lstm_1"]["w_gates"].std() > 0.1 / np.sqrt(20)
    ident = networks.KernelDeepLSTM((2, 3), (20,))
    assert ident.variables["lstm_1"]["w_gates"].shape == (6 + 20, 80) and ident.in_dim == 6
    path = str(tmp_path / "k.l2l")
    saved = networks.save(net, filename=path)
    back = networks.factory("KernelDeepLSTM", dict(kernel_shape=(2, 3), layers=(8, 12), preprocess_name="LogAndSign",
                                                   preprocess_options={"k": 5}, scale=0.1), net_path=path)
    for m in saved:
        for n in saved[m]:
            assert np.array_equal(back.variables[m][n], v[m][n])
    version = back._wversion
    back.assign("linear", "b", np.arange(6))
    assert back.variables["linear"]["b"].tolist() == list(range(6)) and back._wversion != version


@pytest.mark.parametrize("kwargs", [
    dict(kernel_shape=(8, 3), layers=(20, 20)), dict(kernel_shape=(0, 3), layers=(20,)), dict(kernel_shape=(3,), layers=(20,)),
    dict(kernel_shape=(3, 3), layers=()), dict(kernel_shape=(3, 3), layers=(20, 20, 20)),
    dict(kernel_shape=(3, 3), layers=(18,)), dict(kernel_shape=(3, 3), layers=(36,)), dict(kernel_shape=(3, 3), layers=(0,)),
    dict(kernel_shape=(3, 3), layers=(20,), preprocess_name="fc", preprocess_options={"dim": 20})])
def test_range_refusals(kwargs):
    with pytest.raises(NotImplementedError):
        networks.KernelDeepLSTM(**kwargs)


def test_reference_defaults_are_inside_the_range():
    for layers in ((20, 20), (20,), (4,), (32, 32)):
        for shape in ((1, 1), (7, 7), (3, 3)):
            networks.KernelDeepLSTM(shape, layers)


# 2. the eager call and the [K, N] indexing
def test_eager_call_indexing_and_untouched_arguments():
    """A non-square patch: row j = a * kh + b of the [K, N] matrix is patch position (a, b), column n = ci * c_out + co the
    filter; the restatement below goes through the reference's transpose / reshape / transpose-back instead."""
    eng = engine()
    networks.set_random_seed(5)
    net = networks.KernelDeepLSTM((2, 3), (8, 12), preprocess_name="identity", scale=0.5, tanh_output=True)
    rng = np.random.default_rng(6)
    g = rng.normal(size=(2, 3, 7, 3)).astype(np.float32)
    gt = torch.from_numpy(g.copy())
    state = net.initial_state_for_inputs(gt, engine=eng)
    assert state.N == 21 and state.buf.numel() == 2 * 21 * 20 and not state.buf.any()
    d1, s1 = net(gt, state)
    assert np.array_equal(gt.numpy(), g) and not state.buf.any()                       # the arguments are untouched
    d2, s2 = net(gt, s1)
    assert d1.shape == gt.shape and s2.buf.data_ptr() != s1.buf.data_ptr()
    # the reference's route: [kw, kh, ci, co] -> transpose (2, 3, 0, 1) -> [N, kw * kh] -> net -> [N, K] -> transpose -> reshape
    cfg, p = KR.cfg_of(net), KR.as_torch(net.variables, torch.float32)
    rows = torch.from_numpy(g).permute(2, 3, 0, 1).reshape(21, 6)
    want1, st = KR.step(cfg, p, rows.t(), KR.zero_state(cfg, 21, torch.float32))
    want2, st = KR.step(cfg, p, rows.t(), st)
    assert torch.allclose(d1, want1.reshape(2, 3, 7, 3), rtol=1e-6, atol=1e-7)
    assert torch.allclose(d2, want2.reshape(2, 3, 7, 3), rtol=1e-6, atol=1e-7)
    assert not torch.allclose(d1, want1.reshape(3, 2, 7, 3).transpose(0, 1).reshape(2, 3, 7, 3), atol=1e-3)   # a kw + b is not it
    (h1, c1), (h2, c2) = s2.unpack()
    assert h1.shape == (21, 8) and c2.shape == (21, 12) and torch.allclose(h2, st[1][0], atol=1e-6)
    with pytest.raises(ValueError, match="kernel_shape"):
        net(torch.zeros(3, 2, 7, 3), state)
    with pytest.raises(ValueError, match="kernel_shape"):
        net.initial_state_for_inputs(torch.zeros(6, 21), engine=eng)


# 3. the graph
def _problem(batch_norm, idx):
    return problems.mnist_conv(batch_norm=batch_norm, batch_size=idx.shape[1], data=problems.synthetic_mnist(64),
                               sampler=H.sampler(idx))


def test_graph_refusals():
    idx = np.zeros((8, 4), int)
    with H.as_default(engine()):
        with pytest.raises(NotImplementedError, match="second_derivatives"):
            meta.MetaOptimizer(**config()).meta_minimize(_problem(False, idx), 2, net_assignments=assignments(False),
                                                         second_derivatives=True)
        with pytest.raises(NotImplementedError, match="imitation"):
            meta_dm_train.MetaOptimizer(1, **config()).meta_minimize(_problem(False, idx), 2, net_assignments=assignments(False))
        # a variable that is no filter of the net's kernel_shape
        bad = [("k3", NAMES[1:]), ("k5", NAMES[:1]), assignments(False)[2]]
        with pytest.raises(ValueError, match="kernel_shape"):
            meta.MetaOptimizer(**config()).meta_loss(_problem(False, idx), 2, net_assignments=bad)
        # a sharded graph
        _graph_core.emulate_world(0, 2)
        try:
            with pytest.raises(NotImplementedError, match="sharded"):
                meta.MetaOptimizer(k={"net": "KernelDeepLSTM", "net_options": dict(kernel_shape=(1, 1), layers=(20,))}) \
                    .meta_loss(problems.quadratic(batch_size=4, num_dims=3), 2)
        finally:
            _graph_core.emulate_world()


def test_meta_loss_matches_the_restated_unroll():
    """meta_loss on the step path, two chained unrolls of T steps, every net on its variables: the losses and x_T of the
    float32 restatement over the same evaluations (the oracle engine IS float32 torch: the comparison checks the wiring)."""
    T, batch = 3, 4
    idx = np.random.default_rng(1).integers(0, 64, size=(2 * (T + 1), batch))
    eng = engine()
    with H.as_default(eng):
        meta.set_random_seed(2)
        opt = meta.MetaOptimizer(**config())
        ml = opt.meta_loss(_problem(False, idx), T, net_assignments=assignments(False))
        with Session() as sess:
            sess.run(ml.reset)
            v0 = [v.eval() for v in opt.graph.x]
            fx1 = opt.graph.execute({}, True)["fx_array"]
            res = opt.graph.execute({}, True)
    assert opt.graph.last_path == "steps" and eng.calls.count("klstm_step") == 2 * 2 * T
    data = problems.synthetic_mnist(64)
    ref = NET.ref(data["images"], data["labels"], False)
    nets = {k: (KR.cfg_of(n) if k != "cw" else KR.cw_cfg((20, 20), 5, 0.01), n.variables) for k, n in opt._nets.items()}
    names = NET.R.names(False)
    assign = ["k3" if n == NAMES[0] else "k5" if n == NAMES[1] else "cw" for n in names]
    # the second unroll starts from the first one's state: one restated unroll of the 2T steps would evaluate x_T once, the
    # graph evaluates it at the end of unroll 1 and again (next minibatch) at the start of unroll 2
    rows = list(range(T)) + list(range(T + 1, 2 * T + 2))
    fx_r, x_r = KR.graph_unroll(nets, assign, lambda xs, t: ref.fg(xs, idx[rows[t]]), v0, 2 * T, dtype=torch.float32)
    assert np.allclose(fx1[:T], fx_r[:T], rtol=1e-5)
    assert np.allclose(res["fx_array"], fx_r[T:], rtol=1e-5)
    for got, want in zip(res["x"], x_r):
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-6)


def test_meta_minimize_step_moves_all_three_nets():
    T, batch = 3, 4
    idx = np.random.default_rng(3).integers(0, 64, size=(T + 1, batch))
    eng = engine()
    with H.as_default(eng):
        meta.set_random_seed(4)
        opt = meta.MetaOptimizer(**config())
        ms = opt.meta_minimize(_problem(False, idx), T, learning_rate=1e-3, net_assignments=assignments(False))
        w0 = {k: {m: {v: np.array(a) for v, a in d.items()} for m, d in n.variables.items()} for k, n in opt._nets.items()}
        with Session() as sess:
            sess.run(ms.reset)
            cost = sess.run([ms.fx, ms.update, ms.step])[0]
    assert np.isfinite(cost) and opt.graph.last_path == "steps"
    assert eng.calls.count("klstm_step") == 2 * T and eng.calls.count("klstm_bwd_step") == 2 * T
    assert "lstm_step_multi" in eng.calls or "lstm_step" in eng.calls
    for k, n in opt._nets.items():
        moved = [not np.array_equal(w0[k][m][v], np.asarray(n.variables[m][v])) for m in w0[k] for v in w0[k][m]]
        assert all(moved), (k, moved)
    # the kernel nets keep out of the coordinate-wise machinery
    g = opt.graph
    states = [s.state for s in g.slots]
    assert not g._plan_ok(g.slots, states, len(g.x)) and not g._fused_unroll_ok("mlp", g.slots, states)
    assert all(not g._device_adam(n) for k, n in opt._nets.items() if k != "cw")


def test_meta_gradient_of_the_oracle_engine_and_the_bound_sees_a_missing_term():
    """The BPTT's host logic (suffix sums, carries, the blocked act^T dz products, accumulation over steps) against float64
    autograd of the restated unroll, with the project's standing criterion: every block within 5e-4 of its largest float64
    entry.  And the bound can see a missing term: with the dd operand of ONE step of the 3x3 net zeroed in the reference, its
    linear/w block moves by more than the bound (printed below)."""
    T, batch = 3, 4
    idx = np.random.default_rng(5).integers(0, 64, size=(T + 1, batch))
    eng = engine()
    captured = {}
    with H.as_default(eng):
        meta.set_random_seed(6)
        opt = meta.MetaOptimizer(**config())
        ms = opt.meta_minimize(_problem(False, idx), T, learning_rate=1e-3, net_assignments=assignments(False))
        with Session() as sess:
            sess.run(ms.reset)
            g = opt.graph
            v0 = [v.eval() for v in g.x]
            w0 = {k: {m: {v: np.array(a) for v, a in d.items()} for m, d in n.variables.items()} for k, n in opt._nets.items()}
            g._adam_apply = lambda grads, lr, **kw: captured.update(grads)
            g.train_step({}, True, 1e-3)
    data = problems.synthetic_mnist(64)
    ref = NET.ref(data["images"], data["labels"], False)
    nets = {k: (KR.cfg_of(n) if k != "cw" else KR.cw_cfg((20, 20), 5, 0.01), w0[k]) for k, n in opt._nets.items()}
    names = NET.R.names(False)
    assign = ["k3" if n == NAMES[0] else "k5" if n == NAMES[1] else "cw" for n in names]
    fg = lambda xs, t: ref.fg(xs, idx[t])                                   # noqa: E731
    _, _, want = KR.graph_unroll(nets, assign, fg, v0, T, want_grad=True)
    for key in want:
        for m in want[key]:
            for v, w in want[key][m].items():
                got = np.asarray(captured[key][(m, v)], np.float64).reshape(w.shape)
                err = np.abs(got - w).max() / np.abs(w).max()
                print(key, m, v, "err %.3e" % err)
                assert err < 5e-4, (key, m, v, err)
    _, _, cut = KR.graph_unroll(nets, assign, fg, v0, T, want_grad=True, drop_dd=("k3", T - 1))
    w = want["k3"]["linear"]["w"]
    moved = np.abs(cut["k3"]["linear"]["w"] - w).max() / np.abs(w).max()
    print("k3 linear/w with the dd of the last step zeroed: moved by %.3e" % moved)
    assert moved > 5e-4


# 4. the library (no launch: refusals come before one)
def test_library_symbols_header_and_refusals():
    import ctypes as C
    import __graft_entry__  # noqa: F401
    lib = _abi.lib()
    assert lib.l2o_abi_version() == 15
    assert _abi.source_build_id() == _abi.build_id()

    def net(kw=3, kh=3, layers=(20, 20), pre=_abi.PRE_LOGSIGN, flags=0):
        c = _abi.KlstmNet()
        c.kw, c.kh, c.n_layers, c.preprocess, c.flags = kw, kh, len(layers), pre, flags
        for l, h in enumerate(layers[:2]):
            c.hidden[l] = h
        return c

    ok = lambda c: bool(lib.l2o_klstm_supported(C.byref(c)))                                  # noqa: E731
    assert ok(net()) and ok(net(1, 1, (4,))) and ok(net(7, 7, (32, 32))) and ok(net(2, 3, (20,), _abi.PRE_IDENTITY))
    for bad in (net(8, 3), net(3, 0), net(layers=()), net(layers=(20, 20, 20)), net(layers=(18,)), net(layers=(36,)),
                net(pre=_abi.PRE_FC_ELU), net(flags=1)):
        assert not ok(bad) and lib.l2o_klstm_state_floats(C.byref(bad), 16) == 0
        assert lib.l2o_klstm_step(C.byref(bad), None, None, None, None, 16, None) == _abi.L2O_ERR_UNSUPPORTED
        assert lib.l2o_klstm_bwd_step(C.byref(bad), None, 16, None) == _abi.L2O_ERR_UNSUPPORTED
    assert lib.l2o_klstm_state_floats(C.byref(net()), 15) == 2 * 15 * 40 and lib.l2o_klstm_state_floats(C.byref(net()), 0) == 0
    assert lib.l2o_klstm_step(C.byref(net()), None, None, None, None, 0, None) == _abi.L2O_ERR_UNSUPPORTED    # N >= 1
    assert lib.l2o_klstm_step(C.byref(net()), None, None, None, None, 16, None) == _abi.L2O_ERR_ARG           # NULL weights
