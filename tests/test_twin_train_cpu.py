"""open_l2o_amd.twin's meta-training on the CPU: the closed-form seed the kernels implement against autograd of the reference's
graph (twin_train_reference.py), the host logic of train_batch / fit on TorchTwinTrainEngine against the oracle's do_fit loop,
get_index's edge cases, the driver end to end, and the library's refusals before any launch."""
import ctypes as C
import importlib.util
import json
import os
import re
import shutil

import numpy as np
import pytest
import torch

import twin_reference as TR
import twin_train_reference as TT
from open_l2o_amd import _abi, twin
from test_twin_cpu import GOLDEN, as_default, load_driver, make_data

HERE = os.path.dirname(os.path.abspath(__file__))


def load_trainer_script():
    spec = importlib.util.spec_from_file_location("train_twin", os.path.join(HERE, "..", "scripts", "train_twin.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_case(kind, n, dim, H=6, seed=0):
    prob = twin.problem(kind, make_data(kind, n, dim, 100 + seed), dim)
    mn, mx = twin.Optimizer(H, seed=1000 + seed), twin.Optimizer(H + 1, seed=2000 + seed)
    theta0, states = twin.draw_start(prob, mn, mx, seed=3000 + seed)
    return prob, mn, mx, theta0, states


# optim_it = 20: three sign iterations.  Segments inside the sign phase, across its end and past it.
@pytest.mark.parametrize("kind,dim", [(2, 1), (3, 1), (4, 3)])
@pytest.mark.parametrize("iter0,n_iter", [(1, 2), (1, 6), (3, 4), (5, 4)])
def test_closed_form_seed_is_autograd(kind, dim, iter0, n_iter):
    prob, mn, mx, theta0, states = make_case(kind, 4, dim)
    n_sign, lr = twin.schedule(20)
    m = np.float32([1.0, 0.0, 2.0, 1.0])
    r = TT.segment_grad(torch.float64, kind, dim, prob.data, mn.params, mx.params, lr, n_sign, theta0, states, iter0, n_iter,
                        1.0, 0.5, batch_size=7, inst_weight=m)
    want = TT.closed_form_seed(kind, prob.data, r["curve"], iter0, n_iter, n_sign, 0.5, 7, m)
    scale = max(np.abs(r["g_delta"]).max(), 1e-300)
    print("largest |g_delta| %.3e, closed form off by %.3e" % (scale, np.abs(want - r["g_delta"]).max()))
    if iter0 + n_iter - 1 <= n_sign:
        assert not r["g_delta"].any() and not want.any()
        assert all(not g.any() for gs in r["grads"] for g in gs.values())
    else:
        assert np.abs(want - r["g_delta"]).max() <= 1e-12 * scale
        assert not r["g_delta"][:, :max(n_sign - iter0 + 1, 0)].any()
        assert all(np.abs(gs["output.bias"]).max() > 0 for gs in r["grads"][1:])
    # the host's loss is the graph's
    with as_default(TT.TorchTwinTrainEngine()):
        res = twin.meta_gradient(prob, mn, mx, 20, iter0, n_iter, theta0, states, rescale=1.0, out_mul=0.5, batch_size=7,
                                 inst_weight=m)
    assert res.loss == pytest.approx(r["loss"], rel=1e-4, abs=1e-6)
    assert set(res.grads[0]) == set(twin.PARAM_NAMES) and res.curve.shape == (4, n_iter + 1, 2 * dim)


@pytest.mark.parametrize("kind,n,dim,CL", [(3, 6, 1, True), (4, 3, 5, False)])
def test_train_batch_is_the_oracles_loop(kind, n, dim, CL):
    prob, mn, mx, theta0, states = make_case(kind, n, dim, seed=1)
    before = [dict(mn.params), dict(mx.params)]
    want = TT.train_loop(kind, dim, prob.data, mn.params, mx.params, 1e-3, 22, 2, theta0, states, 1.0, CL=CL, epoch_index=30)
    trainer, log = twin.Trainer(mn, mx, lr=1e-3), []
    with as_default(TT.TorchTwinTrainEngine()):
        dv, du, info = twin.train_batch(prob, trainer, 22, 2, rescale=1.0, theta0=theta0, states=states, curriculum=CL,
                                        epoch_index=30, log=log)
    assert trainer.step_counts() == want["steps"] == (5, 5)                  # 22 iterations: five whole segments of 4
    assert [e["iter0"] for e in log] == [1, 5, 9, 13, 17]
    for e, w in zip(log, want["weights"]):
        assert (e["inst_weight"] is None and w is None) if not CL else np.array_equal(e["inst_weight"], w)
    if CL:
        assert all(e["inst_weight"].sum() == int(0.5 * n) for e in log)      # sche_ratio(30) = 0.5
    for opt, old, ref in zip((mn, mx), before, want["params"]):
        for k in twin.PARAM_NAMES:
            assert np.array_equal(opt.params[k], ref[k]), k
            assert not np.array_equal(opt.params[k], old[k]), k
    assert np.array_equal(info, want["curve_info"]) and info.shape == (n, 22, 2 * dim)
    assert np.array_equal(dv, want["distances"][0]) and np.array_equal(du, want["distances"][1])


def test_a_wholly_sign_segment_still_counts_as_an_adam_step():
    prob, mn, mx, theta0, states = make_case(3, 3, 1, seed=2)
    trainer, log = twin.Trainer(mn, mx, lr=1e-3), []
    before = {k: v.copy() for k, v in mn.params.items()}
    with as_default(TT.TorchTwinTrainEngine()):
        twin.train_batch(prob, trainer, 20, 1, theta0=theta0, states=states, log=log)     # segment 1..2 is all sign (n_sign 3)
        first = twin.meta_gradient(prob, twin.Optimizer(6, seed=1002), twin.Optimizer(7, seed=2002), 20, 1, 2, theta0, states)
    assert all(not g.any() for gs in first.grads for g in gs.values())
    assert trainer.step_counts() == (10, 10) and all(e["stepped"] for e in log)
    want = TT.train_loop(3, 1, prob.data, before, twin.Optimizer(7, seed=2002).params, 1e-3, 20, 1, theta0, states, 1e-4)
    assert want["steps"] == (10, 10)
    assert all(np.array_equal(mn.params[k], want["params"][0][k]) for k in twin.PARAM_NAMES)


def test_get_index_edge_cases():
    data = np.float32([[1.0, 1.0], [1.0, 2.0], [1.0, 1.0], [0.5, 1.0]])
    curve = np.zeros((4, 30, 2))
    curve[:, :, 0] = np.float64([0.5, 0.5, 0.5, 1.0])[:, None]                # sin(a pi u) = 1 everywhere: scores 1, 4, 1, 1 per column
    for fn in (twin.get_index, TT.get_index):
        # ties keep their order under the stable descending sort: [1, 0, 2, 3]; the last k
        assert fn(curve, 10, 5, data, 0.5) == [2, 3]
        assert fn(curve, 10, 5, data, 0.75) == [0, 2, 3]
        assert fn(curve, 10, 5, data, 0.2) == [1, 0, 2, 3]                    # k = 0: [-0:] is the whole list
        assert fn(curve, 10, 5, data, 1) == [1, 0, 2, 3]
    # flag = iteration // 10, a literal 10: with unroll_unit 2 the slice is 0 : 4 flag - 1, and 0 : -1 while flag = 0
    c2 = np.zeros((2, 12, 2))
    d2 = np.float32([[1.0, 1.0], [1.0, 1.0]])
    c2[0, 3, 0] = 0.5                                                         # column 3: outside 0:3 (flag 1), inside 0:7 (flag 2), inside 0:-1
    c2[1, 11, 0] = 0.5                                                        # the last column: never inside 0:-1
    for fn in (twin.get_index, TT.get_index):
        assert fn(c2, 4, 2, d2, 0.5) == [1]                                   # flag 0: columns 0:-1 -> scores 1, 0
        assert fn(c2, 12, 2, d2, 0.5) == [1]                                  # flag 1: columns 0:3 -> scores 0, 0: tie, order kept
        assert fn(c2, 20, 2, d2, 0.5) == [1]                                  # flag 2: columns 0:7 -> scores 1, 0
        c3 = c2.copy()
        c3[1, 2, 0] = 0.5
        assert fn(c3, 12, 2, d2, 0.5) == [0]                                  # flag 1: scores 0, 1
    assert twin.sche_ratio(0) == TT.sche_ratio(0) == 0.2 and twin.sche_ratio(80) == 1.0 and twin.sche_ratio(81) == 1
    assert twin.sche_ratio(-1) == 1


def test_curriculum_is_the_seesaws_alone(tmp_path):
    prob, mn, mx, theta0, states = make_case(1, 3, 1)
    with as_default(TT.TorchTwinTrainEngine()):
        with pytest.raises(ValueError, match="loss 3"):
            twin.train_batch(prob, twin.Trainer(mn, mx, 1e-3), 20, 2, theta0=theta0, states=states, curriculum=True)
    cfg = json.load(open(os.path.join(GOLDEN, "saddle_train.json")))
    cfg["CL"] = 1
    (tmp_path / "cfg.json").write_text(json.dumps(cfg))
    with pytest.raises(ValueError, match="loss 3"):
        load_trainer_script().load_config(str(tmp_path / "cfg.json"))
    with pytest.raises(ValueError, match="loss 3"):
        twin.fit(cfg, GOLDEN, str(tmp_path / "out"))
    with pytest.raises(ValueError, match="odd"):
        with as_default(TT.TorchTwinTrainEngine()):
            twin.meta_gradient(prob, mn, mx, 20, 2, 4, theta0, states)


@pytest.mark.parametrize("name", ["seesaw_CL_train.json", "saddle_train.json", "matrix_game_dim5_train.json"])
def test_train_twin_end_to_end(tmp_path, name):
    drv = load_trainer_script()
    cfg = json.load(open(os.path.join(GOLDEN, name)))
    assert set(cfg) <= set(drv.KEYS) and cfg["mode"] == "train" and cfg["unroll_unit"] == 5 and cfg["train_optim_iter"] == 100
    cfg.update(n_train=8, batch_size=8, train_optim_iter=20, unroll_unit=2, n_eval=3, eval_optim_iter=20, hidden_size=6)
    (tmp_path / "cfg.json").write_text(json.dumps(cfg))
    out = tmp_path / "result" / cfg["save_name"]
    with as_default(TT.TorchTwinTrainEngine()):
        drv.main(["--config", str(tmp_path / "cfg.json"), "--root", GOLDEN, "--out", str(out), "--epochs", "2"])
        files = set(os.listdir(out))
        assert {"epoch0min.pth", "epoch0max.pth", "epoch1min.pth", "epoch1max.pth", "bestmin.pth", "bestmax.pth",
                "twin_train.json", "curve_info"} <= files
        curves = sorted(os.listdir(out / "curve_info" / "epoch1"))
        assert len(curves) == 8 and all(re.match(r"iteration0_batch_index_\d_u_[\d.]+_v_[\d.]+\.txt$", c) for c in curves)
        assert np.loadtxt(out / "curve_info" / "epoch1" / curves[0]).shape == (20, 2 * cfg.get("dim", 1))
        record = json.load(open(out / "twin_train.json"))
        assert [e["steps"] for e in record["epochs"]] == [[5, 5], [10, 10]]
        assert record["epochs"][0]["eval_loss"] == record["best_loss"] and record["epochs"][1]["eval_loss"] is None
        # what it wrote loads through evaluate_twin's load_name / load_model
        ev = load_driver()
        test_cfg = dict(cfg, mode="test", load_name=cfg["save_name"], load_model="best", n_test=3, test_epochs=1,
                        test_optim_iter=20, test_data_path=cfg["eval_data_path"], dim=cfg.get("dim", 1))
        shutil.copy(os.path.join(GOLDEN, os.path.basename(cfg["eval_data_path"])), tmp_path)      # setup's root holds data and result/
        prob, mn, mx, _, _ = ev.setup(test_cfg, str(tmp_path))
        best = torch.load(out / "bestmin.pth")
        assert tuple(best) == twin.PARAM_NAMES and all(np.array_equal(mn.params[k], best[k].numpy()) for k in best)
    # Adam's own bound: no weight moves by more than lr per step (1e-3 of slack for its bias corrections' rounding)
    last = torch.load(out / "epoch1min.pth")
    init = twin.Optimizer(6, use_second=True, seed=cfg["seed"]).params
    moved = max(float(np.abs(last[k].numpy() - init[k]).max()) for k in twin.PARAM_NAMES)
    print("largest move of a weight after 10 steps at lr %g: %.3e" % (cfg["meta_lr"], moved))
    assert 0 < moved <= cfg["meta_lr"] * 10 * (1 + 1e-3)


def test_train_refusals_before_any_launch():
    import __graft_entry__  # noqa: F401
    lib = _abi.lib()
    net = _abi.TwinNet(50, 2)
    prob = _abi.TwinProblem(_abi.TWIN_SEESAW, 3, 1, 0, None)
    head = (C.byref(net), C.byref(net), C.byref(prob))
    assert lib.l2o_twin_train_floats(None, None, None, 4) == 0
    # one tile x 4 iterations x (record 64 + 2 * 13 * 448, scratch 48 + 2 * 13 * 256)
    assert lib.l2o_twin_train_floats(*head, 4) == 4 * (64 + 26 * 448 + 48 + 26 * 256)
    assert lib.l2o_twin_train_floats(*head, 3) == 0 and lib.l2o_twin_train_floats(*head, 0) == 0
    assert lib.l2o_twin_train_floats(*head, 64) > 0 and lib.l2o_twin_train_floats(*head, 66) == 0
    big = _abi.TwinNet(97, 2)
    assert lib.l2o_twin_train_floats(C.byref(big), C.byref(net), C.byref(prob), 4) == 0
    work = (C.c_float * 64)()

    def seg(iter0, n_iter):
        return _abi.TwinSegment(_abi.TwinRun(iter0, n_iter, 0, 1e-4, 1.0, None), 1.0, None)
    grads = _abi.TwinGrad()
    for s in (seg(2, 4), seg(1, 3), seg(1, 66), seg(1, 0)):
        assert lib.l2o_twin_train_forward(*head, C.byref(s), *(None,) * 6, work, None) == _abi.L2O_ERR_UNSUPPORTED
        assert lib.l2o_twin_train_backward(*head, C.byref(s), work, C.byref(grads), C.byref(grads), None) == _abi.L2O_ERR_UNSUPPORTED
    assert b"iter0 odd, n_iter even in [2, 64]" in lib.l2o_last_error()
    assert lib.l2o_twin_train_forward(*(None,) * 12) == _abi.L2O_ERR_UNSUPPORTED
    assert lib.l2o_twin_train_forward(C.byref(big), C.byref(net), C.byref(prob), C.byref(seg(1, 4)), *(None,) * 6, work,
                                      None) == _abi.L2O_ERR_UNSUPPORTED
    # in range, but no weights behind the descriptors
    rc = lib.l2o_twin_train_forward(*head, C.byref(seg(1, 4)), *(None,) * 6, work, None)
    assert rc == _abi.L2O_ERR_ARG
    with pytest.raises(ValueError) as ei:
        _abi.check(rc)
    assert str(ei.value) == "libl2o_hip: l2o_twin_train_forward: NULL weights"
    assert lib.l2o_twin_train_backward(*head, C.byref(seg(1, 4)), work, C.byref(grads), C.byref(grads), None) == _abi.L2O_ERR_ARG
    assert lib.l2o_last_error() == b"l2o_twin_train_backward: NULL weights"
