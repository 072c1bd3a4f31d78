"""Several confocal instances per fused launch on the MI355X (l2o_confocal_unroll_multi / _record, replicas.Replicas'
form "rows"; csrc/l2o_confocal_unroll.h with MULTI = true).

The kernel uses no atomics and fixed-order reductions, and the multi form runs the single form's code per row, so the first
check is stronger than any tolerance: everything a multi-instance launch leaves is BIT-IDENTICAL to what the single-instance
launches leave from the same start (fx, x, the whole packed state buffers, the moments, every history buffer).  Against
float64 the bounds are the module bounds of test_confocal.py (test_confocal_unroll._check): fx within max(1e-5 relative,
3 x the float32 host unroll's own distance), x_T under GRAD_TOL, carried state under CARRY_TOL, each with the 3 x own
clause; the meta-gradient of Replicas.train_step within GRAD_TOL of the float64 mean and, between the forms "rows" and
"chip", within REL_MEAN = 1e-6 per block (test_replica_training_cpu: only the pooled summation order may differ)."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import confocal_reference as R
import oracle as O
from helpers import ORACLE_CFGS, block_errors, make_params, oracle_meta_grad, spec_of
from open_l2o_amd import _abi, _engine, meta, meta_rnnprop_eval, problems
from open_l2o_amd.replicas import Replicas
from test_confocal_unroll import _check, _device_carry, _fixed, _host_unrolls
from test_meta_api import _net_config
from test_replica_training_cpu import REL_MEAN, adam_first_step, capture_adam, net_key, snapshot
from test_training_gradient import GRAD_TOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORM_CONFOCAL_MULTI = 13
SENTINEL = -7.0


@pytest.fixture
def eng():
    e = _engine.HipEngine()
    old = _engine._default_engine
    _engine.set_default_engine(e)
    yield e
    _engine.set_default_engine(old)


# ------------------------------------------------------------------------------------------------------------------
# engine level: instances as dicts of device buffers
# ------------------------------------------------------------------------------------------------------------------
def _instance(eng, rn, batch, points, T, seed, img=None):
    theta, sim = R.sample(batch, points, seed)
    nv = 6 * points + 1
    return dict(xs=[eng.tensor(a) for a in theta], sts=[eng.zeros(eng.state_floats(1, batch)) for _ in range(nv)],
                ms=[eng.zeros(batch) if rn else None for _ in range(nv)], vs=[eng.zeros(batch) if rn else None for _ in range(nv)],
                scales=[None] * nv, sim=None if img is not None else [eng.tensor(a) for a in sim],
                img=None if img is None else eng.tensor(img), fx=eng.tensor(np.full(T + 1, SENTINEL, np.float32)))


def _clone(inst):
    cp = lambda t: None if t is None else t.clone()           # noqa: E731
    return {k: ([cp(t) for t in v] if isinstance(v, list) else cp(v)) for k, v in inst.items()}


def _hist(eng, rn, batch, nv, T):
    """History buffers of one instance, every float the sentinel ("not written" and "zeroed" stay apart)."""
    full = lambda *sh: eng.tensor(np.full(sh, SENTINEL, np.float32))     # noqa: E731
    return dict(st=[full(max(T, 1), eng.state_floats(1, batch)) for _ in range(nv)], g=[full(T + 1, batch) for _ in range(nv)],
                m=[full(T + 1, batch) for _ in range(nv)] if rn else None,
                v=[full(T + 1, batch) for _ in range(nv)] if rn else None)


def _singles(eng, spec, wpack, roi, points, insts, T, step0, hists=None):
    for j, i in enumerate(insts):
        d = _engine.ConfocalDesc(i["xs"][0].numel(), points, tuple(roi), i["img"])
        eng.confocal_unroll(spec, wpack, d, i["xs"], i["sts"], i["ms"], i["vs"], i["scales"], i["sim"], T, step0, i["fx"],
                            hist=None if hists is None else hists[j])
        assert int(_abi.lib().l2o_last_unroll_form()) == 12 | (1 << 8)


def _same(eng, a, b, what):
    a, b = eng.to_numpy(a), eng.to_numpy(b)
    assert a.shape == b.shape and np.array_equal(a, b), (what, int((a != b).sum()), a.size)


def _assert_instances_equal(eng, got, want, rn):
    for j, (g, w) in enumerate(zip(got, want)):
        _same(eng, g["fx"], w["fx"], ("fx", j))
        assert np.isfinite(eng.to_numpy(g["fx"])).all() and not (eng.to_numpy(g["fx"]) == SENTINEL).any()
        for k in range(len(g["xs"])):
            _same(eng, g["xs"][k], w["xs"][k], ("x", j, k))
            _same(eng, g["sts"][k], w["sts"][k], ("state", j, k))
            if rn:
                _same(eng, g["ms"][k], w["ms"][k], ("m", j, k))
                _same(eng, g["vs"][k], w["vs"][k], ("v", j, k))


def _start(eng, name, roi, batch, points, T, seeds):
    """Instances from different seeds, one with a non-trivial x-scale on two variables; RNNProp: non-zero moments and state
    from one unroll run first (the next starts at step0 = T + 1)."""
    cfg = ORACLE_CFGS[name]
    rn = cfg.kind == "rnnprop"
    spec = spec_of(cfg)
    wpack = eng.pack_weights(spec, make_params(cfg, seed=43, trained_like=True))
    d = _engine.ConfocalDesc(batch, points, tuple(roi))
    insts = [_instance(eng, rn, batch, points, T, s) for s in seeds]
    rng = np.random.default_rng(5)
    for k in (1, 6 * points):
        insts[1]["scales"][k] = eng.tensor(rng.uniform(0.5, 2.0, batch).astype(np.float32))
    step0 = 1
    if rn:
        eng.confocal_unroll_multi(spec, wpack, d, insts, T, 1)
        step0 = T + 1
        assert all(eng.to_numpy(i["ms"][0]).any() and eng.to_numpy(i["vs"][0]).any() for i in insts)
        for i in insts:
            i["fx"].fill_(SENTINEL)
    return spec, wpack, d, insts, step0, rn


# 1. bit identity with the single form
@pytest.mark.parametrize("name", ["dm", "dm_logsign", "rnnprop"])
def test_multi_is_bit_identical_to_the_single_launches(eng, name):
    """ROI (5, 7, 6), batch 17 (row 16 is the first row of every variable's second state tile), 3 points, T = 4, three
    instances; RNNProp from step0 = 5 with non-zero moments."""
    roi, batch, points, T = (5, 7, 6), 17, 3, 4
    spec, wpack, d, insts, step0, rn = _start(eng, name, roi, batch, points, T, seeds=(11, 12, 13))
    assert step0 == (5 if rn else 1)
    want = [_clone(i) for i in insts]
    eng.confocal_unroll_multi(spec, wpack, d, insts, T, step0)
    assert int(_abi.lib().l2o_last_unroll_form()) == FORM_CONFOCAL_MULTI | (1 << 8)
    assert not eng.last_unroll_exchanges()
    _singles(eng, spec, wpack, roi, points, want, T, step0)
    _assert_instances_equal(eng, insts, want, rn)
    fxs = [eng.to_numpy(i["fx"]) for i in insts]
    assert not np.array_equal(fxs[0], fxs[1]) and not np.array_equal(fxs[1], fxs[2])       # (three different instances)


# 2. the recording form
@pytest.mark.parametrize("name", ["dm", "dm_logsign", "rnnprop"])
def test_recording_multi_is_bit_identical_to_the_single_recordings(eng, name):
    """Every history buffer, whole: the state before each step (the last row's workgroup zeroes the unused coordinates of
    its instance's last tile), the gradients, RNNProp's moments (slot 0 stays unwritten on both sides)."""
    roi, batch, points, T = (5, 7, 6), 17, 3, 4
    nv = 6 * points + 1
    spec, wpack, d, insts, step0, rn = _start(eng, name, roi, batch, points, T, seeds=(21, 22, 23))
    want = [_clone(i) for i in insts]
    hists = [_hist(eng, rn, batch, nv, T) for _ in insts]
    hwant = [_hist(eng, rn, batch, nv, T) for _ in insts]
    eng.confocal_unroll_multi(spec, wpack, d, insts, T, step0, hists=hists)
    assert int(_abi.lib().l2o_last_unroll_form()) == FORM_CONFOCAL_MULTI | (1 << 8)
    _singles(eng, spec, wpack, roi, points, want, T, step0, hists=hwant)
    _assert_instances_equal(eng, insts, want, rn)
    for j, (h, w) in enumerate(zip(hists, hwant)):
        for part in ("st", "g") + (("m", "v") if rn else ()):
            for k in range(nv):
                _same(eng, h[part][k], w[part][k], ("hist", part, j, k))
        st = eng.to_numpy(h["st"][0])
        assert not (st == SENTINEL).any()                      # every coordinate of both tiles written or zeroed
        assert not (eng.to_numpy(h["g"][0]) == SENTINEL).any()
        if rn:
            m = eng.to_numpy(h["m"][0])
            assert (m[0] == SENTINEL).all() and not (m[1:] == SENTINEL).any()


# 3. inference mode
def test_inference_instances_read_their_own_img(eng):
    """Two instances with different targets; the descriptor's own img is instance 0's and is ignored for instance 1."""
    roi, batch, points, T = (3, 2, 4), 2, 1, 3
    cfg = O.DM_IDENTITY
    spec = spec_of(cfg)
    wpack = eng.pack_weights(spec, make_params(cfg, seed=43, trained_like=True))
    rng = np.random.default_rng(31)
    imgs = [(0.1 + rng.random((batch, 2 * 3 * 4))).astype(np.float32) for _ in range(2)]
    insts = [_instance(eng, False, batch, points, T, 32, img=im) for im in imgs]       # (the same x: only img differs)
    want = [_clone(i) for i in insts]
    d = _engine.ConfocalDesc(batch, points, roi, insts[0]["img"])
    eng.confocal_unroll_multi(spec, wpack, d, insts, T, 1)
    _singles(eng, spec, wpack, roi, points, want, T, 1)
    _assert_instances_equal(eng, insts, want, False)
    assert not np.array_equal(eng.to_numpy(insts[0]["fx"]), eng.to_numpy(insts[1]["fx"]))


# 4. edges
def _c_instances(insts, nv):
    arr = (_abi.ConfocalInstance * len(insts))()
    for j, i in enumerate(insts):
        arr[j].fx = i["fx"].data_ptr()
        for k in range(nv):
            arr[j].x[k], arr[j].st[k], arr[j].sim[k] = i["xs"][k].data_ptr(), i["sts"][k].data_ptr(), i["sim"][k].data_ptr()
    return arr


@pytest.mark.parametrize("n_inst", [1, 32])
def test_one_and_thirty_two_instances(eng, n_inst):
    roi, batch, points, T = (2, 2, 2), 1, 1, 1
    cfg = O.DM_IDENTITY
    spec = spec_of(cfg)
    wpack = eng.pack_weights(spec, make_params(cfg, seed=43, trained_like=True))
    insts = [_instance(eng, False, batch, points, T, 40 + j) for j in range(n_inst)]
    want = [_clone(i) for i in insts]
    d = _engine.ConfocalDesc(batch, points, roi)
    assert eng.confocal_unroll_multi_supported(spec, d, n_inst)
    eng.confocal_unroll_multi(spec, wpack, d, insts, T, 1)
    assert int(_abi.lib().l2o_last_unroll_form()) == FORM_CONFOCAL_MULTI | 256
    assert not eng.last_unroll_exchanges()
    _singles(eng, spec, wpack, roi, points, want, T, 1)
    _assert_instances_equal(eng, insts, want, False)


def test_refusals_launch_nothing(eng):
    """33 instances: L2O_ERR_UNSUPPORTED; a NULL x[k] of a live variable in instance 1: L2O_ERR_ARG; nothing is written."""
    lib = _abi.lib()
    roi, batch, points, T = (2, 2, 2), 1, 1, 1
    nv = 6 * points + 1
    cfg = O.DM_IDENTITY
    spec = spec_of(cfg)
    cc = spec.to_c()
    wpack = eng.pack_weights(spec, make_params(cfg, seed=43, trained_like=True))
    insts = [_instance(eng, False, batch, points, T, 60 + j) for j in range(33)]
    for i in insts:
        for t in i["xs"]:
            t.fill_(SENTINEL)
    m = _abi.Confocal()
    m.batch, m.num_points = batch, points
    m.roi[0], m.roi[1], m.roi[2] = roi
    scratch = eng.tensor(np.full(1 << 16, SENTINEL, np.float32))
    vp = lambda t: C.c_void_p(t.data_ptr())                    # noqa: E731
    d = _engine.ConfocalDesc(batch, points, roi)
    assert not eng.confocal_unroll_multi_supported(spec, d, 33) and not eng.confocal_unroll_multi_supported(spec, d, 0)
    assert lib.l2o_confocal_unroll_multi_scratch_floats(C.byref(m), 33, T) == 0
    hists = (_abi.ConfocalHist * 33)()
    arr = _c_instances(insts, nv)
    rc = lib.l2o_confocal_unroll_multi(C.byref(cc), vp(wpack), C.byref(m), arr, 33, T, 1, vp(scratch), eng._stream())
    assert rc == _abi.L2O_ERR_UNSUPPORTED, rc
    rc = lib.l2o_confocal_unroll_multi_record(C.byref(cc), vp(wpack), C.byref(m), arr, 33, T, 1, hists, vp(scratch),
                                              eng._stream())
    assert rc == _abi.L2O_ERR_UNSUPPORTED, rc
    with pytest.raises(_abi.L2OUnsupported):
        eng.confocal_unroll_multi(spec, wpack, d, insts, T, 1)
    arr = _c_instances(insts[:3], nv)
    arr[1].x[nv - 1] = None
    rc = lib.l2o_confocal_unroll_multi(C.byref(cc), vp(wpack), C.byref(m), arr, 3, T, 1, vp(scratch), eng._stream())
    assert rc == _abi.L2O_ERR_ARG, rc
    eng.synchronize()
    for t in [scratch] + [i["fx"] for i in insts] + [t for i in insts for t in i["xs"]]:
        assert (eng.to_numpy(t) == SENTINEL).all()             # nothing ran
    assert all(not eng.to_numpy(t).any() for i in insts for t in i["sts"])


# ------------------------------------------------------------------------------------------------------------------
# Replicas
# ------------------------------------------------------------------------------------------------------------------
def _replicas(name, roi, batch, points, T, seeds, params_seed=43):
    """(Replicas, [sim per replica]): one problem per seed, every replica from its own fixed start."""
    cfg = ORACLE_CFGS[name]
    params = make_params(cfg, seed=params_seed, trained_like=True)
    meta.set_random_seed(44)
    probs, sims = [], []
    for s in seeds:
        theta, sim, data = _fixed(batch, points, seed=s)
        probs.append(problems.confocal_microscopy_3d(batch_size=batch, num_points=points, ROI=list(roi), data=data, fused=True))
        sims.append(sim)
    if cfg.kind == "rnnprop":
        opt = meta_rnnprop_eval.MetaOptimizer(0.95, 0.95, **_net_config(cfg, params, key="rp"))
    else:
        opt = meta.MetaOptimizer(**_net_config(cfg, params))
    return Replicas(opt, probs, T), sims, params


# 5. against float64
@pytest.mark.parametrize("name,n", [("dm", 1), ("rnnprop", 2)])
def test_replicas_run_vs_float64(eng, name, n):
    """Three replicas of test_confocal_unroll's "19-coords-row16" case through Replicas.run (form "rows"), every replica
    under that module's bounds; RNNProp: two consecutive runs, the second from step0 = T + 1 with the carried moments."""
    roi, batch, points, T = (5, 7, 6), 17, 3, 20
    cfg = ORACLE_CFGS[name]
    rn = cfg.kind == "rnnprop"
    reps, sims, params = _replicas(name, roi, batch, points, T, seeds=(41, 42, 45))
    reps.reset()
    assert reps.rows_supported()
    v0s = [[v.eval().reshape(-1).copy() for v in g.x] for g in reps.graphs]
    fxs = [[] for _ in reps.graphs]
    for k in range(n):
        reps.run({reps.step: 1 + k * T} if rn else None)
        assert reps.last_form == "rows" and all(g.last_path == "confocal_multi" for g in reps.graphs)
        assert int(_abi.lib().l2o_last_unroll_form()) == FORM_CONFOCAL_MULTI | (1 << 8)
        for j, fx in enumerate(reps.fx_arrays):
            fxs[j].append(np.asarray(fx, np.float64).copy())
    for j, g in enumerate(reps.graphs):
        carry = _device_carry(eng, g, rn)
        ref64 = _host_unrolls(cfg, params, roi, points, v0s[j], sims[j], T, n, np.float64)
        ref32 = _host_unrolls(cfg, params, roi, points, v0s[j], sims[j], T, n, np.float32)
        _check("%s replica %d" % (name, j), points, fxs[j], carry, ref64, ref32)


# 6. train_step
@pytest.mark.parametrize("name", ["dm", "rnnprop"])
def test_train_step_rows_vs_chip_and_float64(eng, name):
    """Three replicas (batch 4, 2 points, ROI (5, 4, 6), T = 3): the gradient form "rows" hands to Adam against form "chip"
    from the same start (REL_MEAN per block), against the float64 mean of the replicas' oracle meta-gradients (GRAD_TOL), and
    the weights after the step."""
    roi, batch, points, T, lr = (5, 4, 6), 4, 2, 3, 1e-3
    cfg = ORACLE_CFGS[name]
    got = {}
    for form in ("rows", "chip"):
        reps, sims, params = _replicas(name, roi, batch, points, T, seeds=(51, 52, 53), params_seed=52)
        caps = capture_adam(reps)
        key = net_key(reps)
        reps.reset()
        feed = {reps.step: 1} if reps.graphs[0].rnnprop else {}
        snaps = [snapshot(eng, g, key, 1) for g in reps.graphs]
        w0 = {m: {v: np.asarray(a, np.float32).copy() for v, a in d.items()}
              for m, d in reps.graphs[0].nets[key].variables.items()}
        out = reps.train_step(feed, lr, form=form)
        assert reps.last_form == form and len(caps) == 1
        assert all(g.last_path == ("confocal_multi" if form == "rows" else "confocal_unroll") for g in reps.graphs)
        assert out["fx"].shape == (3,) and np.isfinite(out["fx"]).all()
        got[form] = (caps[0], out, snaps, w0, reps, sims)
    g_rows, out_rows, snaps, w0, reps, sims = got["rows"]
    g_chip, out_chip = got["chip"][0], got["chip"][1]
    assert np.array_equal(out_rows["fx"], out_chip["fx"])      # (the forward is bit-identical)
    want_chip = {}
    for (mod, var), a in g_chip.items():
        want_chip.setdefault(mod, {})[var] = a
    errs = block_errors(g_rows, want_chip)
    print("rows vs chip", {k: "%.3e" % e for k, e in errs.items()})
    assert max(errs.values()) < REL_MEAN, errs
    # the float64 mean of the three reference meta-gradients
    ref = R.Confocal(roi, points)
    want = {}
    for snap, sim in zip(snaps, sims):
        st = tuple((h, c) for h, c in snap["state"])
        g64, _ = oracle_meta_grad(cfg, snap["w"], ref.flat_fg(batch, sim), snap["x"], st, T, m0=snap["m"], v0=snap["v"],
                                  step0=snap["step0"])
        for mod, dd in g64.items():
            for var, a in dd.items():
                want.setdefault(mod, {}).setdefault(var, []).append(a)
    want = {mod: {var: np.mean(a, axis=0) for var, a in dd.items()} for mod, dd in want.items()}
    errs = block_errors(g_rows, want)
    print("rows vs float64 mean", {k: "%.3e" % e for k, e in errs.items()})
    assert max(errs.values()) < GRAD_TOL, errs
    w1 = reps.graphs[0].nets[net_key(reps)].variables
    for (mod, var), g in g_rows.items():
        np.testing.assert_allclose(w1[mod][var], adam_first_step(w0[mod][var], g.reshape(w0[mod][var].shape), lr),
                                   rtol=1e-6, atol=1e-9)


# 7. the default shape once
def test_default_shape_eight_replicas_bit_identical_to_single_launches(eng):
    """Batch 32, 5 points, 28^3, T = 5, DM: 256 workgroups in one launch against eight fused launches of 32."""
    roi, batch, points, T = (28, 28, 28), 32, 5, 5
    seeds = tuple(range(71, 79))
    rows, _, _ = _replicas("dm", roi, batch, points, T, seeds)
    rows.reset()
    rows.run()
    assert rows.last_form == "rows"
    chip, _, _ = _replicas("dm", roi, batch, points, T, seeds)
    chip.reset()
    chip.run(form="chip")
    assert chip.last_form == "chip" and all(g.last_path == "confocal_unroll" for g in chip.graphs)
    for j, (a, b) in enumerate(zip(rows.fx_arrays, chip.fx_arrays)):
        assert a.shape == (T + 1,) and np.array_equal(a, b), (j, a, b)
        assert np.isfinite(a).all()
    assert not np.array_equal(rows.fx_arrays[0], rows.fx_arrays[1])
    for ga, gb in zip(rows.graphs, chip.graphs):
        for va, vb in zip(ga.x, gb.x):
            assert np.array_equal(va.eval(), vb.eval())


# 8. the driver
def test_evaluate_dm_driver_with_replicas():
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "evaluate_dm.py"), "--problem", "confocal_microscopy_3d",
           "--num_steps", "10", "--seed", "3", "--confocal_fused", "1", "--unroll_len", "5", "--replicas", "3"]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "kernel form: rows" in out.stdout, out.stdout[-2000:]
    m = re.search(r"final cost per replica: (.+)", out.stdout)
    costs = [float(x) for x in m.group(1).split()]
    assert len(costs) == 3 and all(math.isfinite(c) for c in costs), out.stdout[-2000:]
