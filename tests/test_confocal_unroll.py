"""The fused persistent unroll of problems.confocal_microscopy_3d(fused=True) on the MI355X (csrc/l2o_confocal_unroll.h,
l2o_confocal_unroll / l2o_confocal_unroll_record): against the float64 host unroll (oracle.unroll_multi over
confocal_reference.py), interchanged with the step-granular path on the same buffers, with the training fork's x-scaling,
in inference mode, bit-reproducibility, the recording form's meta-gradient, the fall-backs and refused shapes, and the DM
evaluation driver.

Bounds (the module bounds of test_confocal.py, the project's own): per-step fx within max(1e-5 relative, 3 x the float32
host unroll's own distance from float64); x_T within max(GRAD_TOL of the array's largest float64 entry, 3 x own); carried
LSTM state and RNNProp moments within max(CARRY_TOL, 3 x own) of the array's largest entry.  Every measured error is printed
next to the float32 reference's own."""
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
from helpers import ORACLE_CFGS, block_errors, make_params, spec_of
from open_l2o_amd import _abi, _engine, meta, meta_dm_train, meta_rnnprop_eval, problems
from open_l2o_amd.session import Session
from test_meta_api import _net_config
from test_training_gradient import CARRY_TOL, GRAD_TOL, Trainer, _carried, split_carry

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORM_CONFOCAL_UNROLL = 12


@pytest.fixture
def eng():
    e = _engine.HipEngine()
    old = _engine._default_engine
    _engine.set_default_engine(e)
    yield e
    _engine.set_default_engine(old)


def _bound(got, want, g32):
    scale = float(np.abs(want).max())
    return float(np.abs(got - want).max()), max(GRAD_TOL * scale, 3 * float(np.abs(g32 - want).max()))


def _fixed(batch, points, seed):
    theta, sim = R.sample(batch, points, seed)
    data = dict(zip(R.trainable_names(points), theta))
    data.update(zip(R.sim_names(points), sim))
    return theta, sim, data


def _graph(cfg, params, problem, T, scaled=False):
    """(graph, ml, step placeholder or None, scale placeholders or None) of meta_loss over the problem."""
    if scaled:
        optimizer = meta_dm_train.MetaOptimizer(0, **_net_config(cfg, params))
        out = optimizer.meta_loss(problem, T)
        return optimizer.graph, out[0], None, out[1]
    if cfg.kind == "rnnprop":
        optimizer = meta_rnnprop_eval.MetaOptimizer(0.95, 0.95, **_net_config(cfg, params, key="rp"))
        ml, _, _, step = optimizer.meta_loss(problem, T)
        return optimizer.graph, ml, step, None
    optimizer = meta.MetaOptimizer(**_net_config(cfg, params))
    ml = optimizer.meta_loss(problem, T)
    return optimizer.graph, ml, None, None


def _device_carry(eng, graph, rn):
    """Per variable: x, the unpacked LSTM state and the moments, as float64."""
    slot_of = {s.var_index: s for s in graph.slots}
    out = []
    for j, var in enumerate(graph.x):
        s = slot_of[j]
        h1, c1, h2, c2 = (eng.to_numpy(a).astype(np.float64) for a in eng.state_unpack(s.state.packed, s.state.B, s.state.D))
        out.append(dict(x=var.eval().astype(np.float64).reshape(-1), state=((h1, c1), (h2, c2)),
                        m=eng.to_numpy(s.m).astype(np.float64).reshape(-1) if rn else None,
                        v=eng.to_numpy(s.v).astype(np.float64).reshape(-1) if rn else None))
    return out


def _device_unrolls(eng, monkeypatch, cfg, params, problem, T, paths, scales=None):
    """One committed unroll per entry of `paths` ("confocal_unroll" / "steps": L2O_DISABLE_FUSED set for the latter) from
    the problem's initial values.  Returns (v0, [fx array per unroll], carried state at the end)."""
    rn = cfg.kind == "rnnprop"
    graph, ml, step, scale_ph = _graph(cfg, params, problem, T, scaled=scales is not None)
    fxs = []
    with Session() as sess:
        sess.run(ml.reset)
        v0 = [v.eval().reshape(-1).copy() for v in graph.x]
        for k, path in enumerate(paths):
            if path == "steps":
                monkeypatch.setenv("L2O_DISABLE_FUSED", "1")
            else:
                monkeypatch.delenv("L2O_DISABLE_FUSED", raising=False)
            feed = {step: 1 + k * T} if rn else {}
            if scales is not None:
                feed.update(zip(scale_ph, scales))
            res = graph.execute(feed, True)
            assert graph.last_path == path, (k, graph.last_path)
            if path == "confocal_unroll":
                assert int(_abi.lib().l2o_last_unroll_form()) == FORM_CONFOCAL_UNROLL | (1 << 8)
                assert not eng.last_unroll_exchanges()
            fxs.append(np.asarray(res["fx_array"], np.float64).copy())
        carry = _device_carry(eng, graph, rn)
    monkeypatch.delenv("L2O_DISABLE_FUSED", raising=False)
    return v0, fxs, carry


def _host_unrolls(cfg, params, roi, points, v0, sim, T, n, dt, img=None, scales=None):
    """n consecutive host unrolls in dtype dt.  Returns ([fx per unroll], carried state per variable)."""
    rn = cfg.kind == "rnnprop"
    ref = R.Confocal(roi, points, img)
    p = {m: {v: a.astype(dt) for v, a in d.items()} for m, d in params.items()}
    sm = None if sim is None else [a.astype(dt) for a in sim]
    sc = None if scales is None else [s.reshape(-1).astype(dt) for s in scales]

    def fg(vs, t, wg):
        if sc is None:
            return ref.fg(vs, sm, wg)
        res = ref.fg([v * s for v, s in zip(vs, sc)], sm, wg)
        if not wg:
            return res
        return res[0], [g * s for g, s in zip(res[1], sc)]

    xs = [a.astype(dt) for a in v0]
    states = [tuple((h.astype(dt), c.astype(dt)) for h, c in O.net_initial_state(cfg, a.size)) for a in v0]
    ms = vs = None
    fxs = []
    for k in range(n):
        if rn:
            fx, xs, states, ms, vs = O.unroll_multi(fg, cfg, p, xs, states, T, ms=ms, vs=vs, step0=1 + k * T, return_moments=True)
        else:
            fx, xs, states = O.unroll_multi(fg, cfg, p, xs, states, T)
        fxs.append(np.asarray(fx, np.float64))
    carry = [dict(x=np.asarray(x, np.float64).reshape(-1), state=tuple((np.asarray(h, np.float64), np.asarray(c, np.float64))
                                                                        for h, c in st),
                  m=np.asarray(ms[j], np.float64).reshape(-1) if rn else None,
                  v=np.asarray(vs[j], np.float64).reshape(-1) if rn else None) for j, (x, st) in enumerate(zip(xs, states))]
    return fxs, carry


def _check(what, points, fxs, carry, ref64, ref32):
    """fx of every unroll and step, x_T, the LSTM state and the moments under the module's bounds; prints the worst."""
    (fx64, c64), (fx32, c32) = ref64, ref32
    worst_fx = (0.0, 0.0)
    for k, (a, w, w32) in enumerate(zip(fxs, fx64, fx32)):
        assert a.shape == w.shape
        for t in range(len(w)):
            err, own = abs(a[t] - w[t]), abs(w32[t] - w[t])
            worst_fx = max(worst_fx, (err / abs(w[t]), own / abs(w[t])))
            assert err <= max(1e-5 * abs(w[t]), 3 * own), (what, "fx", k, t, a[t], w[t], w32[t])
    print(what, "fx worst rel %.3e (float32 host unroll at that step %.3e)" % worst_fx)
    worst_x, worst_c = (0.0, 0.0, ""), (0.0, 0.0, "")
    for nm, d, d64, d32 in zip(R.trainable_names(points), carry, c64, c32):
        err, bound = _bound(d["x"], d64["x"], d32["x"])
        scale = float(np.abs(d64["x"]).max())
        worst_x = max(worst_x, (err / scale, float(np.abs(d32["x"] - d64["x"]).max()) / scale, nm))
        assert err <= bound, (what, "x", nm, err, bound)
        a, r64, r32 = _carried(d), _carried(d64), _carried(d32)
        for part in r64:
            if part == "x":
                continue
            scale = max(float(np.abs(r64[part]).max()), 1e-30)
            err = float(np.abs(a[part] - r64[part]).max()) / scale
            own = float(np.abs(r32[part] - r64[part]).max()) / scale
            worst_c = max(worst_c, (err, own, nm + "." + part))
            assert err < max(CARRY_TOL, 3 * own), (what, nm, part, err, own)
    print(what, "x_T worst %.3e of the array's largest entry (float32 host unroll %.3e) at %s" % worst_x)
    print(what, "carried state / moments worst %.3e (float32 host unroll %.3e) at %s" % worst_c)


# ------------------------------------------------------------------------------------------------------------------
# 1. the unroll against the float64 host unroll
# ------------------------------------------------------------------------------------------------------------------
CASES = [pytest.param((3, 2, 4), 5, 1, 3, "dm", 1, id="7-coords-unequal-edges"),
         pytest.param((5, 7, 6), 17, 3, 20, "dm", 1, id="19-coords-row16-dm"),
         pytest.param((5, 7, 6), 17, 3, 20, "dm_logsign", 1, id="19-coords-row16-logsign"),
         pytest.param((5, 7, 6), 17, 3, 20, "rnnprop", 2, id="19-coords-row16-rnnprop-two-unrolls"),
         pytest.param((8, 8, 8), 4, 8, 5, "dm", 1, id="49-coords-four-tiles"),
         pytest.param((28, 28, 28), 32, 5, 5, "dm", 1, id="default-shape")]


@pytest.mark.parametrize("roi,batch,points,T,name,n", CASES)
def test_unroll_vs_float64(eng, monkeypatch, roi, batch, points, T, name, n):
    """x_T, the unpacked LSTM state (and RNNProp's moments) and fx[0..T] of n consecutive committed fused unrolls; RNNProp's
    second unroll starts at step0 = T + 1 with non-zero moments.

    Measured on one MI355X, worst over the six cases (the float32 host unroll's own distance in brackets): fx 4.3e-7
    relative at RNNProp's worst step (4.3e-7), at most 1.5e-7 (1.5e-7) for the DM nets; x_T 3.4e-7 of an array's largest
    entry (3.4e-7); LSTM state and moments 3.5e-6 (3.3e-6; LogAndSign, one variable's h1), the default shape 5.0e-7
    (3.3e-7)."""
    cfg = ORACLE_CFGS[name]
    theta, sim, data = _fixed(batch, points, seed=41)
    params = make_params(cfg, seed=43, trained_like=True)
    meta.set_random_seed(44)
    problem = problems.confocal_microscopy_3d(batch_size=batch, num_points=points, ROI=list(roi), data=data, fused=True)
    v0, fxs, carry = _device_unrolls(eng, monkeypatch, cfg, params, problem, T, ["confocal_unroll"] * n)
    for a, want in zip(v0, theta):
        assert np.array_equal(a, want)
    ref64 = _host_unrolls(cfg, params, roi, points, v0, sim, T, n, np.float64)
    ref32 = _host_unrolls(cfg, params, roi, points, v0, sim, T, n, np.float32)
    _check("%s %r batch %d points %d" % (name, roi, batch, points), points, fxs, carry, ref64, ref32)


# ------------------------------------------------------------------------------------------------------------------
# 2. layout interchange: the fused unroll and the step path on the same buffers, in both orders
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dm", "rnnprop"])
@pytest.mark.parametrize("paths", [("confocal_unroll", "steps"), ("steps", "confocal_unroll")])
def test_layout_interchange_with_the_step_path(eng, monkeypatch, name, paths):
    """Two consecutive committed unrolls, one fused and one step-granular, against the float64 two-unroll reference: the
    state gather / scatter must be the layout the step path keeps (batch 17: row 16 sits in every variable's second tile),
    not merely self-consistent.

    Measured on one MI355X, both orders alike: fx 1.3e-7 relative (dm; float32 host unroll 1.5e-8) and 1.5e-7 (rnnprop;
    1.5e-7); x_T 2.4e-7 and 1.5e-7 of an array's largest entry (the float32 host unroll's own: the same); state and moments
    3.8e-7 (2.5e-7) for dm, and for rnnprop 2.9e-5 on one variable's h1 (float32 host unroll 4.9e-5: the 3 x clause), every
    other array inside CARRY_TOL."""
    roi, batch, points, T = (5, 7, 6), 17, 3, 6
    cfg = ORACLE_CFGS[name]
    theta, sim, data = _fixed(batch, points, seed=61)
    params = make_params(cfg, seed=62, trained_like=True)
    meta.set_random_seed(63)
    problem = problems.confocal_microscopy_3d(batch_size=batch, num_points=points, ROI=list(roi), data=data, fused=True)
    v0, fxs, carry = _device_unrolls(eng, monkeypatch, cfg, params, problem, T, list(paths))
    ref64 = _host_unrolls(cfg, params, roi, points, v0, sim, T, 2, np.float64)
    ref32 = _host_unrolls(cfg, params, roi, points, v0, sim, T, 2, np.float32)
    _check("%s %s" % (name, "+".join(paths)), points, fxs, carry, ref64, ref32)


# ------------------------------------------------------------------------------------------------------------------
# 3. x-scaling
# ------------------------------------------------------------------------------------------------------------------
def test_x_scaling(eng, monkeypatch):
    """The training fork's scale placeholders fed with values in [0.5, 2]: the optimizee is evaluated at x s and the
    optimizer sees grad s; the path stays the fused one.

    Measured on one MI355X: fx 1.3e-7 relative (float32 host unroll 1.3e-7), x_T 1.5e-7 (1.5e-7), state 3.3e-7 (2.0e-7)."""
    roi, batch, points, T = (5, 7, 6), 17, 3, 6
    cfg = O.DM_IDENTITY
    theta, sim, data = _fixed(batch, points, seed=71)
    params = make_params(cfg, seed=72, trained_like=True)
    meta.set_random_seed(73)
    rng = np.random.default_rng(74)
    scales = [rng.uniform(0.5, 2.0, (batch, 1)).astype(np.float32) for _ in range(6 * points + 1)]
    problem = problems.confocal_microscopy_3d(batch_size=batch, num_points=points, ROI=list(roi), data=data, fused=True)
    v0, fxs, carry = _device_unrolls(eng, monkeypatch, cfg, params, problem, T, ["confocal_unroll"], scales=scales)
    ref64 = _host_unrolls(cfg, params, roi, points, v0, sim, T, 1, np.float64, scales=scales)
    ref32 = _host_unrolls(cfg, params, roi, points, v0, sim, T, 1, np.float32, scales=scales)
    _check("x-scale", points, fxs, carry, ref64, ref32)
    # the scaling matters to this check: the unscaled reference is far outside the bound
    plain = _host_unrolls(cfg, params, roi, points, v0, sim, T, 1, np.float64)
    assert abs(plain[0][0][T] - ref64[0][0][T]) > 1e-3 * abs(ref64[0][0][T])


# ------------------------------------------------------------------------------------------------------------------
# 4. inference mode
# ------------------------------------------------------------------------------------------------------------------
def test_inference_mode(eng, monkeypatch):
    """The supplied volume of test_confocal.test_fg_inference (a ramp along each axis plus noise, one all-zero row).

    Measured on one MI355X: fx 1.0e-7 relative (float32 host unroll 3.2e-8), x_T 9.0e-8 (9.0e-8), state 3.6e-7 (1.1e-7)."""
    roi, batch, points, T = (5, 7, 6), 3, 2, 5
    cfg = O.DM_IDENTITY
    theta, _ = R.sample(batch, points, seed=11)
    iy, ix, iz = np.meshgrid(np.arange(7), np.arange(5), np.arange(6), indexing="ij")       # [Ry, Rx, Rz]
    img = 0.2 * np.random.default_rng(12).random((batch, 7, 5, 6)) + (iy / 7.0 + 0.5 * iz / 6.0 + 0.25 * ix / 5.0)[None]
    img = img.reshape(batch, -1).astype(np.float32)
    img[2] = 0.0
    data = dict(zip(R.trainable_names(points), theta))
    data["img"] = img
    params = make_params(cfg, seed=82, trained_like=True)
    meta.set_random_seed(83)
    problem = problems.confocal_microscopy_3d(batch_size=batch, num_points=points, ROI=list(roi), data=data, inference=True,
                                              fused=True)
    v0, fxs, carry = _device_unrolls(eng, monkeypatch, cfg, params, problem, T, ["confocal_unroll"])
    ref64 = _host_unrolls(cfg, params, roi, points, v0, None, T, 1, np.float64, img=img)
    ref32 = _host_unrolls(cfg, params, roi, points, v0, None, T, 1, np.float32, img=img)
    _check("inference", points, fxs, carry, ref64, ref32)


# ------------------------------------------------------------------------------------------------------------------
# 5. bit reproducibility
# ------------------------------------------------------------------------------------------------------------------
def test_two_launches_from_the_same_start_are_bit_identical(eng, monkeypatch):
    roi, batch, points, T = (5, 7, 6), 17, 3, 8
    cfg = O.RNNPROP
    theta, sim, data = _fixed(batch, points, seed=91)
    params = make_params(cfg, seed=92, trained_like=True)
    runs = []
    for _ in range(2):
        meta.set_random_seed(93)
        problem = problems.confocal_microscopy_3d(batch_size=batch, num_points=points, ROI=list(roi), data=data, fused=True)
        v0, fxs, carry = _device_unrolls(eng, monkeypatch, cfg, params, problem, T, ["confocal_unroll"])
        runs.append((np.asarray(fxs[0], np.float64), [d["x"] for d in carry], [d["state"] for d in carry]))
    (fa, xa, sa), (fb, xb, sb) = runs
    assert np.array_equal(fa, fb)
    for a, b in zip(xa, xb):
        assert np.array_equal(a, b)
    for a, b in zip(sa, sb):
        assert all(np.array_equal(p, q) for la, lb in zip(a, b) for p, q in zip(la, lb))


# ------------------------------------------------------------------------------------------------------------------
# 6. the recording form: one first-order train step against helpers.oracle_meta_grad
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dm", "rnnprop"])
def test_recording_form_meta_gradient_vs_float64(eng, name):
    """test_confocal.test_meta_gradient_vs_float64's case with fused=True: the history of l2o_confocal_unroll_record through
    the unchanged back-propagation, under that test's block and carry bounds.

    Measured on one MI355X: every meta-gradient block within 2.0e-7 of its largest entry (dm; float32 oracle 2.5e-7) and
    2.2e-7 (rnnprop; 3.3e-7); the carried x / state / moments at most 1.0e-6 (one variable's h1, float32 oracle 8.7e-6)."""
    T, batch, points, roi = 10, 4, 2, (8, 8, 8)
    theta, sim, data = _fixed(batch, points, seed=51)
    params = make_params(ORACLE_CFGS[name], seed=52, trained_like=True)
    meta.set_random_seed(53)
    tr = Trainer(eng, name, params, problems.confocal_microscopy_3d(batch_size=batch, num_points=points, ROI=list(roi),
                                                                    data=data, fused=True), T)
    shapes = [tuple(v.shape) for v in tr.graph.x]
    assert shapes == [(batch, 1)] * (6 * points + 1)
    ref = R.Confocal(roi, points)
    tr.reset()
    snap = tr.snapshot()
    got = tr.train_step()
    assert tr.graph.last_path == "confocal_unroll"
    assert int(_abi.lib().l2o_last_unroll_form()) & 0xff == FORM_CONFOCAL_UNROLL
    fg = ref.flat_fg(batch, sim)
    want, end = tr.reference(fg, snap)
    g32, end32 = tr.reference(fg, snap, np.float32)
    errs, errs32 = block_errors(got, want), block_errors(g32, want)
    for blk, e in errs.items():
        print("meta-gradient", blk, "err %.3e float32 oracle %.3e" % (e, errs32[blk]))
        assert e < max(GRAD_TOL, 3 * errs32[blk]), (blk, e, errs32[blk])
    after = tr.snapshot()
    for j, (sv, ev, e32) in enumerate(zip(after["vars"], split_carry(end, shapes), split_carry(end32, shapes))):
        a, r64, r32 = _carried(sv), _carried(ev), _carried(e32)
        for nm in r64:
            scale = max(float(np.abs(r64[nm]).max()), 1e-30)
            err = float(np.abs(a[nm] - r64[nm]).max()) / scale
            own = float(np.abs(r32[nm] - r64[nm]).max()) / scale
            print("carry variable", j, nm, "err %.3e own %.3e" % (err, own))
            assert err < max(CARRY_TOL, 3 * own), (j, nm, err, own)


# ------------------------------------------------------------------------------------------------------------------
# 7. fall-backs and limits
# ------------------------------------------------------------------------------------------------------------------
def test_fallbacks_run_on_the_step_path(eng):
    """fused=True where the fused form does not apply: a net that is not the (20, 20) stack, a two-term ensemble, a term
    weight other than 1."""
    opts = {"batch_size": 3, "num_points": 1, "ROI": [4, 5, 3], "fused": True}
    one = O.NetConfig("cw", (1,), "identity", None, 0.1, False)
    cases = [(one, problems.confocal_microscopy_3d(**opts)),
             (O.DM_IDENTITY, problems.ensemble([{"name": "confocal_microscopy_3d", "options": opts}] * 2)),
             (O.DM_IDENTITY, problems.ensemble([{"name": "confocal_microscopy_3d", "options": opts}], weights=[0.5]))]
    for cfg, problem in cases:
        meta.set_random_seed(5)
        optimizer = meta.MetaOptimizer(**_net_config(cfg, make_params(cfg, seed=6, trained_like=cfg is not one)))
        ml = optimizer.meta_loss(problem, 2)
        with Session() as sess:
            sess.run(ml.reset)
            res = optimizer.graph.execute({}, True)
        assert optimizer.graph.last_path == "steps"
        assert np.isfinite(np.asarray(res["fx_array"])).all()
        assert all(t.hyper["fused"] for t in optimizer.graph.terms)


def test_support_predicate_and_refused_shapes_launch_nothing(eng):
    lib = _abi.lib()
    d = _engine.ConfocalDesc(4, 2, (8, 8, 8))
    for name in ("dm", "dm_logsign", "rnnprop"):
        assert eng.confocal_unroll_supported(spec_of(ORACLE_CFGS[name]), d) == 1
    for layers in ((8, 8), (1,), (20,), (20, 20, 20)):
        assert eng.confocal_unroll_supported(spec_of(O.NetConfig("cw", layers, "identity", None, 0.1, False)), d) == 0
    batch, points, T = 4, 2, 3
    cc = spec_of(O.DM_IDENTITY).to_c()
    nmax = _abi.CONFOCAL_MAX_VARS
    theta, sim = R.sample(batch, 8, seed=13)
    xs = [eng.tensor(np.full(batch, -7.0, np.float32)) for _ in range(nmax)]
    sts = [eng.tensor(np.full(eng.state_floats(1, batch), -7.0, np.float32)) for _ in range(nmax)]
    sm = [eng.tensor(a) for a in sim]
    hg = [eng.tensor(np.full((T + 1) * batch, -7.0, np.float32)) for _ in range(nmax)]
    hs = [eng.tensor(np.full(T * eng.state_floats(1, batch), -7.0, np.float32)) for _ in range(nmax)]
    arr = lambda ts: (C.c_void_p * nmax)(*[t.data_ptr() for t in ts])        # noqa: E731
    ax, ast, asm = arr(xs), arr(sts), arr(sm)
    h = _abi.ConfocalHist()
    for k in range(nmax):
        h.st[k], h.g[k] = hs[k].data_ptr(), hg[k].data_ptr()
    wpack = eng.zeros(int(lib.l2o_wpack_floats(C.byref(cc))))
    fx = eng.tensor(np.full(T + 1, -7.0, np.float32))
    scratch = eng.tensor(np.full(1 << 16, -7.0, np.float32))
    vp = lambda t: C.c_void_p(t.data_ptr())                                 # noqa: E731
    for b, p, roi in ((0, points, (8, 8, 8)), (1025, points, (8, 8, 8)), (batch, 0, (8, 8, 8)), (batch, 9, (8, 8, 8)),
                      (batch, points, (1, 8, 8)), (batch, points, (8, 8, 33)), (batch, points, (8, 33, 8)),
                      (batch, points, (8, 1, 8))):
        m = _abi.Confocal()
        m.batch, m.num_points = b, p
        m.roi[0], m.roi[1], m.roi[2] = roi
        assert lib.l2o_confocal_unroll_supported(C.byref(cc), C.byref(m), eng._stream()) == 0
        assert lib.l2o_confocal_unroll_scratch_floats(C.byref(m), T) == 0
        rc = lib.l2o_confocal_unroll(C.byref(cc), vp(wpack), C.byref(m), ax, ast, None, None, None, asm, T, 1, vp(fx),
                                     vp(scratch), eng._stream())
        assert rc == _abi.L2O_ERR_UNSUPPORTED, (b, p, roi, rc)
        rc = lib.l2o_confocal_unroll_record(C.byref(cc), vp(wpack), C.byref(m), ax, ast, None, None, None, asm, T, 1, vp(fx),
                                            C.byref(h), vp(scratch), eng._stream())
        assert rc == _abi.L2O_ERR_UNSUPPORTED, (b, p, roi, rc)
    eng.synchronize()
    for t in [fx, scratch] + xs + sts + hg + hs:
        assert (eng.to_numpy(t) == -7.0).all()                               # nothing ran
    with pytest.raises(_abi.L2OUnsupported):
        eng.confocal_unroll(spec_of(O.DM_IDENTITY), wpack, _engine.ConfocalDesc(1025, 1, (8, 8, 8)),
                            [eng.zeros(1025) for _ in range(7)], sts[:7], [None] * 7, [None] * 7, [None] * 7,
                            [eng.zeros(1025) for _ in range(7)], T, 1, fx)


# ------------------------------------------------------------------------------------------------------------------
# 8. the DM evaluation driver
# ------------------------------------------------------------------------------------------------------------------
def test_evaluate_dm_driver_fused():
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "evaluate_dm.py"), "--problem", "confocal_microscopy_3d",
           "--num_steps", "20", "--seed", "3", "--confocal_fused", "1", "--unroll_len", "20"]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    m = re.search(r"Log Mean Final Error: (\S+)", out.stdout)
    assert m and math.isfinite(float(m.group(1))), out.stdout[-2000:]
