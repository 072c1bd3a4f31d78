"""problems.confocal_microscopy_3d on the MI355X: l2o_confocal_fg (csrc/l2o_confocal.h) against the float64 torch reference
(confocal_reference.py), the unroll of meta_loss over the problem against a float64 host unroll, the first-order
meta-gradient against helpers.oracle_meta_grad, and the DM evaluation driver on it.

Bounds (the project's, from test_training_gradient.py as test_lenet.py uses them): the loss within 1e-5 relative of float64;
every gradient array within max(GRAD_TOL = 5e-4 of its largest float64 entry, 3 x the float32 reference's own distance from
float64); carried state under max(CARRY_TOL, 3 x own).  Every measured error is printed next to the float32 reference's own."""
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
from helpers import ORACLE_CFGS, block_errors, make_params
from open_l2o_amd import _abi, _engine, meta, problems
from open_l2o_amd.session import Session
from test_meta_api import _net_config
from test_training_gradient import CARRY_TOL, GRAD_TOL, Trainer, _carried, split_carry

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def _device_fg(eng, roi, points, theta, sim, img=None, want_grad=True):
    batch = len(theta[0])
    d = _engine.ConfocalDesc(batch, points, tuple(roi), None if img is None else eng.tensor(np.asarray(img, np.float32)))
    th = [eng.tensor(a) for a in theta]
    sm = None if sim is None else [eng.tensor(a) for a in sim]
    grads = [eng.zeros(batch) for _ in theta] if want_grad else None
    loss = eng.zeros(1)
    eng.confocal_fg(d, th, sm, loss, grads)
    return eng.to_numpy(loss)[0], None if grads is None else [eng.to_numpy(g) for g in grads]


def _check_fg(eng, roi, points, theta, sim, img=None):
    """The kernel against float64 under the module's bounds; then bit-reproducibility and the forward-only loss."""
    ref = R.Confocal(roi, points, img)
    s64 = None if sim is None else [a.astype(np.float64) for a in sim]
    f64, g64 = ref.fg([a.astype(np.float64) for a in theta], s64)
    f32, g32 = ref.fg(theta, sim)
    got_f, got = _device_fg(eng, roi, points, theta, sim, img)
    print("loss", got_f, f64, "rel %.3e (float32 torch %.3e)" % (abs(got_f - f64) / abs(f64), abs(f32 - f64) / abs(f64)))
    names = R.trainable_names(points)
    failures = []
    if not abs(got_f - f64) <= 1e-5 * abs(f64):
        failures.append(("loss", got_f, f64))
    top = max(float(np.abs(a).max()) for a in g64)
    for nm, a, want, w32 in zip(names, got, g64, g32):
        err, bound = _bound(a.astype(np.float64), want, w32.astype(np.float64))
        scale = float(np.abs(want).max())
        print("%-16s err %.3e bound %.3e (float32 torch %.3e) of max %.3e: %.3e of it (float32 torch %.3e); the array is "
              "%.1e of the largest" % (nm, err, bound, float(np.abs(w32 - want).max()), scale, err / scale,
                                       float(np.abs(w32 - want).max()) / scale, scale / top))
        if not err <= bound:
            failures.append((nm, err, bound))
    assert not failures, failures
    f2, g2 = _device_fg(eng, roi, points, theta, sim, img)
    f3, _ = _device_fg(eng, roi, points, theta, sim, img, want_grad=False)
    assert f2 == got_f and f3 == got_f
    for a, b in zip(got, g2):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------------------------
# 1. one evaluation against float64
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("roi,batch,points", [((3, 2, 4), 5, 1), ((5, 7, 6), 3, 2), ((28, 28, 28), 32, 5),
                                              ((28, 28, 28), 1, 5), ((28, 28, 28), 37, 5), ((32, 32, 32), 2, 8)])
def test_fg_vs_float64(eng, roi, batch, points):
    """Simulation mode, raw parameters and simulation parameters in [0, 1]; unequal edges catch swapped axes and the
    per-axis prior ranges.  Also: a second call is bit-identical and the forward-only loss has the same bits.

    Measured on one MI355X, worst over the six cases: loss 1.2e-7 relative of float64 (float32 torch on the CPU: 6.7e-8).
    Gradient arrays, as a fraction of each array's largest float64 entry (float32 torch in brackets): at batch 3, 5, 32 and
    37 at most 8.6e-7 (6.8e-6).  The two cases with one or two rows have arrays that are tiny as a whole (a centre's
    gradient at a sign change, 1e-9 to 1e-7 of the largest array of the case), where a fraction of their own largest entry
    is large for any float32 evaluation: at batch 1 x_var_4 7.3e-5 (3.9e-2) and y_var_1 5.4e-5 (1.7e-4), inside GRAD_TOL;
    at (32, 32, 32) with batch 2 y_var_6 1.4e-3 (8.5e-3), an absolute 4.1e-7 on an array 1.1e-8 of the largest: the one
    array that rests on the 3 x clause (bound 2.6e-2); the next is z_var_6 at 5.8e-5 (4.0e-4)."""
    theta, sim = R.sample(batch, points, seed=batch + points)
    _check_fg(eng, roi, points, theta, sim)


def test_fg_off_range(eng):
    """Raw parameters in [-0.4, 1.4]: points outside the volume, sigma down to 1.2 (never at or below 0, which the formula
    does not guard).  For points far outside, the float32 reference's erf differences cancel; the kernel takes erfc
    differences there.

    Measured on one MI355X: loss 3.8e-8 relative (float32 torch the same); worst array y_var_2 at 4.0e-5 of its largest
    float64 entry (float32 torch 7.3e-5; an array 5.1e-7 the size of the largest), the next sigmaxy_var_2 at 3.6e-6
    (3.7e-6): with this draw every array is inside GRAD_TOL and the 3 x clause is not needed."""
    theta, sim = R.sample(4, 5, seed=7, lo=-0.4, hi=1.4)
    assert min(float(a.min()) for a in theta + sim) >= -0.4
    _check_fg(eng, (28, 28, 28), 5, theta, sim)


def test_fg_inference(eng):
    """The target is a supplied volume, positive (a ramp along each axis plus noise) with one all-zero row (the 1e-12 floor of l2_normalize); the
    reference reads it as [batch, iy, ix, iz], so another flattening in the kernel fails.

    Measured on one MI355X: loss 5.6e-8 relative (float32 torch 4.1e-8); gradient arrays at most 2.3e-7 of their largest
    float64 entry (float32 torch 1.4e-6)."""
    roi, batch, points = (5, 7, 6), 4, 2
    theta, _ = R.sample(batch, points, seed=11)
    iy, ix, iz = np.meshgrid(np.arange(7), np.arange(5), np.arange(6), indexing="ij")       # [Ry, Rx, Rz]
    img = 0.2 * np.random.default_rng(12).random((batch, 7, 5, 6)) + (iy / 7.0 + 0.5 * iz / 6.0 + 0.25 * ix / 5.0)[None]
    img = img.reshape(batch, -1).astype(np.float32)
    img[2] = 0.0
    _check_fg(eng, roi, points, theta, None, img)
    # the flattening matters to this check: against the volume read in the order [ix, iy, iz] the centres' gradients move
    # by far more than the bound
    swapped = np.ascontiguousarray(img.reshape(batch, 7, 5, 6).transpose(0, 2, 1, 3)).reshape(batch, -1)
    th64 = [a.astype(np.float64) for a in theta]
    g_a = R.Confocal(roi, points, img).fg(th64)[1]
    g_b = R.Confocal(roi, points, swapped).fg(th64)[1]
    moved = [float(np.abs(a - b).max() / np.abs(a).max()) for a, b in zip(g_a, g_b)]
    print("moved by the other flattening", moved)
    assert max(moved) > 10 * GRAD_TOL


def test_range_limits_return_unsupported_without_launching(eng):
    lib = _abi.lib()
    batch, points = 4, 2
    theta, sim = R.sample(batch, 9, seed=13)              # enough arrays for the widest refused shape
    th = [eng.tensor(a) for a in theta]
    sm = [eng.tensor(a) for a in sim]
    gs = [eng.zeros(batch) for _ in theta]
    ta = (C.c_void_p * len(th))(*[t.data_ptr() for t in th])
    sa = (C.c_void_p * len(sm))(*[t.data_ptr() for t in sm])
    ga = (C.c_void_p * len(gs))(*[t.data_ptr() for t in gs])
    scratch = eng.zeros(1 << 16)
    loss = eng.tensor(np.array([-7.0], np.float32))
    for b, p, roi in ((1025, points, (8, 8, 8)), (batch, 9, (8, 8, 8)), (batch, points, (8, 33, 8)), (batch, points, (33, 8, 8)),
                      (batch, points, (8, 8, 33)), (0, points, (8, 8, 8)), (batch, 0, (8, 8, 8)), (batch, points, (8, 1, 8))):
        m = _abi.Confocal()
        m.batch, m.num_points = b, p
        m.roi[0], m.roi[1], m.roi[2] = roi
        assert lib.l2o_confocal_scratch_floats(C.byref(m)) == 0
        rc = lib.l2o_confocal_fg(C.byref(m), ta, sa, C.c_void_p(loss.data_ptr()), ga, C.c_void_p(scratch.data_ptr()),
                                 eng._stream())
        assert rc == _abi.L2O_ERR_UNSUPPORTED, (b, p, roi, rc)
    assert eng.to_numpy(loss)[0] == -7.0 and all(not eng.to_numpy(g).any() for g in gs)      # nothing ran
    d = _engine.ConfocalDesc(1025, points, (8, 8, 8))
    with pytest.raises(_abi.L2OUnsupported):
        eng.confocal_fg(d, th[:13], sm[:13], loss, None)


# ------------------------------------------------------------------------------------------------------------------
# 2. the unroll: meta_loss over the problem against a float64 host unroll
# ------------------------------------------------------------------------------------------------------------------
def _fixed(batch, points, seed):
    theta, sim = R.sample(batch, points, seed)
    data = dict(zip(R.trainable_names(points), theta))
    data.update(zip(R.sim_names(points), sim))
    return theta, sim, data


@pytest.mark.parametrize("roi,batch,points,T", [((8, 8, 8), 4, 2, 20), ((28, 28, 28), 32, 5, 5)])
def test_unroll_vs_float64(eng, roi, batch, points, T):
    """Per-step fx within max(1e-5 relative, 3 x the float32 host unroll's own distance); the end state under _bound.

    Measured on one MI355X: fx within 2.9e-7 relative at every step of both cases; x_T within 2.6e-7 of each array's
    largest entry (float32 host unroll: 2.6e-7)."""
    theta, sim, data = _fixed(batch, points, seed=41)
    cfg = O.DM_IDENTITY
    params = make_params(cfg, seed=43, trained_like=True)
    meta.set_random_seed(44)
    problem = problems.confocal_microscopy_3d(batch_size=batch, num_points=points, ROI=list(roi), data=data)
    optimizer = meta.MetaOptimizer(**_net_config(cfg, params))
    ml = optimizer.meta_loss(problem, T)
    with Session() as sess:
        sess.run(ml.reset)
        v0 = [v.eval().reshape(-1) for v in optimizer.graph.x]
        res = optimizer.graph.execute({}, True)
    assert optimizer.graph.last_path == "steps"
    fx = np.asarray(res["fx_array"], np.float64)
    xT = [np.asarray(a, np.float64).reshape(-1) for a in res["x"]]
    ref = R.Confocal(roi, points)
    outs = {}
    for dt in (np.float64, np.float32):
        p = {m: {v: a.astype(dt) for v, a in d.items()} for m, d in params.items()}
        states = [tuple((h.astype(dt), c.astype(dt)) for h, c in O.net_initial_state(cfg, a.size)) for a in v0]
        sm = [a.astype(dt) for a in sim]
        fx_r, x_r, _ = O.unroll_multi(lambda vs, t, wg: ref.fg(vs, sm, wg), cfg, p, [a.astype(dt) for a in v0], states, T)
        outs[dt] = (np.asarray(fx_r, np.float64), [np.asarray(a, np.float64) for a in x_r])
    (fx64, x64), (fx32, x32) = outs[np.float64], outs[np.float32]
    assert fx.shape == fx64.shape == (T + 1,)
    for t in range(T + 1):
        print("fx", t, fx[t], fx64[t], fx32[t], "rel %.3e" % (abs(fx[t] - fx64[t]) / abs(fx64[t])))
        assert abs(fx[t] - fx64[t]) <= max(1e-5 * abs(fx64[t]), 3 * abs(fx32[t] - fx64[t])), (t, fx[t], fx64[t], fx32[t])
    for nm, g, w64, w32 in zip(R.trainable_names(points), xT, x64, x32):
        err, bound = _bound(g, w64, w32)
        print("x", nm, "err %.3e bound %.3e (float32 host unroll %.3e) of max %.3e" % (err, bound, float(np.abs(w32 - w64).max()),
                                                                                      float(np.abs(w64).max())))
        assert err <= bound, (nm, err, bound)


# ------------------------------------------------------------------------------------------------------------------
# 3. the meta-gradient: one first-order train step against helpers.oracle_meta_grad
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dm", "rnnprop"])
def test_meta_gradient_vs_float64(eng, name):
    """Measured on one MI355X: every meta-gradient block within 2.0e-7 of its largest entry (dm) and 2.2e-7 (rnnprop); the
    float32 oracle's own 2.5e-7 and 3.3e-7.  The carried x / state / moments after the step, under max(CARRY_TOL, 3 x own):
    at most 1.1e-6 of an array's largest entry (the h1 state of one variable, float32 oracle 8.7e-6), all inside
    CARRY_TOL."""
    T, batch, points, roi = 10, 4, 2, (8, 8, 8)
    theta, sim, data = _fixed(batch, points, seed=51)
    params = make_params(ORACLE_CFGS[name], seed=52, trained_like=True)
    meta.set_random_seed(53)
    tr = Trainer(eng, name, params, problems.confocal_microscopy_3d(batch_size=batch, num_points=points, ROI=list(roi),
                                                                    data=data), T)
    shapes = [tuple(v.shape) for v in tr.graph.x]
    assert shapes == [(batch, 1)] * (6 * points + 1)
    ref = R.Confocal(roi, points)
    tr.reset()
    snap = tr.snapshot()
    got = tr.train_step()
    assert tr.graph.last_path == "steps"
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
# 4. the DM evaluation driver
# ------------------------------------------------------------------------------------------------------------------
def test_evaluate_dm_driver():
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "evaluate_dm.py"), "--problem", "confocal_microscopy_3d",
           "--num_steps", "20", "--seed", "3"]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    m = re.search(r"Log Mean Final Error: (\S+)", out.stdout)
    assert m and math.isfinite(float(m.group(1))), out.stdout[-2000:]
