"""Confocal replicas without a GPU (replicas.Replicas over problems.confocal_microscopy_3d, form "rows"): on the
oracle-backed engine Replicas.train_step hands Adam the mean of the single-replica meta-gradients (form "chip": each graph's
own recording unroll); the form selection and its refusals; on an engine that claims l2o_confocal_unroll_multi, what `auto`
picks and how the launches are chunked; and the C ABI of include/l2o_confocal_multi_abi.h against the ctypes binding."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import confocal_reference as R
import oracle as O
from helpers import ORACLE_CFGS, make_params, spec_of
from open_l2o_amd import _abi, _engine, meta, meta_rnnprop_eval, problems
from open_l2o_amd.replicas import Replicas
from test_confocal_cpu import ConfocalOracleEngine
from test_meta_api import _net_config
from test_replica_training_cpu import (REL_MEAN, adam_first_step, capture_adam, check_rel, live_buffers, mean_of, net_key,
                                       replica_step)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def engine():
    eng = ConfocalOracleEngine()
    old = _engine._default_engine
    _engine.set_default_engine(eng)
    yield eng
    _engine.set_default_engine(old)


def make_replicas(name, n, T, batch=3, points=2, roi=(4, 5, 3), seed=5, shapes=None, fused=True):
    """n confocal replicas of one optimizer, each from its own draw; shapes: per replica (batch, points, roi) overrides;
    fused: one flag, or one per replica."""
    cfg = ORACLE_CFGS[name]
    params = make_params(cfg, seed=41, trained_like=True)
    meta.set_random_seed(seed)
    probs = []
    for j in range(n):
        b, p, r = shapes[j] if shapes else (batch, points, roi)
        theta, sim = R.sample(b, p, 100 + j)
        data = dict(zip(R.trainable_names(p), theta))
        data.update(zip(R.sim_names(p), sim))
        probs.append(problems.confocal_microscopy_3d(batch_size=b, num_points=p, ROI=list(r), data=data,
                                                     fused=fused[j] if isinstance(fused, (list, tuple)) else fused))
    if cfg.kind == "rnnprop":
        opt = meta_rnnprop_eval.MetaOptimizer(0.95, 0.95, **_net_config(cfg, params, key="rp"))
    else:
        opt = meta.MetaOptimizer(**_net_config(cfg, params))
    return Replicas(opt, probs, T)


def single_gradients(reps, feed):
    """Every replica's own meta-gradient from where it stands (its launch + _backward), then its inputs back."""
    key, T = net_key(reps), reps.len_unroll
    grads = []
    for g in reps.graphs:
        live = live_buffers(g)
        bak = [t.clone() for t in live]
        rec = {}
        g.launch(reps._feed(g, feed), True, record=rec)
        gr = g._backward(T, rec)
        grads.append({k: np.array(v, np.float64) for k, v in gr[key].items()})
        for t, b in zip(live, bak):
            t.copy_(b)
    return grads


@pytest.mark.parametrize("name", ["dm", "rnnprop"])
def test_train_step_is_the_mean_of_three_confocal_replicas(engine, name):
    T, n, lr = 3, 3, 1e-3
    reps = make_replicas(name, n, T)
    caps = capture_adam(reps)
    key = net_key(reps)
    reps.reset()
    feed = {reps.step: 1} if reps.graphs[0].rnnprop else {}
    singles = single_gradients(reps, feed)
    w0 = {m: {v: np.asarray(a, np.float32).copy() for v, a in d.items()} for m, d in reps.graphs[0].nets[key].variables.items()}
    out, got = replica_step(reps, feed, lr, caps)
    assert reps.last_form == "chip" and all(g.last_path == "steps" for g in reps.graphs)
    assert out["fx"].shape == (n,) and np.all(np.isfinite(out["fx"])) and len(reps.fx_arrays) == n
    np.testing.assert_allclose(out["loss"], np.mean([f.sum() for f in reps.fx_arrays]), rtol=1e-6)
    check_rel(got, mean_of(singles), REL_MEAN, "mean of the single-replica gradients")
    assert not np.allclose(singles[0][("lstm_1", "w_gates")], singles[1][("lstm_1", "w_gates")])   # (three different replicas)
    w1 = reps.graphs[0].nets[key].variables
    for (mod, var), g in got.items():
        np.testing.assert_allclose(w1[mod][var], adam_first_step(w0[mod][var], g.reshape(w0[mod][var].shape), lr),
                                   rtol=1e-6, atol=1e-9)
    # form="chip" asked for by name is the same path
    reps.train_step(feed, lr, form="chip")
    assert reps.last_form == "chip"


def test_forms_and_refusals_on_an_engine_without_the_kernel(engine):
    assert not hasattr(engine, "confocal_unroll_multi")
    reps = make_replicas("dm", 2, 2)
    reps.reset()
    assert reps.rows_supported() is False and reps.xcd_supported() is False
    with pytest.raises(_abi.L2OUnsupported):
        reps.run(form="rows")
    with pytest.raises(_abi.L2OUnsupported):
        reps.train_step({}, 1e-3, form="rows")
    with pytest.raises(_abi.L2OUnsupported):
        reps.run(form="xcd")
    with pytest.raises(_abi.L2OUnsupported):
        reps.train_step({}, 1e-3, form="xcd")
    with pytest.raises(ValueError):
        reps.run(form="wide")
    with pytest.raises(ValueError):
        reps.train_step({}, 1e-3, form="wide")
    fx = reps.run()
    assert reps.last_form == "chip" and fx.shape == (2,) and np.isfinite(fx).all()
    # replicas of two shapes cannot share a train step
    mixed = make_replicas("dm", 2, 2, shapes=[(3, 2, (4, 5, 3)), (3, 1, (4, 5, 3))])
    mixed.reset()
    with pytest.raises(ValueError):
        mixed.train_step({}, 1e-3)


class _Claiming(ConfocalOracleEngine):
    """An engine that claims the fused confocal kernels and records what the multi launch is given."""

    def __init__(self):
        super().__init__()
        self.asked, self.launches = [], []

    def confocal_unroll(self, *a, **kw):
        raise AssertionError("the single form must not run")

    def confocal_unroll_supported(self, spec, d):
        return 1

    def confocal_unroll_multi_supported(self, spec, d, n):
        self.asked.append(n)
        return 1 <= n <= 32

    def confocal_unroll_multi(self, spec, wpack, d, insts, T, step0, hists=None):
        self.launches.append(([id(i["fx"]) for i in insts], [i["xs"][0].data_ptr() for i in insts], T, step0, hists))


@pytest.fixture
def claiming():
    eng = _Claiming()
    old = _engine._default_engine
    _engine.set_default_engine(eng)
    yield eng
    _engine.set_default_engine(old)


def test_auto_picks_rows_on_an_engine_that_claims_the_kernel(claiming, monkeypatch):
    reps = make_replicas("dm", 2, 2)
    reps.reset()
    assert reps.rows_supported() is True
    reps.run()
    assert reps.last_form == "rows" and all(g.last_path == "confocal_multi" for g in reps.graphs)
    assert len(claiming.launches) == 1 and len(claiming.launches[0][0]) == 2 and claiming.launches[0][4] is None
    # one replica: auto stays on the graph's own launch (which this engine refuses to run: use the step path)
    one = make_replicas("dm", 1, 2)
    one.reset()
    monkeypatch.setattr(claiming, "confocal_unroll", lambda *a, **kw: None)
    n0 = len(claiming.launches)
    one.run()
    assert one.last_form == "chip" and len(claiming.launches) == n0
    one.run(form="rows")                                   # by name, one replica is a launch of one
    assert one.last_form == "rows" and len(claiming.launches) == n0 + 1
    # the disable switch
    monkeypatch.setenv("L2O_DISABLE_FUSED", "1")
    assert reps.rows_supported() is False
    reps.run()
    assert reps.last_form == "chip" and all(g.last_path == "steps" for g in reps.graphs)
    with pytest.raises(_abi.L2OUnsupported):
        reps.run(form="rows")
    monkeypatch.delenv("L2O_DISABLE_FUSED")
    # mixed shapes, or a replica with fused=False: chip
    mixed = make_replicas("dm", 2, 2, shapes=[(3, 2, (4, 5, 3)), (4, 2, (4, 5, 3))])
    mixed.reset()
    assert mixed.rows_supported() is False
    mixed.run()
    assert mixed.last_form == "chip"
    part = make_replicas("dm", 2, 2, fused=[True, False])
    part.reset()
    assert part.rows_supported() is False
    part.run()
    assert part.last_form == "chip"
    # the recording form: one history per instance, the train step's default for two replicas
    n0 = len(claiming.launches)
    reps.train_step({}, 1e-3)                              # (the stub writes no history: only the launch is looked at)
    assert reps.last_form == "rows" and len(claiming.launches) == n0 + 1
    hists = claiming.launches[-1][4]
    assert len(hists) == 2 and all(set(h) >= {"st", "g"} and len(h["g"]) == 13 for h in hists)


def test_seventy_replicas_go_out_as_32_32_6_in_order(claiming):
    reps = make_replicas("rnnprop", 70, 1, batch=1, points=1, roi=(2, 2, 2))
    reps.reset()
    reps.run({reps.step: 7})
    assert reps.last_form == "rows"
    assert [len(l[0]) for l in claiming.launches] == [32, 32, 6]
    assert all(l[2] == 1 and l[3] == 7 for l in claiming.launches)
    sent = [p for l in claiming.launches for p in l[1]]
    assert sent == [g.confocal_instance({g.step: 7})["xs"][0].data_ptr() for g in reps.graphs] and len(set(sent)) == 70
    assert claiming.asked and max(claiming.asked) <= 32
    assert len(reps.fx_arrays) == 70


C_PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "l2o_confocal_multi_abi.h"
int main(void) {
  printf("%d %d %d\n", (int)L2O_CONFOCAL_MAX_INSTANCES, (int)L2O_FORM_CONFOCAL_MULTI, (int)L2O_CONFOCAL_MAX_VARS);
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(l2o_confocal_instance), offsetof(l2o_confocal_instance, x),
         offsetof(l2o_confocal_instance, st), offsetof(l2o_confocal_instance, m), offsetof(l2o_confocal_instance, v),
         offsetof(l2o_confocal_instance, x_scale), offsetof(l2o_confocal_instance, sim), offsetof(l2o_confocal_instance, img),
         offsetof(l2o_confocal_instance, fx));
  return 0;
}
"""


def test_ctypes_struct_matches_the_header(tmp_path):
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(C_PROBE)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    rows = [[int(x) for x in ln.split()] for ln in subprocess.run([str(exe)], check=True, capture_output=True,
                                                                  text=True, timeout=60).stdout.splitlines()]
    assert rows[0] == [_abi.CONFOCAL_MAX_INSTANCES, 13, _abi.CONFOCAL_MAX_VARS] == [32, 13, 49]
    assert _abi.FORM_NAMES[13].startswith("k_cf_unroll") and 13 not in _abi.FORMS_WITH_EXCHANGE
    I = _abi.ConfocalInstance
    assert rows[1] == [C.sizeof(I), I.x.offset, I.st.offset, I.m.offset, I.v.offset, I.x_scale.offset, I.sim.offset,
                       I.img.offset, I.fx.offset]
    assert C.sizeof(I) == (6 * 49 + 2) * C.sizeof(C.c_void_p)


def test_symbols_build_id_and_scratch_query():
    """include/l2o_confocal_multi_abi.h is part of the build id on both sides; the size query and the predicate of its
    exports."""
    if not os.path.exists(_abi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _abi.lib()
    assert lib.l2o_abi_version() == 15
    assert _abi.source_build_id() == _abi.build_id()
    m = _abi.Confocal()
    m.batch, m.num_points = 5, 2
    m.roi[0], m.roi[1], m.roi[2] = 3, 2, 4
    one = lib.l2o_confocal_unroll_multi_scratch_floats(C.byref(m), 1, 7)
    assert one >= 8 * 5 + 2 * (10 * 49 + 3)                # fx_part [T + 1][batch] and the instance's pointer table
    assert lib.l2o_confocal_unroll_multi_scratch_floats(C.byref(m), 32, 7) == 32 * one
    cc = spec_of(O.DM_IDENTITY).to_c()
    assert lib.l2o_confocal_unroll_multi_supported(C.byref(cc), C.byref(m), 1, None) == 1
    assert lib.l2o_confocal_unroll_multi_supported(C.byref(cc), C.byref(m), 32, None) == 1
    for n in (0, 33, -1):
        assert lib.l2o_confocal_unroll_multi_scratch_floats(C.byref(m), n, 7) == 0, n
        assert lib.l2o_confocal_unroll_multi_supported(C.byref(cc), C.byref(m), n, None) == 0
    assert lib.l2o_confocal_unroll_multi_scratch_floats(C.byref(m), 2, -1) == 0
    for b, p, roi in ((0, 2, (3, 2, 4)), (1025, 2, (3, 2, 4)), (5, 0, (3, 2, 4)), (5, 9, (3, 2, 4)), (5, 2, (1, 2, 4)),
                      (5, 2, (3, 2, 33))):
        m.batch, m.num_points = b, p
        m.roi[0], m.roi[1], m.roi[2] = roi
        assert lib.l2o_confocal_unroll_multi_scratch_floats(C.byref(m), 2, 7) == 0, (b, p, roi)
