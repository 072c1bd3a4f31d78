"""The fused confocal unroll's host side without a GPU: the ``fused`` keyword of problems.confocal_microscopy_3d and its way
through util.get_config, the fall-back to the step-granular path on an engine without the kernel (bit-identical to
fused=False), the ctypes structs against include/l2o_abi.h (a tiny C program prints the header's sizes and offsets), the
new symbols and their size query, and the refusals that stay (second derivatives, a sharded graph)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import confocal_reference as R
import oracle as O
from helpers import make_params
from open_l2o_amd import _abi, _engine, meta, problems, util
from open_l2o_amd.session import Session
from test_confocal_cpu import ConfocalOracleEngine
from test_meta_api import _net_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def engine():
    eng = ConfocalOracleEngine()
    old = _engine._default_engine
    _engine.set_default_engine(eng)
    yield eng
    _engine.set_default_engine(old)


def test_fused_keyword_lands_in_hyper_and_goes_through_get_config(engine):
    meta.set_random_seed(1)
    for kw, want in (({}, False), ({"fused": False}, False), ({"fused": True}, True), ({"fused": 1}, True)):
        opt = meta.MetaOptimizer(**_net_config(O.DM_IDENTITY, make_params(O.DM_IDENTITY, seed=2, trained_like=True)))
        opt.meta_loss(problems.confocal_microscopy_3d(batch_size=3, num_points=1, ROI=[4, 4, 4], **kw), 1)
        hyper = opt.graph.terms[0].hyper
        assert hyper["fused"] is want, (kw, hyper)
    problem = util.get_config("confocal_microscopy_3d", problem_options={"fused": True, "batch_size": 3, "num_points": 1,
                                                                         "ROI": [4, 4, 4]})[0]
    opt = meta.MetaOptimizer(**_net_config(O.DM_IDENTITY, make_params(O.DM_IDENTITY, seed=2, trained_like=True)))
    opt.meta_loss(problem, 1)
    assert opt.graph.terms[0].hyper["fused"] is True and opt.graph.terms[0].hyper["batch_size"] == 3
    default = util.get_config("confocal_microscopy_3d")[0]
    opt = meta.MetaOptimizer(**_net_config(O.DM_IDENTITY, make_params(O.DM_IDENTITY, seed=2, trained_like=True)))
    opt.meta_loss(default, 1)
    assert opt.graph.terms[0].hyper["fused"] is False and opt.graph.terms[0].hyper["batch_size"] == 32


def _two_unrolls(fused, record):
    T, batch, points, roi = 3, 4, 2, (5, 4, 6)
    theta, sim = R.sample(batch, points, 8)
    data = dict(zip(R.trainable_names(points), theta))
    data.update(zip(R.sim_names(points), sim))
    meta.set_random_seed(10)
    problem = problems.confocal_microscopy_3d(batch_size=batch, num_points=points, ROI=list(roi), data=data, fused=fused)
    opt = meta.MetaOptimizer(**_net_config(O.DM_IDENTITY, make_params(O.DM_IDENTITY, seed=9, trained_like=True)))
    out = []
    if record:
        ms = opt.meta_minimize(problem, T, learning_rate=1e-3)
        with Session() as sess:
            sess.run(ms.reset)
            for _ in range(2):
                out.append(np.asarray(sess.run([ms.fx, ms.update, ms.step])[0]))
            out += [v.eval().copy() for v in opt.graph.x]
    else:
        ml = opt.meta_loss(problem, T)
        with Session() as sess:
            sess.run(ml.reset)
            for _ in range(2):
                fx, x, _ = sess.run([ml.fx, ml.x, ml.update])
                out += [np.asarray(fx)] + [np.asarray(a).copy() for a in x]
    return opt.graph.last_path, out


@pytest.mark.parametrize("record", [False, True])
def test_engine_without_the_kernel_falls_back_to_steps_bit_for_bit(engine, record):
    """The oracle-backed engine has no confocal_unroll: fused=True runs the step-granular path and computes exactly what
    fused=False computes (plain unrolls and training steps)."""
    assert not hasattr(engine, "confocal_unroll")
    path_f, got = _two_unrolls(True, record)
    n_fused = engine.calls.count("confocal_fg")
    path_0, want = _two_unrolls(False, record)
    assert path_f == "steps" and path_0 == "steps"
    assert engine.calls.count("confocal_fg") == 2 * n_fused > 0
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and np.array_equal(a, b)


def test_disable_switch_and_predicate_conditions(engine, monkeypatch):
    """_confocal_unroll_ok on an engine that claims the kernel: true for one fused term of weight 1 on one LSTM net;
    false with L2O_DISABLE_FUSED, with fused=False, and when the library refuses the shape."""
    asked = []

    def graph_of(**kw):
        meta.set_random_seed(3)
        opt = meta.MetaOptimizer(**_net_config(O.DM_IDENTITY, make_params(O.DM_IDENTITY, seed=4, trained_like=True)))
        opt.meta_loss(problems.confocal_microscopy_3d(batch_size=3, num_points=1, ROI=[4, 4, 4], **kw), 1)
        g = opt.graph
        g._ensure_init()
        return g
    engine.confocal_unroll = lambda *a, **kw: None
    engine.confocal_unroll_supported = lambda spec, d: asked.append((tuple(spec.layers), d.batch, d.num_points, d.roi)) or 1
    g = graph_of(fused=True)
    states = [s.state for s in g.slots]
    assert g._confocal_unroll_ok(g.slots, states) is True
    assert asked == [((20, 20), 3, 1, (4, 4, 4))]
    monkeypatch.setenv("L2O_DISABLE_FUSED", "1")
    assert g._confocal_unroll_ok(g.slots, states) is False
    monkeypatch.delenv("L2O_DISABLE_FUSED")
    engine.confocal_unroll_supported = lambda spec, d: 0
    assert g._confocal_unroll_ok(g.slots, states) is False
    engine.confocal_unroll_supported = lambda spec, d: 1
    g0 = graph_of()
    assert g0._confocal_unroll_ok(g0.slots, [s.state for s in g0.slots]) is False


C_PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "l2o_confocal_unroll_abi.h"
int main(void) {
  printf("%d %d\n", (int)L2O_CONFOCAL_MAX_VARS, (int)L2O_FORM_CONFOCAL_UNROLL);
  printf("%zu %zu %zu %zu %zu\n", sizeof(l2o_confocal_hist), offsetof(l2o_confocal_hist, st), offsetof(l2o_confocal_hist, g),
         offsetof(l2o_confocal_hist, m), offsetof(l2o_confocal_hist, v));
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(l2o_confocal), offsetof(l2o_confocal, batch), offsetof(l2o_confocal, num_points),
         offsetof(l2o_confocal, roi), offsetof(l2o_confocal, inference), offsetof(l2o_confocal, flags), offsetof(l2o_confocal, img));
  return 0;
}
"""


def test_ctypes_structs_match_the_header(tmp_path):
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(C_PROBE)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    rows = [[int(x) for x in ln.split()] for ln in subprocess.run([str(exe)], check=True, capture_output=True,
                                                                  text=True, timeout=60).stdout.splitlines()]
    assert rows[0] == [_abi.CONFOCAL_MAX_VARS, 12] and _abi.FORM_NAMES[12].startswith("k_cf_unroll")
    H = _abi.ConfocalHist
    assert rows[1] == [C.sizeof(H), H.st.offset, H.g.offset, H.m.offset, H.v.offset]
    assert C.sizeof(H) == 4 * 49 * C.sizeof(C.c_void_p)
    M = _abi.Confocal
    assert rows[2] == [C.sizeof(M), M.batch.offset, M.num_points.offset, M.roi.offset, M.inference.offset, M.flags.offset,
                       M.img.offset]


def test_symbols_and_scratch_query():
    """The ABI version the exports of include/l2o_confocal_unroll_abi.h were added under, and their size query."""
    if not os.path.exists(_abi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _abi.lib()
    assert lib.l2o_abi_version() == 15                     # added after v15: test for the symbol
    assert 12 not in _abi.FORMS_WITH_EXCHANGE               # no workgroup waits for another
    m = _abi.Confocal()
    m.batch, m.num_points = 5, 2
    m.roi[0], m.roi[1], m.roi[2] = 3, 2, 4
    n = lib.l2o_confocal_unroll_scratch_floats(C.byref(m), 7)
    assert n >= 8 * 5 + 2 * 4 * 49                          # fx_part [T + 1][batch] and the history pointer table
    for b, p, roi in ((0, 2, (3, 2, 4)), (1025, 2, (3, 2, 4)), (5, 0, (3, 2, 4)), (5, 9, (3, 2, 4)), (5, 2, (1, 2, 4)),
                      (5, 2, (3, 2, 33))):
        m.batch, m.num_points = b, p
        m.roi[0], m.roi[1], m.roi[2] = roi
        assert lib.l2o_confocal_unroll_scratch_floats(C.byref(m), 7) == 0, (b, p, roi)


def test_refusals_stay_with_fused(engine, monkeypatch):
    """second_derivatives=True and a sharded graph still refuse the problem, fused or not."""
    problem = problems.confocal_microscopy_3d(batch_size=4, num_points=2, ROI=[5, 4, 6], fused=True)
    opt = meta.MetaOptimizer(**_net_config(O.DM_IDENTITY, make_params(O.DM_IDENTITY, seed=13, trained_like=True)))
    with pytest.raises(NotImplementedError, match=r"second_derivatives.*confocal_microscopy_3d"):
        opt.meta_minimize(problem, 2, learning_rate=1e-3, second_derivatives=True)
    from open_l2o_amd import _graph_core
    monkeypatch.setattr(_graph_core, "_EMULATED_WORLD", (0, 2))
    with pytest.raises(NotImplementedError, match=r"confocal_microscopy_3d.*sharded"):
        opt.meta_loss(problem, 2)
