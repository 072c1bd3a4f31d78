"""The MLP Hessian-vector product's host side without a GPU: the ABI version stays 15 and include/l2o_mlp_hvp_abi.h is part
of the build id; the size query's range; the float32 reference engine's mlp_hvp against float64."""
import ctypes as C
import os

import numpy as np

from mlp_hvp_reference import HvpOracleEngine, hvp, shapes_of
from open_l2o_amd import _abi, _engine


def _lib():
    if not os.path.exists(_abi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _abi.lib()


def test_symbols():
    lib = _lib()
    assert lib.l2o_abi_version() == 15 == _abi.L2O_ABI_VERSION          # added after v15: test for the symbol
    assert _abi.source_build_id() == _abi.build_id()                    # (the new header is part of the build id)


def test_scratch_query_range():
    """Four [batch][32] arrays per hidden layer (a, Ra, d, Rd) and two for the logits; 0 outside l2o_mlp_deep_fg's range."""
    lib = _lib()
    c = _abi.MlpDeep()

    def ask(n_in, hidden, batch, n_out=10, layers=None):
        c.n_in, c.n_out, c.batch, c.activation, c.n_data = n_in, n_out, batch, 0, 100
        c.n_hidden_layers = len(hidden) if layers is None else layers
        for k in range(3):
            c.hidden[k] = int(hidden[k]) if k < len(hidden) else 0
        return int(lib.l2o_mlp_hvp_scratch_floats(C.byref(c)))
    assert ask(784, (20,), 128) == 128 * 32 * 6
    assert ask(37, (5, 32, 3), 65) == 65 * 32 * 14
    assert ask(1024, (32, 32, 32), 4096, n_out=16) == 4096 * 32 * 14
    for bad in (dict(n_in=1025, hidden=(20,), batch=8), dict(n_in=784, hidden=(33,), batch=8),
                dict(n_in=784, hidden=(20, 20, 20), batch=8, layers=4), dict(n_in=784, hidden=(), batch=8),
                dict(n_in=784, hidden=(20,), batch=0), dict(n_in=784, hidden=(20,), batch=8, n_out=17)):
        assert ask(**bad) == 0, bad


def test_reference_engine_mlp_hvp_vs_float64():
    """HvpOracleEngine.mlp_hvp (float32 torch; what the CPU runs of test_mlp_second_derivatives use) takes both descriptor
    classes and lands within 2e-6 of float64."""
    rng = np.random.default_rng(80)
    eng = HvpOracleEngine()
    for n_in, hidden, batch, act in ((37, (5,), 9, "sigmoid"), (23, (4, 6), 5, "relu")):
        images = ((rng.random((64, n_in)) < 0.2) * rng.random((64, n_in))).astype(np.float32)
        labels = rng.integers(0, 10, size=64).astype(np.int32)
        rows = rng.integers(0, 64, size=batch).astype(np.int32)
        shapes = shapes_of(n_in, hidden)
        ws = [(rng.standard_normal(sh) * 0.3).astype(np.float32) for sh in shapes]
        us = [rng.standard_normal(sh).astype(np.float32) for sh in shapes]
        common = dict(n_in=n_in, n_out=10, batch=batch, activation=0 if act == "sigmoid" else 1, images=eng.tensor(images),
                      labels=eng.int_tensor(labels))
        d = _engine.MlpDesc(n_hidden=hidden[0], **common) if len(hidden) == 1 else _engine.MlpDeepDesc(hidden=hidden, **common)
        outs = [eng.zeros(int(np.prod(sh))) for sh in shapes]
        eng.mlp_hvp(d, eng.int_tensor(rows), [eng.tensor(w) for w in ws], [eng.tensor(u) for u in us], outs)
        ref = hvp(ws, us, images, labels, rows, act)
        for o, r in zip(outs, ref):
            assert float(np.abs(o.numpy().reshape(r.shape) - r).max()) <= 2e-6 * float(np.abs(r).max())
