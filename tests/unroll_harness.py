"""One launch of the fused unroll through the C ABI, written once for the test modules (tests/test_pair_*.py,
tests/test_unroll_instantiations.py), and the vocabulary of their byte comparisons.

``prepare`` turns host arrays into a ``Launch``: every device tensor and scalar that HipEngine.unroll takes, the options it
runs under, whether it records, and whether fx comes from the fused epilogue (l2o_unroll_reduce) or from a separate
l2o_reduce_fx.  ``Launch.run`` allocates fx_part / fx / the history, calls, reports the kernel that ran, synchronises,
checks the status word and returns every output by name, on the device and on the host.  Which kernel SHOULD have run is
for the test to assert; where the inputs come from (seeds, scales, step0) is each module's own recipe, next to its cells.

Nothing here needs a GPU until a HipEngine is made: tests/test_pair_cells_cpu.py prepares the golden cells on the
OracleEngine."""
import collections
import dataclasses
import functools
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from helpers import spec_of
from open_l2o_amd import _abi

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def eng():
    """One HipEngine per test module (imported by name into the modules that use it)."""
    from open_l2o_amd._engine import HipEngine
    return HipEngine()


# ---- one launch ---------------------------------------------------------------------------------------------------------
Result = collections.namedtuple("Result", "dev host form dispatches variant")
# dev / host: {fx, fx_part, x, st (, m, v) (, hist_st, hist_g, hist_g_final (, hist_m, hist_v))} as device tensors / host
# arrays; form, dispatches: last_unroll_form(); variant: last_unroll_variant()


@dataclasses.dataclass
class Launch:
    eng: object
    params: dict                # the host weights wpack was packed from
    spec: object
    wpack: object
    pd: object                  # ProblemDesc
    T: int
    step0: int
    x: object
    st: object
    m: object                   # None: the net carries no moments
    v: object
    x0: object                  # with zero_state: the launch starts from x0 and zeros, whatever x / st / m / v hold
    zero_state: bool
    options: dict
    record: bool                # l2o_unroll_record's history
    fused_fx: bool              # fx by the unroll's epilogue (fx=) / by l2o_reduce_fx afterwards

    def then(self, step0, T=None):
        """The launch that continues on the same buffers from where this one stopped."""
        return dataclasses.replace(self, x0=None, zero_state=False, step0=step0, T=self.T if T is None else T)

    def hist_keys(self):
        return () if not self.record else ("st", "g", "g_final") + (("m", "v") if self.m is not None else ())

    def call(self, fx_part, fx=None, hist=None):
        """The call alone, under this launch's options: asynchronous, nothing allocated, nothing checked."""
        with _abi.option_scope(self.options):
            self.eng.unroll(self.spec, self.wpack, self.pd, self.x, self.st, self.m, self.v, self.T, self.step0, fx_part,
                            hist=hist, fx=fx, x0=self.x0, zero_state=self.zero_state)

    def run(self, check=True):
        """check = False: leave the status word to the caller (the injected-timeout tests)."""
        eng, T, B, N = self.eng, self.T, self.pd.B_local, self.pd.B_local * self.pd.D
        fx_part, fx = eng.zeros((T + 1) * B), eng.zeros(T + 1)
        rows = {"st": (T, eng.state_floats(B, self.pd.D)), "g": (T, N), "g_final": (N,), "m": (T, N), "v": (T, N)}
        hist = {k: eng.zeros(*rows[k]) for k in self.hist_keys()} or None
        self.call(fx_part, fx if self.fused_fx else None, hist)
        (form, dispatches), variant = eng.last_unroll_form(), eng.last_unroll_variant()
        if not self.fused_fx:
            eng.reduce_fx(fx_part, T + 1, B, self.pd.B_global, fx)
        eng.synchronize()
        if check:
            eng.check_unroll_status()                             # (raises on a partner timeout)
        dev = {"fx": fx, "fx_part": fx_part, "x": self.x, "st": self.st}
        if self.m is not None:
            dev.update(m=self.m, v=self.v)
        dev.update({"hist_" + k: t for k, t in (hist or {}).items()})
        return Result(dev, {k: eng.to_numpy(t) for k, t in dev.items()}, form, dispatches, variant)


def prepare(eng, cfg, params, pd, T, x0=None, x=None, state=None, m=None, v=None, step0=1, options=None, record=False,
            fused_fx=None, wpack=None):
    """Host arrays -> Launch.  x0: a fresh launch (x0, the zero state, zero moments for RNNProp; fx by the epilogue).
    x (with state as ((h1, c1), (h2, c2)), None: zeros; m, v): a launch that continues from them (fx by l2o_reduce_fx
    unless fused_fx says otherwise).  wpack: the packed params, where the caller keeps them across launches."""
    assert (x0 is None) != (x is None)
    B, D = pd.B_local, pd.D
    spec = spec_of(cfg)
    if wpack is None:
        wpack = eng.pack_weights(spec, params)
    if x0 is not None:
        x0, x, st = eng.tensor(x0.reshape(B, D)), eng.zeros(B, D), eng.state_alloc(B, D)
        m, v = (eng.zeros(B, D), eng.zeros(B, D)) if cfg.kind == "rnnprop" else (None, None)
    else:
        x = eng.tensor(x.reshape(B, D))
        st = eng.state_alloc(B, D) if state is None else eng.state_pack(*[eng.tensor(a) for hc in state for a in hc], B, D)
        m, v = (None if a is None else eng.tensor(a.reshape(B, D)) for a in (m, v))
    return Launch(eng, params, spec, wpack, pd, T, step0, x, st, m, v, x0, x0 is not None, dict(options or {}),
                  bool(record), (x0 is not None) if fused_fx is None else fused_fx)


# ---- bytes --------------------------------------------------------------------------------------------------------------
def sha(a):
    """SHA-256 of the raw bytes of an array or a tensor."""
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def assert_same_bytes(a, b, what):
    """Two {name: host array} hold the same names and, name by name, the same bytes."""
    assert a.keys() == b.keys(), what
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), "%s: %s differs" % (what, k)


class Golden:
    """tests/golden/<name>: {"cells": {cell id: {quantity: sha256}}, ...} recorded with the PARENT commit's library
    (scripts/record_pair_bytes.py)."""

    def __init__(self, name):
        self.path = os.path.join(GOLDEN_DIR, name)

    @functools.cached_property
    def data(self):
        with open(self.path) as f:
            return json.load(f)

    @property
    def cells(self):
        return self.data["cells"]

    def check_covers(self, ids):
        assert sorted(self.cells) == sorted(ids)

    def check(self, cell, got):
        """got: {quantity: sha256, host array or tensor} of one cell."""
        got = {k: a if isinstance(a, str) else sha(a) for k, a in got.items()}
        want = self.cells[cell]
        print("%s: %s" % (cell, " ".join("%s %s" % (k, got[k][:12]) for k in sorted(got))))
        assert sorted(got) == sorted(want), cell
        for k in sorted(got):
            assert got[k] == want[k], "%s: %s differs from the parent commit's bytes" % (cell, k)


# ---- the two-CU workspace (include/l2o_abi.h) ------------------------------------------------------------------------------
WS_STATUS, WS_SEQ, WS_FAULT = 0, 1, 2     # int32 words of the header: sticky status, launch sequence, the test hook's fault word
HEADER_BYTES = 192                        # the granule area follows the header


def ws_word(ws, i):
    """Word i of a workspace's header as an unsigned int (synchronises the host)."""
    return int(ws[4 * i:4 * i + 4].view(torch.int32).item()) & 0xffffffff


def set_ws_word(ws, i, value):
    ws[4 * i:4 * i + 4].view(torch.int32).fill_(value)


def assert_granules_zero(eng, B, D, what):
    """The exchange granules of the last launch -- [B][2 halves][2 parities][SQ = D] of 8 bytes, full tiles -- are all zero."""
    gran = eng._last_ws[HEADER_BYTES:HEADER_BYTES + B * 2 * 2 * D * 8]
    assert int(torch.count_nonzero(gran).item()) == 0, what
