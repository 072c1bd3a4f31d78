"""Launch after launch on ONE workspace of the two-CU unroll (csrc/l2o_unroll_pair.h), whose step loop has every lane
of a wave publish, poll and write its residual row (lanes gq = 2, 3 duplicate gq = 0, 1: the same value to the same
address) and whose loss terms are selects rather than exec-masked regions.

What is checked: back-to-back launches of two alternating instances on one workspace equal the same launches on a
freshly zeroed one bit for bit (granules, ws->seq and the loss partials re-arm between launches); ws->seq advances by
exactly one per launch; fx equals l2o_reduce_fx over fx_part bit for bit; the recording and the multi-launch (chunked)
forms; a launch that took the timeout path returns and the next one on the same workspace is clean."""
import pytest

import oracle as O
import unroll_harness as H
from helpers import device_problem, lib_option, make_params, make_problem, spec_of
from open_l2o_amd import _abi
from unroll_harness import eng  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu


def _seq(eng):
    return H.ws_word(eng._last_ws, H.WS_SEQ)


class _Case:
    """One problem instance (x0, data) at a shape of the two-CU form, launched through l2o_unroll_reduce from x0 and the
    zero state: every launch of it computes the same thing, whatever ran on the workspace before."""

    def __init__(self, eng, name, kind, B, D, T, seed, record=False):
        self.cfg = {"dm": O.DM_IDENTITY, "rnnprop": O.RNNPROP}[name]
        self.eng, self.T, self.record = eng, T, record
        self.params = make_params(self.cfg, seed=5, trained_like=True)
        self.wpack = eng.pack_weights(spec_of(self.cfg), self.params)
        _, self.x0, arrays = make_problem(kind, B, D, seed=seed)
        self.pd = device_problem(eng, arrays, B, D)

    def run(self, check=True):
        """One launch on buffers of its own -> {name: host array}"""
        return H.prepare(self.eng, self.cfg, self.params, self.pd, self.T, x0=self.x0, record=self.record,
                         wpack=self.wpack).run(check).host


def _fresh(eng):
    """Zero the engine's workspace (what l2o_unroll_workspace_init leaves; none yet: the next launch allocates a zeroed one)."""
    if eng._workspace is not None:
        eng._workspace.zero_()
        eng.synchronize()


def _assert_fx_is_reduce_fx(eng, out, B, T):
    """The epilogue's fx is l2o_reduce_fx of its own fx_part, bit for bit (k_reduce_fx's summation order)."""
    fx = eng.zeros(T + 1)
    eng.reduce_fx(eng.tensor(out["fx_part"]), T + 1, B, B, fx)
    assert eng.to_numpy(fx).tobytes() == out["fx"].tobytes()


@pytest.mark.parametrize("name,kind,B,D", [("dm", "quadratic", 128, 128), ("rnnprop", "rastrigin", 40, 50),
                                           ("dm", "lasso", 24, 64)])
def test_back_to_back_launches_equal_fresh_workspace(eng, name, kind, B, D):
    T = 9
    cases = [_Case(eng, name, kind, B, D, T, seed=s) for s in (21, 22)]
    ref = []
    for c in cases:
        _fresh(eng)
        ref.append(c.run())
        assert eng.last_unroll_form()[0] == "k_unroll_pair"
    _fresh(eng)
    for i in range(5):                                           # A B A B A on one workspace, never re-zeroed
        s0 = _seq(eng)
        out = cases[i & 1].run()
        assert _seq(eng) == (s0 + 1) & 0xffffffff, "ws->seq must advance by exactly one per launch"
        H.assert_same_bytes(out, ref[i & 1], "launch %d" % i)
        _assert_fx_is_reduce_fx(eng, out, B, T)
    assert (ref[0]["fx"] != ref[1]["fx"]).any()                  # (the two instances differ: alternating them means something)


def test_recording_launches_equal_fresh_workspace(eng):
    B, D, T = 64, 96, 7
    c = _Case(eng, "rnnprop", "quadratic", B, D, T, seed=31, record=True)
    _fresh(eng)
    ref = c.run()
    assert eng.last_unroll_form()[0] == "k_unroll_pair"
    for i in range(3):
        s0 = _seq(eng)
        out = c.run()
        assert _seq(eng) == (s0 + 1) & 0xffffffff
        H.assert_same_bytes(out, ref, "recording launch %d" % i)
        _assert_fx_is_reduce_fx(eng, out, B, T)


def test_chunked_launches(eng):
    """More problems than one launch holds (L2O_OPT_ONE_LDS = 0: consecutive chunk launches of the two-CU kernel, fx by
    l2o_reduce_fx afterwards): every chunk launch advances ws->seq once and re-arms the workspace for the next."""
    B, D, T = 384, 128, 6
    with lib_option(_abi.OPT_ONE_LDS, 0):
        c = _Case(eng, "dm", "quadratic", B, D, T, seed=41)
        _fresh(eng)
        ref = c.run()
        form, launches = eng.last_unroll_form()
        assert form == "k_unroll_pair" and launches >= 2, (form, launches)
        for i in range(2):
            s0 = _seq(eng)
            out = c.run()
            assert _seq(eng) == (s0 + launches) & 0xffffffff
            H.assert_same_bytes(out, ref, "chunked launch %d" % i)
            _assert_fx_is_reduce_fx(eng, out, B, T)


def test_timeout_path_returns_and_next_launch_is_clean(eng):
    """The injected timeout (workspace fault word): the launch returns with the status raised and its epilogue still
    re-arms the workspace; with the status and the fault word cleared BY HAND -- the workspace otherwise untouched --
    the next launch equals the one on a fresh workspace."""
    B, D, T = 128, 128, 8
    c = _Case(eng, "dm", "quadratic", B, D, T, seed=51)
    _fresh(eng)
    ref = c.run()
    ws = eng._workspace
    s0 = _seq(eng)
    H.set_ws_word(ws, H.WS_FAULT, 1)
    c.run(check=False)                                           # (run() synchronises: the launch came back)
    assert H.ws_word(ws, H.WS_STATUS) == 1                       # the sticky status word
    assert _seq(eng) == (s0 + 1) & 0xffffffff                    # (the dead launch's epilogue still ran)
    H.set_ws_word(ws, H.WS_STATUS, 0)
    H.set_ws_word(ws, H.WS_FAULT, 0)
    out = c.run()
    assert H.ws_word(ws, H.WS_STATUS) == 0
    H.assert_same_bytes(out, ref, "launch after the timeout")
