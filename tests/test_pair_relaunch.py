"""Launch after launch on ONE workspace of the two-CU unroll (csrc/l2o_unroll_pair.h), whose step loop has every lane
of a wave publish, poll and write its residual row (lanes gq = 2, 3 duplicate gq = 0, 1: the same value to the same
address) and whose loss terms are selects rather than exec-masked regions.

What is checked: back-to-back launches of two alternating instances on one workspace equal the same launches on a
freshly zeroed one bit for bit (granules, ws->seq and the loss partials re-arm between launches); ws->seq advances by
exactly one per launch; fx equals l2o_reduce_fx over fx_part bit for bit; the recording and the multi-launch (chunked)
forms; a launch that took the timeout path returns and the next one on the same workspace is clean."""
import pytest
import torch

import oracle as O
from helpers import device_problem, lib_option, make_params, make_problem, spec_of
from open_l2o_amd import _abi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from open_l2o_amd._engine import HipEngine
    return HipEngine()


def _seq(eng):
    return int(eng._last_ws[4:8].view(torch.int32).item()) & 0xffffffff


class _Case:
    """One problem instance (x0, data) at a shape of the two-CU form, launched through l2o_unroll_reduce from x0 and the
    zero state: every launch of it computes the same thing, whatever ran on the workspace before."""

    def __init__(self, eng, name, kind, B, D, T, seed, record=False):
        cfg = {"dm": O.DM_IDENTITY, "rnnprop": O.RNNPROP}[name]
        self.eng, self.B, self.D, self.T, self.rnnprop = eng, B, D, T, name == "rnnprop"
        self.spec = spec_of(cfg)
        self.wpack = eng.pack_weights(self.spec, make_params(cfg, seed=5, trained_like=True))
        _, x0, arrays = make_problem(kind, B, D, seed=seed)
        self.pd = device_problem(eng, arrays, B, D)
        self.x0 = eng.tensor(x0.reshape(B, D))
        self.record = record

    def run(self):
        e, B, D, T = self.eng, self.B, self.D, self.T
        x, st = e.zeros(B, D), e.state_alloc(B, D)
        m, v = (e.zeros(B, D), e.zeros(B, D)) if self.rnnprop else (None, None)
        fx_part, fx = e.zeros((T + 1) * B), e.zeros(T + 1)
        hist = None
        if self.record:
            N = B * D
            hist = {"st": e.zeros(T, st.numel()), "g": e.zeros(T, N), "g_final": e.zeros(N)}
            if self.rnnprop:
                hist.update(m=e.zeros(T, N), v=e.zeros(T, N))
        e.unroll(self.spec, self.wpack, self.pd, x, st, m, v, T, 1, fx_part, hist=hist, fx=fx, x0=self.x0,
                 zero_state=True)
        out = {"fx": fx, "fx_part": fx_part, "x": x, "st": st}
        if m is not None:
            out.update(m=m, v=v)
        if hist is not None:
            out.update({"hist_" + k: t for k, t in hist.items()})
        torch.cuda.synchronize()
        return {k: t.cpu().numpy() for k, t in out.items()}


def _fresh(eng):
    """Zero the engine's workspace (what l2o_unroll_workspace_init leaves; none yet: the next launch allocates a zeroed one)."""
    if eng._workspace is not None:
        eng._workspace.zero_()
        torch.cuda.synchronize()


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), "%s: %s differs" % (what, k)


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
        _assert_same(out, ref[i & 1], "launch %d" % i)
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
        _assert_same(out, ref, "recording launch %d" % i)
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
            _assert_same(out, ref, "chunked launch %d" % i)
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
    ws[8:12].view(torch.int32).fill_(1)
    c.run()                                                      # (run() synchronises: the launch came back)
    assert int(ws[0:4].view(torch.int32).item()) == 1            # the sticky status word
    assert _seq(eng) == (s0 + 1) & 0xffffffff                    # (the dead launch's epilogue still ran)
    ws[0:4].view(torch.int32).fill_(0)
    ws[8:12].view(torch.int32).fill_(0)
    out = c.run()
    assert int(ws[0:4].view(torch.int32).item()) == 0
    _assert_same(out, ref, "launch after the timeout")
