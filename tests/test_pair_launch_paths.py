"""The prologue of the two-CU unroll (csrc/l2o_unroll_pair.h) has two ways to fill a wave's copy of the matrix -- the
unpredicated loads of a problem of full tiles (M = D = 32 / 64 / 128: the kernel with the FAST prologue, which also issues
every other load of a launch up front behind one drain and publishes its half of the XCD handshake before that drain and
polls the partner's behind it; L2O_OPT_PAIR_FAST_LOAD, the default) and the kernel with the per-element predicated gather
that ragged shapes always run.

Checked here, T = 3, through the C ABI, every shape with a FRESH launch (x0 given, zero state: `restart`) and a SECOND
launch that continues from the first one's x / LSTM state / moments:
 * fast path == L2O_OPT_PAIR_FAST_LOAD = 0, byte for byte: x_T, fx[0..T], fx_part, the final state (and m / v, and every
   history array of the recording launch);
 * the ragged shapes equal what the commit BEFORE the fast path computed (tests/golden/pair_launch_paths_parent.npz,
   recorded with that commit's library on an MI355X), byte for byte;
 * fused == the step-granular path (l2o_problem_fg + l2o_cwlstm_step per step), within the bounds tests/test_hip_kernels.py
   uses for that comparison (rel fx < 1e-5, |dx| < 1e-5 max(1, |x|));
 * a matrix that is not 16-byte aligned takes the gather inside the FAST kernel and gives the same bytes;
 * the injected partner timeout (workspace fault word) still raises the sticky status in both kernels.
"""
import dataclasses

import numpy as np
import pytest

import oracle as O
import unroll_harness as H
from helpers import device_problem, lib_option, make_params, make_problem, max_abs, rel_err, spec_of
from open_l2o_amd import _abi
from unroll_harness import eng  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

T = 3
GOLDEN = H.GOLDEN_DIR + "/pair_launch_paths_parent.npz"

# id -> (net, kind, B, D, M, shared matrix, recording launch, x_scale, problem seed)
# (the seeds are part of tests/golden/pair_launch_paths_parent.npz: a case keeps its seed for good)
CASES = {
    "quadratic_d128_b3": ("dm", "quadratic", 3, 128, None, False, False, False, 102),  # full tiles, odd batch, padding blocks
    "quadratic_d32": ("dm", "quadratic", 3, 32, None, False, False, False, 104),       # CH = 2, full
    "quadratic_d64": ("dm", "quadratic", 3, 64, None, False, False, False, 105),       # CH = 4, full
    "quadratic_d24": ("dm", "quadratic", 3, 24, None, False, False, False, 103),       # ragged
    "quadratic_d100": ("dm", "quadratic", 3, 100, None, False, False, False, 101),     # ragged (config 4's width)
    "lasso_m48_d64": ("dm", "lasso", 3, 64, 48, False, False, False, 100),             # rows ragged, columns full
    "quadratic_d64_shared": ("dm", "quadratic", 5, 64, None, True, False, False, 106),  # one matrix for the batch
    "rnnprop_d64": ("rnnprop", "quadratic", 3, 64, None, False, False, False, 109),    # m / v loads in the merged drain
    "rastrigin_d128": ("dm", "rastrigin", 3, 128, None, False, False, False, 107),     # the C loads too
    "recording_d64": ("rnnprop", "quadratic", 3, 64, None, False, True, False, 108),   # HIST kernel (main translation unit)
    "quadratic_d64_xscale": ("dm", "quadratic", 3, 64, None, False, False, True, 110),  # the x_scale load (clamped address + select)
}
# (the step-granular kernels take no x_scale: that case is compared between the two fused kernels only)
STEP_CASES = sorted(c for c in CASES if not CASES[c][7])
RAGGED = ("quadratic_d24", "quadratic_d100", "lasso_m48_d64")


class _Setup:
    def __init__(self, eng, case, misalign=False):
        name, kind, B, D, M, shared, record, scaled, seed = CASES[case]
        self.eng, self.B, self.D, self.record = eng, B, D, record
        self.cfg = {"dm": O.DM_IDENTITY, "rnnprop": O.RNNPROP}[name]
        self.spec = spec_of(self.cfg)
        self.params = make_params(self.cfg, seed=5, trained_like=True)
        self.wpack = eng.pack_weights(self.spec, self.params)
        _, x0, arrays = make_problem(kind, B, D, seed=seed, M=M)
        if shared:
            arrays = dict(arrays, W=np.ascontiguousarray(arrays["W"][0]), w_shared=True)
        x_scale = np.exp(np.random.default_rng(seed + 1000).uniform(-0.5, 0.5, (B, D))).astype(np.float32) if scaled else None
        self.pd = device_problem(eng, arrays, B, D, x_scale=x_scale)
        if misalign:                                   # the same matrix 4 bytes off a 16-byte boundary
            W = self.pd.W
            buf = eng.zeros(W.numel() + 4)
            buf[1:1 + W.numel()].copy_(W.reshape(-1))
            self._keep = buf
            self.pd = dataclasses.replace(self.pd, W=buf[1:1 + W.numel()], x_scale=None)
            assert self.pd.W.data_ptr() % 16 == 4
        self.x0 = x0.reshape(B, D)

    def fresh(self):
        """The launch from x0 and the zero state, on buffers of its own."""
        return H.prepare(self.eng, self.cfg, self.params, self.pd, T, x0=self.x0, record=self.record, wpack=self.wpack)

    def fused(self):
        """Two launches on the two-CU kernel: fresh (x0, zero state), then continuing.  -> [dict of host arrays] x 2"""
        first = self.fresh()
        outs = []
        for launch in (first, first.then(1 + T)):
            r = launch.run()
            assert r.form == "k_unroll_pair"
            D = self.D
            full = self.pd.M == D and D in (32, 64, 128)       # (an unaligned matrix gathers INSIDE the FAST kernel)
            assert r.variant == dict(CH=(D + 31) // 32 * 2 if D <= 64 else 8, HIST=int(self.record), EXACT=0,
                                     FAST=int(full and _abi.get_option(_abi.OPT_PAIR_FAST_LOAD) == 1), KR=0, NV=0)
            outs.append(r.host)
        return outs

    def steps(self):
        """The same 2 T steps on the step-granular kernels.  -> (fx[0..2T], x after T steps, x after 2 T steps)"""
        e, B, D = self.eng, self.B, self.D
        xd, std, md, vd = e.tensor(self.x0), e.state_alloc(B, D), e.zeros(B, D), e.zeros(B, D)
        f, g = e.zeros(B), e.zeros(B, D)
        fx = e.zeros(2 * T + 1)
        b95 = float(np.float32(0.95))
        xs = []
        for t in range(2 * T):
            e.problem_fg(self.pd, xd, f, g)
            e.reduce_fx(f, 1, B, B, fx[t:t + 1])
            e.lstm_step(self.spec, self.wpack, g, md, vd, b95 ** (1 + t), b95 ** (1 + t), std, xd, B, D)
            if t + 1 == T:
                xs.append(e.to_numpy(xd).copy())
        e.problem_fg(self.pd, xd, f, None)
        e.reduce_fx(f, 1, B, B, fx[2 * T:2 * T + 1])
        xs.append(e.to_numpy(xd).copy())
        return e.to_numpy(fx), xs[0], xs[1]


_FAST = {}


def _fast_outputs(eng, case):
    """The default (fast-load) launches of a case, computed once and shared by the tests that compare against them."""
    if case not in _FAST:
        _FAST[case] = _Setup(eng, case).fused()
    return _FAST[case]


@pytest.mark.parametrize("case", sorted(CASES))
def test_fast_load_equals_predicated_gather(eng, case):
    fast = _fast_outputs(eng, case)
    with lib_option(_abi.OPT_PAIR_FAST_LOAD, 0):
        slow = _Setup(eng, case).fused()
    for i, what in enumerate(("fresh launch", "continuing launch")):
        H.assert_same_bytes(fast[i], slow[i], "%s, %s" % (case, what))
    assert np.all(np.isfinite(fast[1]["fx"])) and (fast[0]["fx"] != fast[1]["fx"]).any()


@pytest.mark.parametrize("case", STEP_CASES)
def test_fused_equals_step_granular_path(eng, case):
    fast = _fast_outputs(eng, case)
    s = _Setup(eng, case)
    fx, x_T, x_2T = s.steps()
    for i, (want_fx, want_x) in enumerate(((fx[:T + 1], x_T), (fx[T:], x_2T))):
        e_fx, e_x = rel_err(fast[i]["fx"], want_fx), max_abs(fast[i]["x"], want_x)
        print("%s launch %d: fused vs step path rel fx=%.3g |dx|=%.3g" % (case, i, e_fx, e_x))
        assert e_fx < 1e-5
        assert e_x < 1e-5 * max(1.0, float(np.abs(want_x).max()))


@pytest.mark.parametrize("case", RAGGED)
def test_ragged_shapes_equal_the_parent_commit(eng, case):
    """Ragged shapes take the predicated gather whatever the option says; x and fx of both launches equal the arrays the
    commit before the fast path computed, the final state its SHA-256."""
    gold = np.load(GOLDEN)
    for fast_load in (1, 0):
        with lib_option(_abi.OPT_PAIR_FAST_LOAD, fast_load):
            outs = _fast_outputs(eng, case) if fast_load else _Setup(eng, case).fused()
        for i, out in enumerate(outs):
            for k in ("x", "fx"):
                want = gold["%s/%d/%s" % (case, i, k)]
                assert out[k].tobytes() == want.tobytes(), (case, i, k, fast_load)
            digest = np.frombuffer(bytes.fromhex(H.sha(out["st"])), dtype=np.uint8)
            assert digest.tobytes() == gold["%s/%d/st_sha256" % (case, i)].tobytes(), (case, i, fast_load)


def test_unaligned_matrix_takes_the_gather(eng):
    case = "quadratic_d64"
    fast = _fast_outputs(eng, case)
    off = _Setup(eng, case, misalign=True).fused()
    for i in range(2):
        H.assert_same_bytes(fast[i], off[i], "matrix 4 bytes off, launch %d" % i)


@pytest.mark.parametrize("case", ["quadratic_d128_b3", "quadratic_d24"])
def test_injected_timeout_still_raises_status(eng, case):
    """The fault word makes every workgroup give up on its partner: the launch returns (bounded), the sticky status is
    raised, l2o_unroll_status reports the timeout -- and with both words cleared the next launch is clean."""
    ref = _fast_outputs(eng, case)
    s = _Setup(eng, case)
    s.fused()                                                    # (allocates / lays out the workspace for this shape)
    ws = eng._workspace
    eng.inject_unroll_fault()
    s.fresh().run(check=False)                                   # (synchronises: the launch came back)
    assert H.ws_word(ws, H.WS_STATUS) == 1
    with pytest.raises(_abi.L2OPartnerTimeout):
        eng.check_unroll_status()                                # (clears the workspace, the fault word with it)
    assert H.ws_word(ws, H.WS_STATUS) == 0 and H.ws_word(ws, H.WS_FAULT) == 0
    again = s.fused()
    for i in range(2):
        H.assert_same_bytes(again[i], ref[i], "%s after the timeout, launch %d" % (case, i))
