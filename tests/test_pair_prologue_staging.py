"""The FAST prologue of the two-CU unroll (csrc/l2o_unroll_pair.h) brings the bf16 gate fragments into LDS once per
workgroup (one LDS-DMA copy; every wave reads its registers from it behind a drain and a barrier); a launch that starts
from the zero state must not let the contents of the state buffers reach its results; the epilogue kernel
k_combine_halves loads every partial of a lane up front and zeroes the exchange granules with 16-byte stores from the
waves that do not sum.  None of it changes a bit of any result.

Checked here through the C ABI, T = 3:
 * FAST kernel == the gather kernel (L2O_OPT_PAIR_FAST_LOAD = 0: its prologue loads per wave, straight into registers, and
   reads the state only when it must), byte for byte, over THREE launches on one workspace -- fresh (x0, zero state), continuing,
   fresh again -- with the state (and m / v) filled with NaN before each fresh launch: a fresh launch that used the state
   would carry the NaN into its results, a continuing launch that did not read it would differ from the gather's.
   Shapes the other files lack: the LogAndSign net at D = 64 (both input-weight rows), RNNProp at D = 128 (CH = 8, four
   fragment chunks in the stage), exact gates at D = 64 (the fp32 core has no fragment image: unaffected), B = 1 and
   B = 9 at D = 128 (one lane of the combine; two launch groups whose padding workgroups return in front of the barriers);
 * after every launch the status word is 0, the sequence word has advanced by one and the granule area is all zero;
 * k_combine_halves: fx and fx_part of four shapes equal the SHA-256 recorded with the PARENT commit's library on an MI355X
   (tests/golden/pair_combine_bytes.json, scripts/record_pair_bytes.py): two partials per problem and a second
   problem on a few lanes (D = 32, B = 70), one float4 (D = 64, B = 65), two float4 (D = 128, B = 9), and two chunk
   launches -- no fx in the kernel, the b0 offset (D = 32, B = 136).
"""
import numpy as np
import pytest

import unroll_harness as H
from helpers import ORACLE_CFGS, device_problem, lib_option, make_params, make_problem
from open_l2o_amd import _abi
from unroll_harness import eng  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

T = 3
GOLDEN = H.Golden("pair_combine_bytes.json")

# id -> (net, B, D, exact gates, problem seed)
CASES = {
    "dm_logsign_d64": ("dm_logsign", 3, 64, 0, 401),
    "rnnprop_d128": ("rnnprop", 3, 128, 0, 402),
    "exact_gates_d64": ("dm", 3, 64, 1, 403),
    "dm_d128_b1": ("dm", 1, 128, 0, 404),
    "dm_d128_b9": ("dm", 9, 128, 0, 405),
}
# id -> (B, D, dispatches of the unroll, problem seed)   (the seeds are part of the golden file)
COMBINE_CELLS = {
    "d32_b70": (70, 32, 1, 411),
    "d64_b65": (65, 64, 1, 412),
    "d128_b9": (9, 128, 1, 413),
    "d32_b136_two_chunks": (136, 32, 2, 414),
}


def _fresh_launch(eng, net, B, D, seed):
    """The net on Quadratic (full tiles) from x0 and the zero state, T = 3."""
    cfg = ORACLE_CFGS[net]
    _, x0, arrays = make_problem("quadratic", B, D, seed=seed)
    return H.prepare(eng, cfg, make_params(cfg, seed=5, trained_like=True), device_problem(eng, arrays, B, D), T, x0=x0)


def _three_launches(eng, case):
    """fresh, continuing, fresh again on the engine's workspace -> [dict of host arrays] x 3"""
    net, B, D, exact, seed = CASES[case]
    fresh = _fresh_launch(eng, net, B, D, seed)
    fast = _abi.get_option(_abi.OPT_PAIR_FAST_LOAD) == 1
    outs = []
    for i, launch in enumerate((fresh, fresh.then(1 + T), fresh)):
        if launch.zero_state:
            for t in (launch.st, launch.m, launch.v):
                if t is not None:
                    t.fill_(float("nan"))
        ws0 = eng._workspace                 # (the first launch of a shape may lay the workspace out anew: sequence 0)
        seq0 = 0 if ws0 is None else H.ws_word(ws0, H.WS_SEQ)
        r = launch.run()
        assert (r.form, r.dispatches) == ("k_unroll_pair", 1)
        assert r.variant == dict(CH=D // 16, HIST=0, EXACT=exact, FAST=int(fast), KR=0, NV=0)
        status, seq = H.ws_word(eng._last_ws, H.WS_STATUS), H.ws_word(eng._last_ws, H.WS_SEQ)
        assert status == 0, (case, i)
        assert seq == (seq0 + 1) & 0xffffffff or (i == 0 and seq == 1), (case, i, seq0, seq)
        H.assert_granules_zero(eng, B, D, (case, i))
        outs.append(r.host)
    return outs


@pytest.mark.parametrize("case", sorted(CASES))
def test_staged_prologue_equals_the_gather(eng, case):
    exact = CASES[case][3]
    with lib_option(_abi.OPT_EXACT_GATES, exact):
        fast = _three_launches(eng, case)
        with lib_option(_abi.OPT_PAIR_FAST_LOAD, 0):
            slow = _three_launches(eng, case)
    for i, what in enumerate(("fresh launch", "continuing launch", "second fresh launch")):
        for k in fast[i]:
            assert not np.isnan(fast[i][k]).any(), "%s, %s: NaN in %s" % (case, what, k)
        H.assert_same_bytes(fast[i], slow[i], "%s, %s, against the gather kernel" % (case, what))
    # a fresh launch does not depend on what the buffers held; the continuing one went somewhere else
    H.assert_same_bytes(fast[0], fast[2], case)
    assert (fast[0]["fx"] != fast[1]["fx"]).any() and (fast[0]["st"] != fast[1]["st"]).any()


def golden_launches(eng):
    return {name: _fresh_launch(eng, "dm", B, D, seed) for name, (B, D, _, seed) in COMBINE_CELLS.items()}


def run_combine_cell(eng, name):
    """One fresh launch of the cell (the DM net) -> {fx, fx_part: sha256 of the raw bytes}.
    With two chunk launches the kernel leaves fx to the caller: l2o_unroll_reduce finishes it (fx_part -> fx)."""
    B, D, dispatches, seed = COMBINE_CELLS[name]
    r = _fresh_launch(eng, "dm", B, D, seed).run()
    assert (r.form, r.dispatches) == ("k_unroll_pair", dispatches), (r.form, r.dispatches)
    assert r.variant == dict(CH=D // 16, HIST=0, EXACT=0, FAST=1, KR=0, NV=0)
    assert H.ws_word(eng._last_ws, H.WS_STATUS) == 0
    H.assert_granules_zero(eng, B, D, name)
    return {k: H.sha(r.host[k]) for k in ("fx", "fx_part")}


def golden_cells(eng):
    return {name: run_combine_cell(eng, name) for name in sorted(COMBINE_CELLS)}


def test_combine_golden_covers_every_cell():
    GOLDEN.check_covers(COMBINE_CELLS)


@pytest.mark.parametrize("name", sorted(COMBINE_CELLS))
def test_combine_bytes_equal_the_parent_commit(eng, name):
    GOLDEN.check(name, run_combine_cell(eng, name))
