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
   (tests/golden/pair_combine_bytes.json, scripts/record_pair_combine_bytes.py): two partials per problem and a second
   problem on a few lanes (D = 32, B = 70), one float4 (D = 64, B = 65), two float4 (D = 128, B = 9), and two chunk
   launches -- no fx in the kernel, the b0 offset (D = 32, B = 136).
"""
import hashlib
import json
import os

import numpy as np
import pytest

from helpers import ORACLE_CFGS, device_problem, lib_option, make_params, make_problem, spec_of
from open_l2o_amd import _abi

pytestmark = pytest.mark.gpu

T = 3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pair_combine_bytes.json")
HEADER_BYTES = 192                    # the workspace header (include/l2o_abi.h); the granule area follows it

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


@pytest.fixture(scope="module")
def eng():
    from open_l2o_amd._engine import HipEngine
    return HipEngine()


def _granule_bytes(B, D):
    return B * 2 * 2 * D * 8           # [B][2 halves][2 parities][SQ = D] granules of 8 bytes (full tiles)


def _header(eng):
    import torch
    ws = eng._last_ws
    status, seq = (int(v) for v in ws[0:8].view(torch.int32).cpu())
    return status, seq & 0xffffffff


def _three_launches(eng, case):
    """fresh, continuing, fresh again on the engine's workspace -> [dict of host arrays] x 3"""
    import torch
    net, B, D, exact, seed = CASES[case]
    cfg = ORACLE_CFGS[net]
    spec = spec_of(cfg)
    wpack = eng.pack_weights(spec, make_params(cfg, seed=5, trained_like=True))
    _, x0, arrays = make_problem("quadratic", B, D, seed=seed)
    pd = device_problem(eng, arrays, B, D)
    x0d = eng.tensor(x0.reshape(B, D))
    rn = cfg.kind == "rnnprop"
    x, st = eng.zeros(B, D), eng.state_alloc(B, D)
    m, v = (eng.zeros(B, D), eng.zeros(B, D)) if rn else (None, None)
    fast = _abi.get_option(_abi.OPT_PAIR_FAST_LOAD) == 1
    outs = []
    for launch, fresh in enumerate((True, False, True)):
        fx_part, fx = eng.zeros((T + 1) * B), eng.zeros(T + 1)
        if fresh:
            for t in (st, m, v):
                if t is not None:
                    t.fill_(float("nan"))
        ws0 = eng._workspace                 # (the first launch of a shape may lay the workspace out anew: sequence 0)
        seq0 = 0 if ws0 is None else int(ws0[4:8].view(torch.int32).item()) & 0xffffffff
        if fresh:
            eng.unroll(spec, wpack, pd, x, st, m, v, T, 1, fx_part, fx=fx, x0=x0d, zero_state=True)
        else:
            eng.unroll(spec, wpack, pd, x, st, m, v, T, 1 + T, fx_part, fx=fx)
        assert eng.last_unroll_form() == ("k_unroll_pair", 1)
        assert eng.last_unroll_variant() == dict(CH=D // 16, HIST=0, EXACT=exact, FAST=int(fast), KR=0, NV=0)
        torch.cuda.synchronize()
        status, seq = _header(eng)
        assert status == 0, (case, launch)
        assert seq == (seq0 + 1) & 0xffffffff or (launch == 0 and seq == 1), (case, launch, seq0, seq)
        gran = eng._last_ws[HEADER_BYTES:HEADER_BYTES + _granule_bytes(B, D)]
        assert int(torch.count_nonzero(gran).item()) == 0, (case, launch)
        out = {"fx": fx, "fx_part": fx_part, "x": x, "st": st}
        if rn:
            out.update(m=m, v=v)
        outs.append({k: t.cpu().numpy().copy() for k, t in out.items()})
    return outs


@pytest.mark.parametrize("case", sorted(CASES))
def test_staged_prologue_equals_the_gather(eng, case):
    exact = CASES[case][3]
    with lib_option(_abi.OPT_EXACT_GATES, exact):
        fast = _three_launches(eng, case)
        with lib_option(_abi.OPT_PAIR_FAST_LOAD, 0):
            slow = _three_launches(eng, case)
    for i, what in enumerate(("fresh launch", "continuing launch", "second fresh launch")):
        assert fast[i].keys() == slow[i].keys()
        for k in fast[i]:
            assert not np.isnan(fast[i][k]).any(), "%s, %s: NaN in %s" % (case, what, k)
            assert fast[i][k].tobytes() == slow[i][k].tobytes(), "%s, %s: %s differs from the gather kernel's" % (case, what, k)
    # a fresh launch does not depend on what the buffers held; the continuing one went somewhere else
    for k in fast[0]:
        assert fast[0][k].tobytes() == fast[2][k].tobytes(), (case, k)
    assert (fast[0]["fx"] != fast[1]["fx"]).any() and (fast[0]["st"] != fast[1]["st"]).any()


def _sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()


def run_combine_cell(eng, name):
    """One fresh launch of the cell (the DM net, Quadratic, full tiles) -> {fx, fx_part: sha256 of the raw bytes}.
    With two chunk launches the kernel leaves fx to the caller: l2o_unroll_reduce finishes it (fx_part -> fx)."""
    import torch
    B, D, dispatches, seed = COMBINE_CELLS[name]
    cfg = ORACLE_CFGS["dm"]
    spec = spec_of(cfg)
    wpack = eng.pack_weights(spec, make_params(cfg, seed=5, trained_like=True))
    _, x0, arrays = make_problem("quadratic", B, D, seed=seed)
    pd = device_problem(eng, arrays, B, D)
    x, st = eng.zeros(B, D), eng.state_alloc(B, D)
    fx_part, fx = eng.zeros((T + 1) * B), eng.zeros(T + 1)
    eng.unroll(spec, wpack, pd, x, st, None, None, T, 1, fx_part, fx=fx, x0=eng.tensor(x0.reshape(B, D)), zero_state=True)
    assert eng.last_unroll_form() == ("k_unroll_pair", dispatches), eng.last_unroll_form()
    assert eng.last_unroll_variant() == dict(CH=D // 16, HIST=0, EXACT=0, FAST=1, KR=0, NV=0)
    torch.cuda.synchronize()
    assert _header(eng)[0] == 0
    gran = eng._last_ws[HEADER_BYTES:HEADER_BYTES + _granule_bytes(B, D)]
    assert int(torch.count_nonzero(gran).item()) == 0, name
    return {"fx": _sha(fx), "fx_part": _sha(fx_part)}


def test_combine_golden_covers_every_cell():
    with open(GOLDEN) as f:
        assert sorted(json.load(f)["cells"]) == sorted(COMBINE_CELLS)


@pytest.mark.parametrize("name", sorted(COMBINE_CELLS))
def test_combine_bytes_equal_the_parent_commit(eng, name):
    with open(GOLDEN) as f:
        want = json.load(f)["cells"][name]
    got = run_combine_cell(eng, name)
    print("%s: %s" % (name, " ".join("%s %s" % (k, got[k][:12]) for k in sorted(got))))
    assert sorted(got) == sorted(want)
    for k in sorted(got):
        assert got[k] == want[k], "%s: %s differs from the parent commit's bytes" % (name, k)
