"""The control paths of the two-CU unroll's step loop (csrc/l2o_unroll_pair_loop.h): the exit behind the final loss
evaluation (T = 0, 1, 4: no step at all, one, both parities of the granule buffers), the agent-scope publish of a pair that
is not confirmed on one XCD (L2O_OPT_PAIR_PLAIN_STORES = 0), the tanh output of the RNNProp nets, the gather kernel on a
ragged shape, the recording kernel with its second exit, and the partner-timeout bookkeeping (the injected fault).  Moving
any of them in or out of the straight-line step changes no operand and no operation of the arithmetic: every cell below
must reproduce, byte for byte, what the commit BEFORE the straight-line step computed.

tests/golden/pair_step_paths_bytes.json holds the SHA-256 of the raw bytes of fx_part, fx[0..T], x_T, the packed final
LSTM state, m / v (RNNProp) and the history buffers (recording launch), recorded with that commit's library on an MI355X
by scripts/record_pair_step_bytes.py.  Every cell also asserts the kernel instantiation it ran (l2o_last_unroll_variant).

Every cell: a random non-zero initial LSTM state, fixed seeds, B = 2 or 3 -- a launch group (8 problems x 2 halves) that
is not full, so the padding workgroups return at once.
"""
import hashlib
import json
import os

import numpy as np
import pytest

from helpers import ORACLE_CFGS, device_problem, lib_option, make_params, make_problem, random_state, spec_of
from open_l2o_amd import _abi

pytestmark = pytest.mark.gpu

STEP0 = 1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pair_step_paths_bytes.json")

# id -> (net, kind, D, M, B, T, recording launch, plain stores, problem seed, expected template arguments)
# (the seeds are part of tests/golden/pair_step_paths_bytes.json: a cell keeps its seed for good)
_Q32 = ("dm", "quadratic", 32, None, 3)
CELLS = {
    # CH 2, FAST: the final loss evaluation alone / one step / both parities
    "quadratic_d32_T0": _Q32 + (0, False, 1, 301, dict(CH=2, HIST=0, EXACT=0, FAST=1)),
    "quadratic_d32_T1": _Q32 + (1, False, 1, 301, dict(CH=2, HIST=0, EXACT=0, FAST=1)),
    "quadratic_d32_T4": _Q32 + (4, False, 1, 301, dict(CH=2, HIST=0, EXACT=0, FAST=1)),
    # the publish of a pair that may not use plain stores: agent scope, out of line
    "quadratic_d32_T4_agent_stores": _Q32 + (4, False, 0, 301, dict(CH=2, HIST=0, EXACT=0, FAST=1)),
    # RNNProp (fc + ELU preprocessing, tanh output): the out-of-line tanh; M != D, so the gather kernel, CH 2
    "lasso_16x32_rnnprop_T3": ("rnnprop", "lasso", 32, 16, 2, 3, False, 1, 302, dict(CH=2, HIST=0, EXACT=0, FAST=0)),
    # ragged: the gather kernel, CH 4, a cos term
    "rastrigin_d40_T3": ("dm", "rastrigin", 40, None, 2, 3, False, 1, 303, dict(CH=4, HIST=0, EXACT=0, FAST=0)),
    # the recording kernel: its exit lies behind the gradient at x_T
    "quadratic_d32_T3_recording": _Q32 + (3, True, 1, 301, dict(CH=2, HIST=1, EXACT=0, FAST=1)),
}
FAULT_CELL = "quadratic_d32_T4"


def _sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()


def _launch(eng, name, check=True):
    """One launch of the cell -> ({buffer: sha256 of its raw bytes}, kernel name, template arguments)."""
    import torch
    net, kind, D, M, B, T, record, plain, seed, _ = CELLS[name]
    cfg = ORACLE_CFGS[net]
    spec = spec_of(cfg)
    wpack = eng.pack_weights(spec, make_params(cfg, seed=5, trained_like=True))
    prob, x0, arrays = make_problem(kind, B, D, seed=seed, M=M)
    rng = np.random.default_rng(seed + 50000)
    state0 = random_state(cfg, B * D, seed + 60000, scale=0.5)
    pd = device_problem(eng, arrays, B, D)
    x = eng.tensor(x0.reshape(B, D))
    st = eng.state_pack(*[eng.tensor(a) for hc in state0 for a in hc], B, D)
    m = v = None
    rn = cfg.kind == "rnnprop"
    if rn:
        assert cfg.tanh_output
        gs = float(np.abs(prob.grad(x0)).max())
        m = eng.tensor((rng.standard_normal((B, D)) * 0.3 * gs).astype(np.float32))
        v = eng.tensor((rng.uniform(0.1, 1.0, (B, D)) * gs * gs).astype(np.float32))
    fx_part, fx = eng.zeros((T + 1) * B), eng.zeros(T + 1)
    hist = None
    if record:
        N = B * D
        hist = {"st": eng.zeros(T, st.numel()), "g": eng.zeros(T, N), "g_final": eng.zeros(N)}
        if rn:
            hist.update(m=eng.zeros(T, N), v=eng.zeros(T, N))
    with lib_option(_abi.OPT_PAIR_PLAIN_STORES, plain):
        eng.unroll(spec, wpack, pd, x, st, m, v, T, STEP0, fx_part, hist=hist)
        form, variant = eng.last_unroll_form()[0], eng.last_unroll_variant()
    eng.reduce_fx(fx_part, T + 1, B, B, fx)
    torch.cuda.synchronize()
    if check:
        eng.check_unroll_status()                                 # (raises on a partner timeout)
    out = {"fx_part": _sha(fx_part), "fx": _sha(fx), "x": _sha(x), "st": _sha(st)}
    if rn:
        out.update(m=_sha(m), v=_sha(v))
    if record:
        out.update({"hist_" + k: _sha(t) for k, t in hist.items()})
    return out, form, variant


def run_cell(eng, name):
    return _launch(eng, name)


@pytest.fixture(scope="module")
def eng():
    from open_l2o_amd._engine import HipEngine
    return HipEngine()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _assert_cell(got, form, variant, golden, name):
    assert form == "k_unroll_pair"
    assert variant == dict(CELLS[name][9], KR=0, NV=0)
    want = golden["cells"][name]
    print("%s: %s" % (name, " ".join("%s %s" % (k, got[k][:12]) for k in sorted(got))))
    assert sorted(got) == sorted(want)
    for k in sorted(got):
        assert got[k] == want[k], "%s: %s differs from the parent commit's bytes" % (name, k)


def test_golden_covers_every_cell(golden):
    assert sorted(golden["cells"]) == sorted(CELLS)


@pytest.mark.parametrize("name", sorted(CELLS))
def test_bytes_equal_the_parent_commit(eng, golden, name):
    got, form, variant = run_cell(eng, name)
    _assert_cell(got, form, variant, golden, name)


def test_cells_are_not_degenerate(golden):
    """The steps reach the hashed bytes (T = 0, 1, 4 differ), and so does the final LSTM state."""
    c = golden["cells"]
    for k in ("x", "st"):
        assert len({c["quadratic_d32_T%d" % t][k] for t in (0, 1, 4)}) == 3, k
    # the publish's scope is no arithmetic: the same bytes either way
    assert c["quadratic_d32_T4"] == c["quadratic_d32_T4_agent_stores"]


def test_injected_timeout_raises_status_and_the_next_launch_is_clean(eng, golden):
    """The fault word makes every workgroup give up on its partner: the launch returns, the sticky status word is raised
    and the host reports the timeout; on the re-initialised workspace the same launch gives the recorded bytes again."""
    import torch
    run_cell(eng, FAULT_CELL)                                     # (allocates / lays out the workspace for this shape)
    ws = eng._workspace
    eng.inject_unroll_fault()
    _, form, variant = _launch(eng, FAULT_CELL, check=False)
    torch.cuda.synchronize()
    assert form == "k_unroll_pair" and variant == dict(CELLS[FAULT_CELL][9], KR=0, NV=0)
    assert int(ws[0:4].view(torch.int32).item()) == 1
    with pytest.raises(_abi.L2OPartnerTimeout):
        eng.check_unroll_status()                                 # (clears the workspace, the fault word with it)
    assert int(ws[0:4].view(torch.int32).item()) == 0 and int(ws[8:12].view(torch.int32).item()) == 0
    got, form, variant = run_cell(eng, FAULT_CELL)
    _assert_cell(got, form, variant, golden, FAULT_CELL)
