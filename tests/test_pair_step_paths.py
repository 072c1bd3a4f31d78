"""The control paths of the two-CU unroll's step loop (csrc/l2o_unroll_pair_loop.h): the exit behind the final loss
evaluation (T = 0, 1, 4: no step at all, one, both parities of the granule buffers), the agent-scope publish of a pair that
is not confirmed on one XCD (L2O_OPT_PAIR_PLAIN_STORES = 0), the tanh output of the RNNProp nets, the gather kernel on a
ragged shape, the recording kernel with its second exit, and the partner-timeout bookkeeping (the injected fault).  Moving
any of them in or out of the straight-line step changes no operand and no operation of the arithmetic: every cell below
must reproduce, byte for byte, what the commit BEFORE the straight-line step computed.

tests/golden/pair_step_paths_bytes.json holds the SHA-256 of the raw bytes of fx_part, fx[0..T], x_T, the packed final
LSTM state, m / v (RNNProp) and the history buffers (recording launch), recorded with that commit's library on an MI355X
by scripts/record_pair_bytes.py.  Every cell also asserts the kernel instantiation it ran (l2o_last_unroll_variant).

Every cell: a random non-zero initial LSTM state, fixed seeds, B = 2 or 3 -- a launch group (8 problems x 2 halves) that
is not full, so the padding workgroups return at once.
"""
import numpy as np
import pytest

import unroll_harness as H
from helpers import ORACLE_CFGS, device_problem, make_params, make_problem, random_state
from open_l2o_amd import _abi
from unroll_harness import eng  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

STEP0 = 1
GOLDEN = H.Golden("pair_step_paths_bytes.json")

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


def prepare_cell(eng, name):
    net, kind, D, M, B, T, record, plain, seed, _ = CELLS[name]
    cfg = ORACLE_CFGS[net]
    prob, x0, arrays = make_problem(kind, B, D, seed=seed, M=M)
    rng = np.random.default_rng(seed + 50000)
    state0 = random_state(cfg, B * D, seed + 60000, scale=0.5)
    m = v = None
    if cfg.kind == "rnnprop":
        assert cfg.tanh_output
        gs = float(np.abs(prob.grad(x0)).max())
        m = (rng.standard_normal((B, D)) * 0.3 * gs).astype(np.float32)
        v = (rng.uniform(0.1, 1.0, (B, D)) * gs * gs).astype(np.float32)
    return H.prepare(eng, cfg, make_params(cfg, seed=5, trained_like=True), device_problem(eng, arrays, B, D), T, x=x0,
                     state=state0, m=m, v=v, step0=STEP0, options={_abi.OPT_PAIR_PLAIN_STORES: plain}, record=record)


def _launch(eng, name, check=True):
    """One launch of the cell -> Result; it ran the kernel the cell names."""
    r = prepare_cell(eng, name).run(check=check)
    assert r.form == "k_unroll_pair", (name, r.form)
    assert r.variant == dict(CELLS[name][9], KR=0, NV=0), (name, r.variant)
    return r


def run_cell(eng, name):
    """-> {buffer: sha256 of its raw bytes}: fx_part, fx, x, st, m / v (RNNProp), the history (recording launch)."""
    return {k: H.sha(a) for k, a in _launch(eng, name).host.items()}


def golden_launches(eng):
    return {name: prepare_cell(eng, name) for name in CELLS}


def golden_cells(eng):
    return {name: run_cell(eng, name) for name in sorted(CELLS)}


def test_golden_covers_every_cell():
    GOLDEN.check_covers(CELLS)


@pytest.mark.parametrize("name", sorted(CELLS))
def test_bytes_equal_the_parent_commit(eng, name):
    GOLDEN.check(name, run_cell(eng, name))


def test_cells_are_not_degenerate():
    """The steps reach the hashed bytes (T = 0, 1, 4 differ), and so does the final LSTM state."""
    c = GOLDEN.cells
    for k in ("x", "st"):
        assert len({c["quadratic_d32_T%d" % t][k] for t in (0, 1, 4)}) == 3, k
    # the publish's scope is no arithmetic: the same bytes either way
    assert c["quadratic_d32_T4"] == c["quadratic_d32_T4_agent_stores"]


def test_injected_timeout_raises_status_and_the_next_launch_is_clean(eng):
    """The fault word makes every workgroup give up on its partner: the launch returns, the sticky status word is raised
    and the host reports the timeout; on the re-initialised workspace the same launch gives the recorded bytes again."""
    run_cell(eng, FAULT_CELL)                                     # (allocates / lays out the workspace for this shape)
    ws = eng._workspace
    eng.inject_unroll_fault()
    _launch(eng, FAULT_CELL, check=False)                         # (synchronises: the launch came back)
    assert H.ws_word(ws, H.WS_STATUS) == 1
    with pytest.raises(_abi.L2OPartnerTimeout):
        eng.check_unroll_status()                                 # (clears the workspace, the fault word with it)
    assert H.ws_word(ws, H.WS_STATUS) == 0 and H.ws_word(ws, H.WS_FAULT) == 0
    GOLDEN.check(FAULT_CELL, run_cell(eng, FAULT_CELL))
