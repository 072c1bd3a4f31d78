"""The FAST kernel of the two-CU unroll (csrc/l2o_unroll_pair.h) builds the bf16x3 operands of its packed gate GEMM in the step
loop with the scalar-residual form of bx::split5 (plain v_sub_f32 on the four components instead of v_pk_add_f32 on pairs:
beside MFMAs a packed fp32 instruction costs more than its issue slot); the gather kernel keeps the packed form.  The same
fp32 subtractions in the same order: the change must not move a bit of any output, and it must not reach the kernels that
keep the packed form.

Checked here: every cell below reproduces, byte for byte, what the commit BEFORE the scalar-residual form computed
(tests/golden/pair_split_bytes.json: the SHA-256 of the raw bytes of fx[0..T], of x_T and of the packed final LSTM state,
recorded with that commit's library on an MI355X by scripts/record_pair_bytes.py), and runs the kernel instantiation
it is meant to run (l2o_last_unroll_variant).

Every cell: T = 4, B = 8 (one group of 16 workgroups), a random non-zero initial LSTM state, fixed seeds.
"""
import numpy as np
import pytest

import unroll_harness as H
from helpers import ORACLE_CFGS, device_problem, make_params, make_problem, random_state
from open_l2o_amd import _abi
from unroll_harness import eng  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

T, B, STEP0 = 4, 8, 1
GOLDEN = H.Golden("pair_split_bytes.json")
GOLDEN_META = {"T": T, "B": B}

# id -> (net, kind, D, M, recording launch, exact gates, problem seed, expected template arguments)
# (the seeds are part of tests/golden/pair_split_bytes.json: a cell keeps its seed for good)
CELLS = {
    # CH 2, FAST prologue
    "quadratic_d32": ("dm", "quadratic", 32, None, False, False, 201, dict(CH=2, HIST=0, EXACT=0, FAST=1)),
    # CH 8, FAST: the flagship instantiation
    "quadratic_d128": ("dm", "quadratic", 128, None, False, False, 202, dict(CH=8, HIST=0, EXACT=0, FAST=1)),
    # CH 4, ragged: the kernel with the predicated gather (packed residuals, as before)
    "rastrigin_d40_logsign": ("dm_logsign", "rastrigin", 40, None, False, False, 203, dict(CH=4, HIST=0, EXACT=0, FAST=0)),
    # the 6-product core: must be untouched, the hash guards against collateral change
    "lasso_24x64_rnnprop": ("rnnprop", "lasso", 64, 24, False, False, 204, dict(CH=4, HIST=0, EXACT=0, FAST=0)),
    # the D = 128 cell on the recording kernel
    "quadratic_d128_recording": ("dm", "quadratic", 128, None, True, False, 202, dict(CH=8, HIST=1, EXACT=0, FAST=1)),
    # the D = 128 cell on the fp32-MFMA (exact gates) kernel: no split at all
    "quadratic_d128_exact": ("dm", "quadratic", 128, None, False, True, 202, dict(CH=8, HIST=0, EXACT=1, FAST=1)),
}


def prepare_cell(eng, name):
    net, kind, D, M, record, exact, seed, _ = CELLS[name]
    cfg = ORACLE_CFGS[net]
    prob, x0, arrays = make_problem(kind, B, D, seed=seed, M=M)
    rng = np.random.default_rng(seed + 50000)
    state0 = random_state(cfg, B * D, seed + 60000, scale=0.5)
    m = v = None
    if cfg.kind == "rnnprop":
        gs = float(np.abs(prob.grad(x0)).max())
        m = (rng.standard_normal((B, D)) * 0.3 * gs).astype(np.float32)
        v = (rng.uniform(0.1, 1.0, (B, D)) * gs * gs).astype(np.float32)
    return H.prepare(eng, cfg, make_params(cfg, seed=5, trained_like=True), device_problem(eng, arrays, B, D), T, x=x0,
                     state=state0, m=m, v=v, step0=STEP0, options={_abi.OPT_EXACT_GATES: 1} if exact else {}, record=record)


def run_cell(eng, name):
    """One launch of the cell -> {"fx", "x", "st": sha256 of the raw bytes}; it ran the kernel the cell names."""
    r = prepare_cell(eng, name).run()
    assert r.form == "k_unroll_pair", (name, r.form)
    assert r.variant == dict(CELLS[name][7], KR=0, NV=0), (name, r.variant)
    return {k: H.sha(r.host[k]) for k in ("fx", "x", "st")}


def golden_launches(eng):
    return {name: prepare_cell(eng, name) for name in CELLS}


def golden_cells(eng):
    return {name: run_cell(eng, name) for name in sorted(CELLS)}


def test_golden_covers_every_cell():
    GOLDEN.check_covers(CELLS)
    assert {k: GOLDEN.data[k] for k in GOLDEN_META} == GOLDEN_META


@pytest.mark.parametrize("name", sorted(CELLS))
def test_bytes_equal_the_parent_commit(eng, name):
    GOLDEN.check(name, run_cell(eng, name))


def test_cells_are_not_degenerate():
    """The guard is only worth something where the gate arithmetic reaches the hashed bytes: the exact-gates run of the
    D = 128 inputs must differ in bits from the bf16x3 run of the same inputs."""
    c = GOLDEN.cells
    for k in ("fx", "x", "st"):
        assert c["quadratic_d128"][k] != c["quadratic_d128_exact"][k], k
