"""The plain FAST kernels of the two-CU unroll (csrc/l2o_unroll_pair.h) issue only five of the twenty MFMAs of chunk L2B --
the chunk that carries h2(t-1) into layer 2 -- in the exchange window; seven go out behind barrier B2 and eight beside the
layer-1 gate exponentials (bx::finish; kPairL2bLate, kPairL2bB2 in csrc/l2o_lstm_bx3.h), and the split of h2 sits in the gaps
of chunk L1H.  The accumulation chain of every layer-2 accumulator keeps its order (bias quad as C of the first MFMA -> L2B
products 0..3 -> L2A products 0..3), so no bit of any result moves.

Checked here through the C ABI: fx[0..T], x_T and the final LSTM state of every cell equal the SHA-256 recorded with the
PARENT commit's library on an MI355X (tests/golden/pair_l2b_bytes.json, scripts/record_pair_bytes.py l2b).  The cells:
 * full tiles M = D = 32, 64, 128 (CH 2, 4, 8: one, two and four waves per half), B = 2, T = 3, for the nets dm (identity
   preprocessing) and dm_logsign (LogAndSign) on quadratic and rastrigin;
 * every cell starts from a random non-zero LSTM state, so step 0 already feeds a non-zero h2 through chunk L2B;
 * two cells with a per-coordinate x_scale != 1;
 * one ragged shape (D = 100), which must run the gather kernel, whose text is untouched.
Each cell asserts the kernel and the template arguments that ran (last_unroll_variant).
"""
import numpy as np
import pytest

import unroll_harness as H
from helpers import ORACLE_CFGS, device_problem, make_params, make_problem, random_state
from unroll_harness import eng  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

B, T, STEP0 = 2, 3, 1
GOLDEN = H.Golden("pair_l2b_bytes.json")


def _cells():
    """id -> (net, kind, D, scaled, problem seed, expected template arguments)   (the seeds are part of the golden file)"""
    cells, seed = {}, 700
    for net in ("dm", "dm_logsign"):
        for kind in ("quadratic", "rastrigin"):
            for D in (32, 64, 128):
                seed += 1
                cells["%s_%s_d%d" % (net, kind, D)] = (net, kind, D, False, seed, dict(CH=D // 16, HIST=0, EXACT=0, FAST=1))
    cells["dm_quadratic_d128_xscale"] = ("dm", "quadratic", 128, True, 721, dict(CH=8, HIST=0, EXACT=0, FAST=1))
    cells["dm_logsign_rastrigin_d64_xscale"] = ("dm_logsign", "rastrigin", 64, True, 722, dict(CH=4, HIST=0, EXACT=0, FAST=1))
    cells["dm_rastrigin_d100_ragged"] = ("dm", "rastrigin", 100, False, 723, dict(CH=8, HIST=0, EXACT=0, FAST=0))
    return cells


CELLS = _cells()


def initial_state(name):
    net, _, D, _, seed, _ = CELLS[name]
    return random_state(ORACLE_CFGS[net], B * D, seed + 60000, scale=0.5)


def prepare_cell(eng, name):
    net, kind, D, scaled, seed, _ = CELLS[name]
    cfg = ORACLE_CFGS[net]
    _, x0, arrays = make_problem(kind, B, D, seed=seed)
    x_scale = None
    if scaled:
        x_scale = np.random.default_rng(seed + 50000).uniform(0.5, 1.5, (B, D)).astype(np.float32)
        assert np.all(x_scale != 1.0)
    return H.prepare(eng, cfg, make_params(cfg, seed=5, trained_like=True), device_problem(eng, arrays, B, D, x_scale=x_scale),
                     T, x=x0, state=initial_state(name), step0=STEP0)


def run_cell(eng, name):
    """One launch of the cell -> {fx, x, st: sha256 of the raw bytes}; it ran the kernel the cell names."""
    r = prepare_cell(eng, name).run()
    assert (r.form, r.dispatches) == ("k_unroll_pair", 1), (name, r.form, r.dispatches)
    assert r.variant == dict(CELLS[name][5], KR=0, NV=0), (name, r.variant)
    for k in ("fx", "x", "st"):
        assert not np.isnan(r.host[k]).any(), "%s: NaN in %s" % (name, k)
    assert r.host["fx"].shape == (T + 1,)
    return {k: H.sha(r.host[k]) for k in ("fx", "x", "st")}


def golden_launches(eng):
    return {name: prepare_cell(eng, name) for name in CELLS}


def golden_cells(eng):
    return {name: run_cell(eng, name) for name in sorted(CELLS)}


def test_golden_covers_every_cell():
    GOLDEN.check_covers(CELLS)


@pytest.mark.parametrize("name", sorted(CELLS))
def test_bytes_equal_the_parent_commit(eng, name):
    GOLDEN.check(name, run_cell(eng, name))


@pytest.mark.parametrize("name", sorted(CELLS))
def test_initial_h2_is_nonzero(name):
    """Step 0 multiplies a non-zero h2 in chunk L2B: every unit of every coordinate."""
    (_, _), (h2, _) = initial_state(name)
    assert h2.shape == (B * CELLS[name][2], 20) and np.all(h2 != 0.0)


def test_cells_are_not_degenerate():
    """x_scale reaches the hashed bytes, and no two cells share a final state."""
    c = GOLDEN.cells
    assert len({c[name]["st"] for name in CELLS}) == len(CELLS)
    assert len({c[name]["fx"] for name in CELLS}) == len(CELLS)
