"""Chunk L2A of the two-CU unroll (csrc/l2o_unroll_pair.h) -- the twenty MFMAs that carry h1(t) into layer 2 -- and the layer-2
gate block behind it (bx::finish in csrc/l2o_lstm_bx3.h) are the one stretch of a step in which every instruction waits for the
one before.  Any change to where those MFMAs and the gates' first-stage exponentials are issued must keep the accumulation
chain of every layer-2 accumulator (bias quad -> L2B products 0..3 -> L2A products 0..3) and every operand of the gates, so no
bit of any result may move.

Checked here through the C ABI: fx[0..T], x_T and the final LSTM state of every cell (and the recorded history of the
recording cell) equal the SHA-256 recorded with the PARENT commit's library on an MI355X (tests/golden/pair_l2a_bytes.json,
scripts/record_pair_bytes.py l2a).  The cells:
 * full tiles M = D = 32, 64, 128 (CH 2, 4, 8), B = 2, T = 3, for the nets dm and dm_logsign on quadratic and rastrigin;
 * every cell starts from a random non-zero LSTM state with a non-zero c2, so step 0 already runs non-trivial layer-2 gates
   on an accumulator that carries a non-zero L2B part;
 * one cell whose layer-2 gate weights are scaled up so that, at EVERY step, every one of the four layer-2 gates sees
   negative and positive pre-activations (asserted on the host with the oracle): the -|x| exponentials and the copysigns
   run on both signs;
 * T = 1 and T = 2: the first and the last trip of the step loop and the final loss evaluation behind it;
 * a ragged shape (D = 100: the gather kernel), a recording cell and dm_logsign at CH = 8, whose kernels keep the
   placement they had (kPairL2bLate is 0 for them) -- they are held to their parent hashes like the rest.
Each cell asserts the kernel and the template arguments that ran (last_unroll_variant).
"""
import copy

import numpy as np
import pytest

import oracle as O
import unroll_harness as H
from helpers import ORACLE_CFGS, device_problem, make_params, make_problem, random_state
from unroll_harness import eng  # noqa: F401  (the fixture)

B, STEP0 = 2, 1
GOLDEN = H.Golden("pair_l2a_bytes.json")
L2_GAIN = 8.0                 # the "mixed signs" cell: lstm_2's weights times this


def _cells():
    """id -> dict(net, kind, D, T, seed, record, gain, scale, variant)   (the seeds are part of the golden file)"""
    cells, seed = {}, 900

    def add(name, net, kind, D, T=3, record=False, gain=1.0, scale=0.5, fast=1):
        nonlocal seed
        seed += 1
        cells[name] = dict(net=net, kind=kind, D=D, T=T, seed=seed, record=record, gain=gain, scale=scale,
                           variant=dict(CH=(D + 15) // 16 if D % 16 == 0 else 8, HIST=int(record), EXACT=0, FAST=fast, KR=0, NV=0))

    for net in ("dm", "dm_logsign"):
        for kind in ("quadratic", "rastrigin"):
            for D in (32, 64, 128):
                add("%s_%s_d%d" % (net, kind, D), net, kind, D)
    add("dm_quadratic_d128_mixed_signs", "dm", "quadratic", 128, gain=L2_GAIN, scale=1.0)
    add("dm_quadratic_d128_T1", "dm", "quadratic", 128, T=1)
    add("dm_rastrigin_d64_T2", "dm", "rastrigin", 64, T=2)
    add("dm_rastrigin_d100_ragged", "dm", "rastrigin", 100, fast=0)
    add("dm_quadratic_d128_record", "dm", "quadratic", 128, record=True)
    return cells


CELLS = _cells()
# the cells whose kernel keeps the parent's placement of chunk L2A by the trait (csrc/l2o_lstm_bx3.h, kPairL2bLate): the
# gather, the recording kernel and LogAndSign at CH = 8
KEEPS_PARENT_TEXT = ("dm_rastrigin_d100_ragged", "dm_quadratic_d128_record", "dm_logsign_quadratic_d128", "dm_logsign_rastrigin_d128")


def cell_params(name):
    c = CELLS[name]
    p = make_params(ORACLE_CFGS[c["net"]], seed=5, trained_like=True)
    if c["gain"] != 1.0:
        p = copy.deepcopy(p)
        p["lstm_2"]["w_gates"] = (p["lstm_2"]["w_gates"] * np.float32(c["gain"])).astype(np.float32)
    return p


def initial_state(name):
    c = CELLS[name]
    return random_state(ORACLE_CFGS[c["net"]], B * c["D"], c["seed"] + 60000, scale=c["scale"])


def prepare_cell(eng, name):
    c = CELLS[name]
    cfg = ORACLE_CFGS[c["net"]]
    _, x0, arrays = make_problem(c["kind"], B, c["D"], seed=c["seed"])
    return H.prepare(eng, cfg, cell_params(name), device_problem(eng, arrays, B, c["D"]), c["T"], x=x0,
                     state=initial_state(name), step0=STEP0, record=c["record"])


def run_cell(eng, name):
    """One launch of the cell -> {quantity: sha256 of the raw bytes}; it ran the kernel the cell names."""
    c = CELLS[name]
    r = prepare_cell(eng, name).run()
    assert (r.form, r.dispatches) == ("k_unroll_pair", 1), (name, r.form, r.dispatches)
    assert r.variant == c["variant"], (name, r.variant)
    keys = ("fx", "x", "st") + (("hist_st", "hist_g", "hist_g_final") if c["record"] else ())
    for k in keys:
        assert not np.isnan(r.host[k]).any(), "%s: NaN in %s" % (name, k)
    assert r.host["fx"].shape == (c["T"] + 1,)
    return {k: H.sha(r.host[k]) for k in keys}


def golden_launches(eng):
    return {name: prepare_cell(eng, name) for name in CELLS}


def golden_cells(eng):
    return {name: run_cell(eng, name) for name in sorted(CELLS)}


def layer2_preactivations(name):
    """The oracle's layer-2 gate pre-activations (i, j, f + forget_bias, o), [B * D, 20] each, at every step of the cell."""
    c = CELLS[name]
    cfg, params = ORACLE_CFGS[c["net"]], cell_params(name)
    prob, x, _ = make_problem(c["kind"], B, c["D"], seed=c["seed"])
    state, out = initial_state(name), []
    for _ in range(c["T"]):
        g = prob.grad(x)
        delta, nxt = O.net_apply(cfg, params, g, state)
        h1 = nxt[0][0]                                             # h1(t): the input of layer 2
        z = np.concatenate([h1, state[1][0]], axis=1) @ params["lstm_2"]["w_gates"] + params["lstm_2"]["b_gates"]
        i, j, f, o = np.split(z, 4, axis=1)
        out.append((i, j, f + np.float32(1.0), o))
        x, state = x + delta, nxt
    return out


def test_golden_covers_every_cell():
    GOLDEN.check_covers(CELLS)


def test_cells_that_keep_the_parent_text():
    """The trait's exceptions are among the cells: not FAST, recording, or LogAndSign at CH = 8 -- and only those."""
    for name, c in CELLS.items():
        v = c["variant"]
        keeps = not v["FAST"] or v["HIST"] or (c["net"] == "dm_logsign" and v["CH"] == 8)
        assert keeps == (name in KEEPS_PARENT_TEXT), name
    assert {CELLS[n]["variant"]["CH"] for n in CELLS if n not in KEEPS_PARENT_TEXT} == {2, 4, 8}


@pytest.mark.parametrize("name", sorted(CELLS))
def test_initial_state_is_nonzero(name):
    """Step 0 multiplies a non-zero h2 in chunk L2B and gates a non-zero c2: every unit of every coordinate."""
    (h1, c1), (h2, c2) = initial_state(name)
    for a in (h1, c1, h2, c2):
        assert a.shape == (B * CELLS[name]["D"], 20) and np.all(a != 0.0)


def test_mixed_signs_cell_has_both_signs_in_every_gate_at_every_step():
    steps = layer2_preactivations("dm_quadratic_d128_mixed_signs")
    assert len(steps) == 3
    for t, gates in enumerate(steps):
        for gate, z in zip("ijfo", gates):
            frac = float((z < 0).mean())
            print("step %d gate %s: %.3f negative, min %.3g max %.3g" % (t, gate, frac, z.min(), z.max()))
            # not a token sign: at least a tenth of the pre-activations on either side
            assert 0.1 < frac < 0.9, (t, gate, frac)


def test_cells_are_not_degenerate():
    c = GOLDEN.cells
    assert len({c[name]["st"] for name in CELLS}) == len(CELLS)
    assert len({c[name]["fx"] for name in CELLS}) == len(CELLS)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CELLS))
def test_bytes_equal_the_parent_commit(eng, name):
    GOLDEN.check(name, run_cell(eng, name))
