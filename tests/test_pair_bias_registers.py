"""The plain kernels of the two-CU unroll (csrc/l2o_unroll_pair.h, the bf16x3 core) keep the lane's ten gate-bias quads
in registers for the whole launch (LstmCoreRegs::hold_bias / arm, csrc/l2o_lstm_bx3.h, kPairBiasRegs): the accumulators
of every step start from them, the first MFMA of each accumulation chain reading the quad as its C operand, and the step no
longer re-reads the 160-float table from LDS.  The recording kernels (and two gather instantiations that would spill)
keep the LDS reads.  None of it changes a bit of any result.

Checked here through the C ABI:
 * the weights (make_params(..., trained_like=True)) give a packed bias table whose ten quads per lane group are pairwise
   different and non-zero in every word -- with equal or zero biases a swapped layer or M-tile would pass everything below;
 * FAST (registers) == the RECORDING kernel of the same library (LDS reads) on fx and x_T, and == the gather kernel
   (L2O_OPT_PAIR_FAST_LOAD = 0: the other prologue; registers too in these cells) on fx, x_T, the state and m / v, byte for
   byte, T = 3: quadratic at D = 32, 64, 128 (CH 2, 4, 8) x the nets dm, dm_logsign, rnnprop x B = 1, 3, 9 (one lane, a
   partial group, two launch groups), one rastrigin and one lasso cell at D = 64 -- each from the zero state (x0,
   zero_state) and continuing from a random state (random moments for RNNProp, step0 = 4);
 * first step versus later steps: one launch of T = 2 == two chained launches of T = 1, byte for byte, on fx[0..2], x_T
   and the final state -- the first step of a launch is armed in front of the loop, every later one inside it;
 * long enough for a clobbered register to show: D = 128, dm, B = 3, T = 64 against the float64 reference, with the harness
   and the bounds of tests/test_unroll_instantiations.py (its float32-oracle conditions hold at T = 64 and are asserted);
 * the parent's bytes: fx, x_T, the final state (and m, v) of every cell above equal the SHA-256 recorded with the PARENT
   commit's library on an MI355X (tests/golden/pair_bias_bytes.json, scripts/record_pair_bytes.py).
"""
import numpy as np
import pytest

import mfma_emulator as E
import test_unroll_instantiations as ui
import unroll_harness as H
from helpers import ORACLE_CFGS, device_problem, make_params, make_problem, random_state, spec_of
from open_l2o_amd import _abi
from unroll_harness import eng  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

T = 3
T_LONG = 64
GOLDEN = H.Golden("pair_bias_bytes.json")
NETS = ("dm", "dm_logsign", "rnnprop")


def _cells():
    """id -> (net, kind, B, D, problem seed)   (the seeds are part of the golden file)"""
    cells, seed = {}, 500
    for D in (32, 64, 128):
        for net in NETS:
            for B in (1, 3, 9):
                seed += 1
                cells["%s_quadratic_d%d_b%d" % (net, D, B)] = (net, "quadratic", B, D, seed)
    cells["dm_rastrigin_d64_b3"] = ("dm", "rastrigin", 3, 64, 541)
    cells["dm_lasso_d64_b3"] = ("dm", "lasso", 3, 64, 542)
    return cells


CELLS = _cells()
MODES = ("zero_state", "continuing")
CHAIN_CELL = ("dm", "quadratic", 3, 128, 551)          # T = 2 in one launch and in two
LONG_CELL = ui._cell("k_unroll_pair", "dm", "quadratic", 128, {}, CH=8, FAST=1, HIST=0, EXACT=0)


def bias_table(net):
    """The packed gate-bias table of the test weights: [layer][M-tile][lane group][gate] (l2o::bx::bias_off)."""
    from open_l2o_amd._engine import pack_weights_host
    cfg = ORACLE_CFGS[net]
    spec = spec_of(cfg)
    wp = pack_weights_host(_abi.lib(), spec, make_params(cfg, seed=5, trained_like=True))
    pre = spec.preprocess
    off = E.wp_rows(pre)["total"] * 64 + E.bx_packed_words(pre) + E.bx_level_words(pre) + E.bx_win_words(pre)
    return np.asarray(wp[off:off + E.BX_BIAS_WORDS], np.float32).reshape(2, E.KNT, 4, 4)


def assert_biases_tell_quads_apart(net):
    tab = bias_table(net)
    assert np.all(tab != 0.0), "%s: a zero word in the packed bias table" % net
    for q in range(4):
        quads = [tab[layer, t, q].tobytes() for layer in range(2) for t in range(E.KNT)]
        assert len(quads) == 10 and len(set(quads)) == 10, "%s: lane group %d has equal bias quads" % (net, q)


def prepare_cell(eng, cell, mode, fast, record=False, steps=T):
    """`steps` steps from the zero state (x0, zero_state) or continuing from a random state.  fast: 1 the FAST kernel, 0
    full tiles on the gather; record: the recording kernel (HIST) of the same prologue."""
    net, kind, B, D, seed = cell
    cfg = ORACLE_CFGS[net]
    _, x0, arrays = make_problem(kind, B, D, seed=seed, M=D if kind == "lasso" else None)
    common = dict(options={_abi.OPT_PAIR_FAST_LOAD: fast}, record=record)
    args = (eng, cfg, make_params(cfg, seed=5, trained_like=True), device_problem(eng, arrays, B, D), steps)
    if mode == "zero_state":
        return H.prepare(*args, x0=x0, **common)
    rng = np.random.default_rng(seed + 7000)
    m = v = None
    if cfg.kind == "rnnprop":
        m = (rng.standard_normal((B, D)) * 0.3).astype(np.float32)
        v = rng.uniform(0.1, 1.0, (B, D)).astype(np.float32)
    return H.prepare(*args, x=x0, state=random_state(cfg, B * D, seed + 6000, scale=0.5), m=m, v=v, step0=1 + T,
                     fused_fx=True, **common)


def _expect(r, D, fast=1, record=False):
    assert (r.form, r.dispatches) == ("k_unroll_pair", 1)
    assert r.variant == dict(CH=D // 16, HIST=int(record), EXACT=0, FAST=fast, KR=0, NV=0)
    return r


def run_cell(eng, cell, mode, fast, record=False):
    """One launch of T steps -> {fx, x, st (, m, v): host arrays}."""
    r = _expect(prepare_cell(eng, cell, mode, fast, record).run(), cell[3], fast, record)
    return {k: r.host[k] for k in ("fx", "x", "st", "m", "v") if k in r.host}


def run_chain(eng, launches):
    """CHAIN_CELL from x0 and the zero state: T = 2 as one launch (launches = 1) or as two chained launches of T = 1
    -> {fx[0..2], x, st}."""
    D = CHAIN_CELL[3]
    first = prepare_cell(eng, CHAIN_CELL, "zero_state", 1, steps=2 // launches)
    r = _expect(first.run(), D)
    fx = r.host["fx"]
    if launches == 2:
        r = _expect(first.then(step0=2).run(), D)
        # f(x_1) is the last loss of the first launch and the first of the second: the same bytes
        assert fx[1:].tobytes() == r.host["fx"][:1].tobytes()
        fx = np.concatenate([fx, r.host["fx"][1:]])
    return {"x": r.host["x"], "st": r.host["st"], "fx": fx}


def run_long(eng):
    """LONG_CELL through the launch of test_unroll_instantiations at T = 64 -> (outputs, float64 trajectory, float32
    envelope, one-ulp spread)."""
    inp = ui.inputs(ui.recipe_of(LONG_CELL))
    f64, f32 = ui.trajectory(inp, np.float64, T_LONG), ui.trajectory(inp, np.float32, T_LONG)
    out, form, variant, _ = ui.launch(eng, LONG_CELL, T=T_LONG)
    assert form == LONG_CELL.template and variant == LONG_CELL.variant, (form, variant)
    return out, f64, ui.measure(f32, f64), ui.ulp_spread(inp, T_LONG)


def _long_bytes(out):
    return {"fx": out["fx"], "x": out["x"], "st": np.stack(out["st"])}


def golden_launches(eng):
    """Every launch behind the golden file, prepared and not run."""
    cells = {"%s/%s" % (name, mode): prepare_cell(eng, CELLS[name], mode, 1) for name in CELLS for mode in MODES}
    cells["chain_t2/one_launch"] = prepare_cell(eng, CHAIN_CELL, "zero_state", 1, steps=2)
    cells["long_t64"] = ui.prepare(eng, LONG_CELL, T=T_LONG)
    return cells


def golden_cells(eng):
    """Every cell of this file on the FAST kernel -> {id: {quantity: sha256 of the raw bytes}} (what the golden file holds)."""
    for net in NETS:
        assert_biases_tell_quads_apart(net)
    cells = {"%s/%s" % (name, mode): run_cell(eng, CELLS[name], mode, 1) for name in sorted(CELLS) for mode in MODES}
    cells["chain_t2/one_launch"] = run_chain(eng, 1)
    cells["long_t64"] = _long_bytes(run_long(eng)[0])
    return {name: {k: H.sha(a) for k, a in out.items()} for name, out in cells.items()}


@pytest.mark.parametrize("net", NETS)
def test_bias_quads_are_pairwise_different_and_nonzero(net):
    assert_biases_tell_quads_apart(net)


@pytest.mark.parametrize("name", sorted(CELLS))
def test_registers_equal_the_lds_reads_and_the_parent(eng, name):
    assert_biases_tell_quads_apart(CELLS[name][0])
    res = {}
    for mode in MODES:
        fast = res[mode] = run_cell(eng, CELLS[name], mode, 1)
        rec = run_cell(eng, CELLS[name], mode, 1, record=True)
        slow = run_cell(eng, CELLS[name], mode, 0)
        for k in fast:
            assert not np.isnan(fast[k]).any(), "%s, %s: NaN in %s" % (name, mode, k)
        H.assert_same_bytes(fast, slow, "%s, %s, against the gather kernel" % (name, mode))
        H.assert_same_bytes({k: fast[k] for k in ("fx", "x")}, {k: rec[k] for k in ("fx", "x")},
                            "%s, %s, against the recording kernel" % (name, mode))
        GOLDEN.check("%s/%s" % (name, mode), fast)
    # the two modes are different computations (a launch that ignored its state would make them equal)
    assert (res["zero_state"]["st"] != res["continuing"]["st"]).any()


def test_first_step_equals_later_steps(eng):
    one, two = run_chain(eng, 1), run_chain(eng, 2)
    for k in one:
        assert not np.isnan(one[k]).any(), k
    H.assert_same_bytes(one, two, "one launch of T = 2 against two launches of T = 1")
    GOLDEN.check("chain_t2/one_launch", one)


def test_long_unroll_vs_float64(eng):
    out, f64, env, ulp = run_long(eng)
    err = ui.measure(out, f64)
    print("T = %d: %s" % (T_LONG, " ".join("%s %.2g/%.2g (bound %.2g)" % (k, err[k], env[k], ui.bound_of(k, env)) for k in sorted(err))))
    bad = ui.oracle_conditions(env, ulp) + ui.violations(err, env)
    assert not bad, "\n".join(bad)
    GOLDEN.check("long_t64", _long_bytes(out))


def test_golden_covers_every_cell():
    GOLDEN.check_covers(["%s/%s" % (n, m) for n in CELLS for m in MODES] + ["chain_t2/one_launch", "long_t64"])
