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
   commit's library on an MI355X (tests/golden/pair_bias_bytes.json, scripts/record_pair_bias_bytes.py).
"""
import hashlib
import json
import os

import numpy as np
import pytest

import mfma_emulator as E
import test_unroll_instantiations as ui
from helpers import ORACLE_CFGS, device_problem, lib_option, make_params, make_problem, random_state, spec_of
from open_l2o_amd import _abi

pytestmark = pytest.mark.gpu

T = 3
T_LONG = 64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pair_bias_bytes.json")
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


@pytest.fixture(scope="module")
def eng():
    from open_l2o_amd._engine import HipEngine
    return HipEngine()


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


def _problem(eng, kind, B, D, seed):
    _, x0, arrays = make_problem(kind, B, D, seed=seed, M=D if kind == "lasso" else None)
    return x0.reshape(B, D), device_problem(eng, arrays, B, D)


def _outputs(out):
    return {k: t.detach().cpu().numpy().copy() for k, t in out.items()}


def run_cell(eng, cell, mode, fast, steps=T, record=False):
    """One launch of `steps` steps -> {fx, x, st (, m, v): host arrays}.  fast: 1 the FAST kernel, 0 full tiles on the gather;
    record: the recording kernel (HIST) of the same prologue."""
    import torch
    net, kind, B, D, seed = cell
    cfg = ORACLE_CFGS[net]
    spec = spec_of(cfg)
    wpack = eng.pack_weights(spec, make_params(cfg, seed=5, trained_like=True))
    x0, pd = _problem(eng, kind, B, D, seed)
    rn = cfg.kind == "rnnprop"
    fx_part, fx = eng.zeros((steps + 1) * B), eng.zeros(steps + 1)
    hist = None
    if record:
        N = B * D
        hist = {"st": eng.zeros(steps, eng.state_floats(B, D)), "g": eng.zeros(steps, N), "g_final": eng.zeros(N)}
        if rn:
            hist.update(m=eng.zeros(steps, N), v=eng.zeros(steps, N))
    with lib_option(_abi.OPT_PAIR_FAST_LOAD, fast):
        if mode == "zero_state":
            x, st = eng.zeros(B, D), eng.state_alloc(B, D)
            m, v = (eng.zeros(B, D), eng.zeros(B, D)) if rn else (None, None)
            eng.unroll(spec, wpack, pd, x, st, m, v, steps, 1, fx_part, fx=fx, x0=eng.tensor(x0), zero_state=True, hist=hist)
        else:
            rng = np.random.default_rng(seed + 7000)
            x = eng.tensor(x0)
            st = eng.state_pack(*[eng.tensor(a) for hc in random_state(cfg, B * D, seed + 6000, scale=0.5) for a in hc], B, D)
            m = v = None
            if rn:
                m = eng.tensor((rng.standard_normal((B, D)) * 0.3).astype(np.float32))
                v = eng.tensor(rng.uniform(0.1, 1.0, (B, D)).astype(np.float32))
            eng.unroll(spec, wpack, pd, x, st, m, v, steps, 1 + T, fx_part, fx=fx, hist=hist)
        assert eng.last_unroll_form() == ("k_unroll_pair", 1)
        assert eng.last_unroll_variant() == dict(CH=D // 16, HIST=int(record), EXACT=0, FAST=fast, KR=0, NV=0)
    torch.cuda.synchronize()
    eng.check_unroll_status()
    out = {"fx": fx, "x": x, "st": st}
    if rn:
        out.update(m=m, v=v)
    return _outputs(out)


def run_chain(eng, launches):
    """CHAIN_CELL from x0 and the zero state: T = 2 as one launch (launches = 1) or as two chained launches of T = 1
    -> {fx[0..2], x, st}."""
    import torch
    net, kind, B, D, seed = CHAIN_CELL
    cfg = ORACLE_CFGS[net]
    spec = spec_of(cfg)
    wpack = eng.pack_weights(spec, make_params(cfg, seed=5, trained_like=True))
    x0, pd = _problem(eng, kind, B, D, seed)
    x, st = eng.zeros(B, D), eng.state_alloc(B, D)
    if launches == 1:
        fx_part, fx = eng.zeros(3 * B), eng.zeros(3)
        eng.unroll(spec, wpack, pd, x, st, None, None, 2, 1, fx_part, fx=fx, x0=eng.tensor(x0), zero_state=True)
        assert eng.last_unroll_variant() == dict(CH=D // 16, HIST=0, EXACT=0, FAST=1, KR=0, NV=0)
        torch.cuda.synchronize()
        fx_all = fx.cpu().numpy().copy()
    else:
        fa_part, fa, fb_part, fb = eng.zeros(2 * B), eng.zeros(2), eng.zeros(2 * B), eng.zeros(2)
        eng.unroll(spec, wpack, pd, x, st, None, None, 1, 1, fa_part, fx=fa, x0=eng.tensor(x0), zero_state=True)
        assert eng.last_unroll_variant() == dict(CH=D // 16, HIST=0, EXACT=0, FAST=1, KR=0, NV=0)
        eng.unroll(spec, wpack, pd, x, st, None, None, 1, 2, fb_part, fx=fb)
        assert eng.last_unroll_variant() == dict(CH=D // 16, HIST=0, EXACT=0, FAST=1, KR=0, NV=0)
        torch.cuda.synchronize()
        fa, fb = fa.cpu().numpy(), fb.cpu().numpy()
        # f(x_1) is the last loss of the first launch and the first of the second: the same bytes
        assert fa[1:].tobytes() == fb[:1].tobytes()
        fx_all = np.concatenate([fa, fb[1:]])
    eng.check_unroll_status()
    out = _outputs({"x": x, "st": st})
    out["fx"] = fx_all
    return out


def run_long(eng, monkeypatch):
    """LONG_CELL through the harness of test_unroll_instantiations at T = 64 -> (outputs, form, variant, float64
    trajectory, float32 envelope, one-ulp spread)."""
    monkeypatch.setattr(ui, "T", T_LONG)
    inp = ui.inputs(ui.recipe_of(LONG_CELL))
    f64, f32 = ui.trajectory(inp, np.float64), ui.trajectory(inp, np.float32)
    out, form, variant, _ = ui.launch(eng, LONG_CELL)
    return out, form, variant, f64, ui.measure(f32, f64), ui.ulp_spread(inp)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def golden_cells(eng, monkeypatch):
    """Every cell of this file on the FAST kernel -> {id: {quantity: sha256 of the raw bytes}} (what the golden file holds)."""
    cells = {}
    for name in sorted(CELLS):
        for mode in MODES:
            cells["%s/%s" % (name, mode)] = {k: sha(a) for k, a in run_cell(eng, CELLS[name], mode, 1).items()}
    cells["chain_t2/one_launch"] = {k: sha(a) for k, a in run_chain(eng, 1).items()}
    out = run_long(eng, monkeypatch)[0]
    cells["long_t64"] = {"fx": sha(out["fx"]), "x": sha(out["x"]), "st": sha(np.stack(out["st"]))}
    return cells


@pytest.mark.parametrize("net", NETS)
def test_bias_quads_are_pairwise_different_and_nonzero(net):
    assert_biases_tell_quads_apart(net)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["cells"]


def _check_golden(golden, key, out):
    want = golden[key]
    got = {k: sha(a) for k, a in out.items()}
    assert sorted(got) == sorted(want), key
    for k in sorted(got):
        assert got[k] == want[k], "%s: %s differs from the parent commit's bytes" % (key, k)


@pytest.mark.parametrize("name", sorted(CELLS))
def test_registers_equal_the_lds_reads_and_the_parent(eng, golden, name):
    assert_biases_tell_quads_apart(CELLS[name][0])
    res = {}
    for mode in MODES:
        fast = res[mode] = run_cell(eng, CELLS[name], mode, 1)
        rec = run_cell(eng, CELLS[name], mode, 1, record=True)
        slow = run_cell(eng, CELLS[name], mode, 0)
        assert fast.keys() == slow.keys()
        for k in fast:
            assert not np.isnan(fast[k]).any(), "%s, %s: NaN in %s" % (name, mode, k)
            assert fast[k].tobytes() == slow[k].tobytes(), "%s, %s: %s differs from the gather kernel's" % (name, mode, k)
        for k in ("fx", "x"):
            assert fast[k].tobytes() == rec[k].tobytes(), "%s, %s: %s differs from the recording kernel's" % (name, mode, k)
        _check_golden(golden, "%s/%s" % (name, mode), fast)
    # the two modes are different computations (a launch that ignored its state would make them equal)
    assert (res["zero_state"]["st"] != res["continuing"]["st"]).any()


def test_first_step_equals_later_steps(eng, golden):
    one, two = run_chain(eng, 1), run_chain(eng, 2)
    assert one.keys() == two.keys()
    for k in one:
        assert not np.isnan(one[k]).any(), k
        assert one[k].tobytes() == two[k].tobytes(), "%s: one launch of T = 2 differs from two launches of T = 1" % k
    _check_golden(golden, "chain_t2/one_launch", one)


def test_long_unroll_vs_float64(eng, golden, monkeypatch):
    out, form, variant, f64, env, ulp = run_long(eng, monkeypatch)
    assert form == LONG_CELL.template and variant == LONG_CELL.variant, (form, variant)
    err = ui.measure(out, f64)
    print("T = %d: %s" % (T_LONG, " ".join("%s %.2g/%.2g (bound %.2g)" % (k, err[k], env[k], ui.bound_of(k, env)) for k in sorted(err))))
    bad = ui.oracle_conditions(env, ulp) + ui.violations(err, env)
    assert not bad, "\n".join(bad)
    _check_golden(golden, "long_t64", {"fx": out["fx"], "x": out["x"], "st": np.stack(out["st"])})


def test_golden_covers_every_cell(golden):
    want = ["%s/%s" % (n, m) for n in CELLS for m in MODES] + ["chain_t2/one_launch", "long_t64"]
    assert sorted(golden) == sorted(want)
