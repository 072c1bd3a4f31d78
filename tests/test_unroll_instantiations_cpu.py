"""The CPU half of tests/test_unroll_instantiations.py: the cell table is what the dispatch rules give, and the fixed
bounds of that module rest on the reference alone -- the float32 oracle stays within a third of every bound, and its
state envelope below 3.3e-5, and from 8 starts one ulp away it stays within half of every bound, in EVERY cell -- before
anything runs on an MI355X."""
import collections

import numpy as np

import oracle as O
import test_unroll_instantiations as U
from open_l2o_amd import _abi

ALL_CELLS = U.CELLS + U.PINS_IGNORED + U.PINS_ROUTED


def test_cell_counts_are_what_the_dispatch_rules_give():
    primary = [c for c in U.CELLS if c.second is None]
    count = collections.Counter(c.template for c in primary)
    nets, kinds = len(U.NETS), len(U.KINDS)
    # k_unroll: CH 1, 2, 4 plain / exact / recording, CH 8 plain / recording (no <8, false, true> instantiation)
    assert count["k_unroll"] == nets * kinds * (3 * 3 + 2) == 132
    # k_unroll_pair: CH 2, 4, 8 (a one-tile problem is not split) x plain / exact / recording x gather / FAST
    assert count["k_unroll_pair"] == nets * kinds * 3 * 3 * 2 == 216
    assert count["k_unroll_lds"] == nets * kinds * 2 == 24
    assert count["k_unroll_cu"] == nets * 2 * 2 == 12
    # k_unroll_cu8: every (NV, KR, HIST) for which some D of that NV fits() -- all of them, NV 2 / KR 2 only up to D = 384
    reach = sum(1 for net in U.NETS for NV, Ds in ((1, range(132, 257, 4)), (2, range(260, 513, 4))) for KR in (4, 3, 2)
                for hist in (0, 1) if any(U.cu8_fits(D, net, KR) for D in Ds))
    assert count["k_unroll_cu8"] == reach == 36
    assert sum(count.values()) == 420
    for net in U.NETS:
        assert not U.cu8_fits(512, net, 2) and U.cu8_fits(384, net, 2) and not U.cu8_fits(388, net, 2)
        assert U.cu8_fits(512, net, 3) and U.cu8_fits(512, net, 4)


def test_no_two_primary_cells_select_the_same_instantiation():
    seen = {}
    for c in U.CELLS:
        key = U.instantiation(c)
        if c.second is None:
            assert key not in seen, (U.cell_id(c), U.cell_id(seen[key]))
            seen[key] = c
    for c in ALL_CELLS:                                           # a second shape repeats a primary instantiation
        if c.second is not None:
            assert U.instantiation(c) in seen, U.cell_id(c)
    ids = [(U.cell_id(c), tuple(sorted(c.options.items()))) for c in U.CELLS]
    assert len(set(ids)) == len(ids)


def test_cells_match_the_geometry_they_claim():
    P, L, F, X, UC = _abi.OPT_PAIR, _abi.OPT_ONE_LDS, _abi.OPT_PAIR_FAST_LOAD, _abi.OPT_EXACT_GATES, _abi.OPT_UNROLL_CU
    scaled = collections.Counter()
    for c in ALL_CELLS:
        inp = U.inputs(U.recipe_of(c))
        M, D, v, o = inp.arrays["M"], c.D, c.variant, c.options
        ch = U.geom_ch(D, M)
        if c.template in ("k_unroll_cu", "k_unroll_cu8"):
            assert ch is None and D % 4 == 0 and v["NV"] == (1 if D <= 256 else 2) and v["CH"] == v["EXACT"] == v["FAST"] == 0
            form = o[UC]
            if form == 1:
                assert (c.template, v["KR"]) == U.default_streaming_route(D, c.net, v["HIST"])
            elif c.template == "k_unroll_cu8":
                assert v["KR"] == 7 - form and U.cu8_fits(D, c.net, v["KR"])
            else:
                assert form == 2 and v["KR"] == 0
        else:
            assert ch == (v["CH"] or 8) and v["KR"] == v["NV"] == 0
            exact_asked = o.get(X, 0) == 1 and not v["HIST"]
            full = M == D == 16 * ch
            if c.template == "k_unroll":
                assert o[P] == 0 and (ch < 8 or o.get(L) == 0 or exact_asked)       # else k_unroll_lds takes 5..8 tiles
                assert v["EXACT"] == int(exact_asked and ch <= 4) and v["FAST"] == 0
            elif c.template == "k_unroll_pair":
                assert ch >= 2 and o.get(P, 1) == 1 and (o.get(L, 1) != 2 or exact_asked)
                assert v["EXACT"] == int(exact_asked) and v["FAST"] == int(full and o.get(F, 1) == 1)
            else:
                assert c.template == "k_unroll_lds" and ch == 8 and D > 64 and o[L] == 2 and not exact_asked
                assert v["CH"] == v["EXACT"] == v["FAST"] == 0
        scaled[(c.template, inp.xs is None)] += 1
        if c.kind == "lasso" and ch is not None:                   # (the resident forms: ragged rows, or M = D at full tiles)
            assert (M == D) == (D in U.FULL.values()) and (M == D or M % 4)
    for tpl in U.TEMPLATES:                                        # every template runs with and without x_scale
        assert scaled[(tpl, True)] > 0 and scaled[(tpl, False)] > 0, tpl
    lasso = {(U.inputs(U.recipe_of(c)).arrays["M"], c.D) for c in U.CELLS if c.kind == "lasso"}
    assert (7, 10) in lasso and (300, 256) in lasso and (45, 20) in lasso


def test_float32_oracle_keeps_the_bounds_honest_in_every_cell():
    recipes = sorted({U.recipe_of(c) for c in ALL_CELLS})
    worst = collections.defaultdict(float)
    bad, above = [], 0
    for r in recipes:
        ref = U.reference(r)
        bad += ["%s/%s D=%d: %s" % (r + (b,)) for b in U.oracle_conditions(ref.env, ref.ulp)]
        for k, e in ref.env.items():
            worst[k] = max(worst[k], e)
        above += ref.env["st"] > 3.3e-6
        assert np.all(np.isfinite(ref.f64["fx"])) and np.all(np.isfinite(ref.f64["x"]))
        assert (ref.f64["fx"][0] != ref.f64["fx"][-1])                # the optimizer moved the iterate
    print("%d recipes; float32 oracle worst: %s; state envelope above 3.3e-6 in %d"
          % (len(recipes), " ".join("%s %.3g" % kv for kv in sorted(worst.items())), above))
    assert not bad, "\n".join(bad)
    assert len(recipes) >= 140


def test_trajectory_is_the_oracle_unroll():
    """The reference loop with its per-step values kept computes what O.unroll computes, bit for bit, in both precisions."""
    for recipe in (("dm", "quadratic", 16), ("dm_logsign", "lasso", 10), ("rnnprop", "rastrigin", 24),
                   ("rnnprop", "square_cos", 40), ("dm", "lasso", 20)):
        inp = U.inputs(recipe)
        for dt in (np.float32, np.float64):
            got = U.trajectory(inp, dt)
            prob = U.as_float64(inp.prob) if dt == np.float64 else inp.prob
            params = {k: {n: a.astype(dt) for n, a in d.items()} for k, d in inp.params.items()}
            state = tuple((h.astype(dt), c.astype(dt)) for h, c in inp.state0)
            rn = inp.cfg.kind == "rnnprop"
            res = O.unroll(prob, inp.cfg, params, inp.x0.astype(dt), state, U.T,
                           x_scale=None if inp.xs is None else inp.xs.astype(dt),
                           m0=inp.m0.astype(dt) if rn else None, v0=inp.v0.astype(dt) if rn else None, step0=U.STEP0)
            assert got["fx"].dtype == dt and got["fx"].tobytes() == res.fx.tobytes()
            assert got["x"].tobytes() == res.x.tobytes()
            for a, b in zip(got["st"], [a for hc in res.state for a in hc]):
                assert a.tobytes() == b.tobytes()
            if rn:
                assert got["m"].tobytes() == res.m.tobytes() and got["v"].tobytes() == res.v.tobytes()
