"""l2o_twin_unroll (csrc/l2o_twin.h) on the MI355X, through the C ABI and through twin.unroll, against the float64 torch
restatement of twin_reference.py.

Criterion.  Every output array (curve, f, delta, theta, the two final states) is compared relative to its largest float64
entry.  The bound is 4 x the float32 torch restatement's own worst such error against float64 on the same inputs (the kernel
sums in another order), computed here on the CPU per group of cases -- the criterion and margin of test_kernel_lstm.py.
Networks are at torch's default initialisation scale, optim_it = 40 (7 sign iterations), a, b in [0.5, 3], A in [0.5, 1]
under a 0.5 mask, starts and states drawn as in the reference.

Measured on one MI355X (float32 torch worst -> bound; kernel worst; the tests print every figure before they assert):
delta phase (11 cases) 1.34e-06 -> 5.37e-06; 2.47e-06.  rescale = 1: 2.65e-06 -> 1.06e-05; 2.65e-06, and zeroing a weight
block of either network moves the float64 curve by 3.3e-02 ... 8.7e-01.  Widths: 1.04e-06 -> 4.17e-06; 6.2e-07.  Sign phase:
4.53e-07 -> 1.81e-06; 7.1e-07, min |delta| over the sign iterations 2.5e-02 (seesaw) and 2.7e-02 (matrix game).  out_mul = 0.5:
2.30e-06 -> 9.19e-06; 5.2e-07.  The driver's mean distances: 2.8e-09 and 1.2e-09 from the float32 restatement's (allowed
1.3e-05).  (The float32 restatement runs on the CPU of the machine at hand, so its worst error moves in the last digits.)"""
import functools
import json
import os

import numpy as np
import pytest
import torch

import twin_reference as TR
from open_l2o_amd import _abi, _engine, twin
from test_twin_cpu import GOLDEN, load_driver, make_data

pytestmark = pytest.mark.gpu

OPTIM_IT = 40
ARRAYS = ("curve", "f", "delta", "theta", "state_min", "state_max")
BLOCKS = ("recurs.weight_ih", "recurs.weight_hh", "recurs2.weight_ih", "recurs2.weight_hh", "recurs2.bias_ih", "output.weight")


@pytest.fixture
def eng():
    e, old = _engine.HipEngine(), _engine._default_engine
    _engine.set_default_engine(e)
    try:
        yield e
    finally:
        _engine.set_default_engine(old)


def spec(kind, n_inst, dim=1, H=(50, 50), n_in=2, iter0=9, n_iter=56, rescale=1e-4, out_mul=1.0, seed=0):
    return (kind, n_inst, dim, H, n_in, iter0, n_iter, rescale, out_mul, seed)


# 1. the delta phase: rows at, below and above one and two tiles; matrix games whose instances would straddle 16-row tiles
DELTA = [spec(3, n) for n in (1, 15, 16, 17, 33)] + [spec(4, n, d) for n, d in ((7, 5), (11, 3), (2, 16), (1, 1))] + \
        [spec(1, 17), spec(2, 17)]
# 2. rescale = 1: the recurrent weights count
RECUR = [spec(3, 17, rescale=1.0), spec(4, 7, 5, rescale=1.0)]
# 3. widths: padded (5, 50), two k-step groups of four (80), the largest (96), two different nets, one input column
WIDTHS = [spec(4, 7, 5, H=(5, 5)), spec(4, 7, 5, H=(80, 80)), spec(4, 7, 5, H=(96, 96)), spec(4, 7, 5, H=(50, 80)),
          spec(4, 7, 5, n_in=1)]
# 4. the sign phase
SIGN = [spec(3, 7, iter0=1, n_iter=40), spec(4, 7, 5, iter0=1, n_iter=40)]
# 6. out_mul
OUTMUL = [spec(3, 17, out_mul=0.5)]


@functools.lru_cache(maxsize=None)
def make_case(kind, n_inst, dim, H, n_in, seed):
    prob = twin.problem(kind, make_data(kind, n_inst, dim, 100 + seed), dim)
    mn = twin.Optimizer(H[0], use_second=n_in == 2, seed=1000 + seed)
    mx = twin.Optimizer(H[1], use_second=n_in == 2, seed=2000 + seed)
    theta0, states = twin.draw_start(prob, mn, mx, seed=3000 + seed)
    return prob, mn, mx, theta0, states


def case_of(s):
    kind, n_inst, dim, H, n_in, _, _, _, _, seed = s
    return make_case(kind, n_inst, dim, H, n_in, seed)


def restate(dtype, s, params=None):
    kind, n_inst, dim, H, n_in, iter0, n_iter, rescale, out_mul, seed = s
    prob, mn, mx, theta0, states = case_of(s)
    pmin, pmax = params or (mn.params, mx.params)
    n_sign, lr = twin.schedule(OPTIM_IT)
    r = TR.run(dtype, kind, dim, prob.data, pmin, pmax, lr, n_sign, theta0, states, iter0, n_iter, rescale, out_mul)
    r["state_min"], r["state_max"] = r["states"]
    return r


@functools.lru_cache(maxsize=None)
def reference(s):
    """The float64 and the float32 restatement of a case, computed once."""
    return restate(torch.float64, s), restate(torch.float32, s)


def rel(got, want):
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64).reshape(want.shape) - want).max() / max(np.abs(want).max(), 1e-30))


@functools.lru_cache(maxsize=None)
def group_bound(group):
    worst = max(rel(reference(s)[1][a], reference(s)[0][a]) for s in group for a in ARRAYS)
    return worst, 4 * worst


def gpu_run(s, mn=None, mx=None):
    kind, n_inst, dim, H, n_in, iter0, n_iter, rescale, out_mul, seed = s
    prob, mn0, mx0, theta0, states = case_of(s)
    res = twin.unroll(prob, mn or mn0, mx or mx0, OPTIM_IT, rescale=rescale, out_mul=out_mul, theta0=theta0, states=states,
                      iter0=iter0, n_iter=n_iter, record=("curve", "f", "delta"))
    return dict(curve=res.curve, f=res.f, delta=res.delta, theta=res.theta, state_min=res.states[0], state_max=res.states[1])


def check_against_float64(s, group):
    own, bound = group_bound(tuple(group))
    print("case", s, "float32 torch worst %.3e, bound %.3e" % (own, bound))
    got, r64 = gpu_run(s), reference(s)[0]
    errs = {a: rel(got[a], r64[a]) for a in ARRAYS}
    for a in ARRAYS:
        print("  %-9s err %.3e  (float32 torch %.3e)" % (a, errs[a], rel(reference(s)[1][a], r64[a])))
    for a in ARRAYS:
        assert np.isfinite(np.asarray(got[a])).all(), a
        assert errs[a] <= bound, (a, errs[a], bound)


@pytest.mark.parametrize("s", DELTA)
def test_delta_phase(eng, s):
    check_against_float64(s, DELTA)


@pytest.mark.parametrize("s", RECUR)
def test_rescale_one_sees_every_weight_block(eng, s):
    own, bound = group_bound(tuple(RECUR))
    prob, mn, mx, _, _ = case_of(s)
    base = reference(s)[0]["curve"]
    for which in (0, 1):
        for block in BLOCKS:
            params = [dict(mn.params), dict(mx.params)]
            params[which][block] = np.zeros_like(params[which][block])
            moved = rel(restate(torch.float64, s, params)["curve"], base)
            print("zeroing %s of %s moves the float64 curve by %.3e (bound %.3e)" % (block, ("min", "max")[which], moved, bound))
            assert moved >= 100 * bound, (block, which, moved, bound)
    check_against_float64(s, RECUR)


@pytest.mark.parametrize("s", WIDTHS)
def test_widths(eng, s):
    check_against_float64(s, WIDTHS)


@pytest.mark.parametrize("s", SIGN)
def test_sign_phase(eng, s):
    n_sign, _ = twin.schedule(OPTIM_IT)
    assert n_sign == 7
    smallest = float(np.abs(reference(s)[0]["delta"][:, :n_sign]).min())
    print("min |delta| over the sign iterations (float64): %.3e" % smallest)
    assert smallest >= 1e-3
    check_against_float64(s, SIGN)


@pytest.mark.parametrize("s", SIGN)
def test_zero_head_moves_nothing(eng, s):
    prob, mn, mx, theta0, _ = case_of(s)
    zeroed = []
    for o in (mn, mx):
        sd = o.state_dict()
        sd["output.weight"].zero_()
        sd["output.bias"].zero_()
        zeroed.append(twin.Optimizer(o.hidden_size, use_second=o.use_second).load_state_dict(sd))
    got = gpu_run(s, *zeroed)
    start = theta0.reshape(prob.n_inst, 1, 2 * prob.dim)
    assert np.array_equal(got["curve"], np.broadcast_to(start, got["curve"].shape))
    assert not got["delta"].any() and np.array_equal(got["theta"], theta0)


# 5. continuation and memory discipline, through the C ABI
class Launcher(object):
    def __init__(self, eng, s):
        kind, n_inst, dim, H, n_in, _, _, rescale, out_mul, _ = s
        self.eng, self.s = eng, s
        self.prob, self.mn, self.mx, self.theta0, self.states = case_of(s)
        self.n_sign, self.lr = twin.schedule(OPTIM_IT)

    def device(self, iter0, n_iter):
        kind, n_inst, dim, H, n_in, _, _, rescale, out_mul, _ = self.s
        nets = tuple((o.hidden_size, o.n_in, o.params) for o in (self.mn, self.mx))
        return _engine.TwinDevice(self.eng, nets, (kind, n_inst, dim, self.prob.data),
                                  dict(iter0=iter0, n_iter=n_iter, n_sign=self.n_sign, rescale=rescale, out_mul=out_mul,
                                       sign_lr=self.lr))

    def start(self):
        return [self.eng.tensor(self.theta0)] + [self.eng.tensor(st) for st in self.states]

    def run(self, bufs, iter0, n_iter, record=True):
        n, dim = self.prob.n_inst, self.prob.dim
        outs = [torch.full(shape, float("nan"), dtype=torch.float32, device=self.eng.device)
                for shape in ((n_iter, n, 2 * dim), (n_iter, n), (n_iter, n, dim))] if record else [None] * 3
        rc = self.device(iter0, n_iter).unroll(*bufs, *outs, self.eng._stream())
        assert rc == _abi.L2O_OK, _abi.lib().l2o_last_error()
        torch.cuda.synchronize()
        return [None if o is None else o.cpu().numpy() for o in outs]


def test_continuation_is_bit_identical(eng):
    L = Launcher(eng, spec(4, 7, 5, iter0=1, n_iter=40))
    whole = L.start()
    rec = L.run(whole, 1, 40)
    assert all(not np.isnan(r).any() for r in rec)          # NaN-filled buffers come back fully written
    again = L.start()
    rec2 = L.run(again, 1, 40)
    for a, b in zip(whole + rec, again + rec2):
        assert np.array_equal(a.cpu().numpy() if torch.is_tensor(a) else a, b.cpu().numpy() if torch.is_tensor(b) else b)
    for first in (13, 20):                                   # split at an odd and at an even k
        bufs = L.start()
        r1 = L.run(bufs, 1, first)
        r2 = L.run(bufs, first + 1, 40 - first)
        for w, b in zip(whole, bufs):
            assert torch.equal(w, b), first
        for w, a, b in zip(rec, r1, r2):
            assert np.array_equal(w, np.concatenate([a, b], axis=0)), first
    quiet = L.start()
    L.run(quiet, 1, 40, record=False)                        # curve = fval = delta = NULL
    for w, b in zip(whole, quiet):
        assert torch.equal(w, b)
    ref64 = reference(spec(4, 7, 5, iter0=1, n_iter=40))[0]
    assert rel(rec[0].transpose(1, 0, 2), ref64["curve"][:, 1:]) < 1e-4


@pytest.mark.parametrize("s", OUTMUL)
def test_out_mul(eng, s):
    check_against_float64(s, OUTMUL)


# 7. out-of-range descriptors
@pytest.mark.parametrize("what", ["hidden 97", "dim 17", "kind 5", "kind 1 with dim 2"])
def test_unsupported_descriptors_touch_nothing(eng, what):
    if what == "hidden 97":
        s = spec(3, 5, H=(97, 50))
    elif what == "dim 17":
        s = spec(4, 2, 17, H=(8, 8))
    else:
        s = spec(1, 6, H=(8, 8))
    L = Launcher(eng, s)
    dev = L.device(1, 4)
    n, dim = L.prob.n_inst, L.prob.dim
    if what == "kind 5":
        dev.problem.kind = 5
    elif what == "kind 1 with dim 2":
        dev.problem.dim, dev.problem.n_inst, n, dim = 2, 3, 3, 2      # the same 6 rows
    assert _abi.lib().l2o_twin_supported(dev.nets[0], dev.nets[1], dev.problem) == 0
    bufs = L.start()
    outs = [torch.full(shape, 7.0, dtype=torch.float32, device=eng.device) for shape in ((4, n, 2 * dim), (4, n), (4, n, dim))]
    before = [t.clone() for t in bufs + outs]
    rc = dev.unroll(*bufs, *outs, eng._stream())
    torch.cuda.synchronize()
    assert rc == _abi.L2O_ERR_UNSUPPORTED
    assert all(torch.equal(a, b) for a, b in zip(before, bufs + outs))
    if what == "hidden 97":
        assert _abi.lib().l2o_twin_state_floats(dev.nets[0], 5) == 0 and _abi.lib().l2o_twin_state_floats(dev.nets[1], 5) == 4 * 50 * 5


# 8. the driver
def test_evaluate_twin_on_the_seesaw_fixture(eng, tmp_path):
    drv = load_driver()
    cfg = json.load(open(os.path.join(GOLDEN, "seesaw_test.json")))
    cfg.update(n_test=8, test_epochs=2, test_optim_iter=40)
    (tmp_path / "cfg.json").write_text(json.dumps(cfg))
    drv.main(["--config", str(tmp_path / "cfg.json"), "--root", GOLDEN, "--out", str(tmp_path / "out"), "--random-weights"])
    got = json.load(open(tmp_path / "out" / "twin_eval.json"))
    params = drv.load_config(str(tmp_path / "cfg.json"))
    prob, mn, mx, theta0, states = drv.setup(params, GOLDEN, random_weights=True)
    n_sign, lr = twin.schedule(40)
    r = TR.run(torch.float32, 3, 1, prob.data, mn.params, mx.params, lr, n_sign, theta0, states, 1, 40, cfg["rescale"], 1.0)
    want = drv.summarize(params, *TR.distances(3, prob.data, r["curve"], 1))
    own, bound = group_bound(tuple(DELTA))
    scale = float(np.abs(r["curve"]).max())
    assert got["runs"] == 16 and got["burn_in"] == 20
    for key in ("mean_distance_u", "mean_distance_v"):
        print(key, got[key], want[key], "bound %.3e x largest curve entry %.3e" % (bound, scale))
        assert abs(got[key] - want[key]) <= bound * scale, key
