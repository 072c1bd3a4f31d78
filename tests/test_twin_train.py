"""The Twin-L2O meta-gradient (csrc/l2o_twin_train.h: k_twin_record, k_twin_bptt, k_twin_wgrad) on the MI355X, through
twin.meta_gradient and through the C ABI, against autograd of the reference's graph in float64 (twin_train_reference.py).

Criterion (tests/test_twin.py's).  Every gradient array is compared relative to its own largest float64 entry.  The bound is
4 x the float32 autograd restatement's own worst such error against float64 over the group of cases, computed here on the
CPU (the kernels sum rows, iterations and k in another order than torch).  An array whose float64 value is identically zero
must come back as exactly 0.0.  Every case that crosses the sign phase first asserts, on the float64 reference, that
min |delta| over its sign iterations is >= 1e-3: a sign flipped in float32 would move the point and hide behind the bound.
The tests print every figure before they assert (float32 torch worst, bound, kernel worst per case).

Measured on one MI355X, build id 3fc2befbafe9c8e3 (float32 torch worst -> bound; kernel worst): rows and tiles 8.68e-07 -> 3.47e-06; 1.47e-06.  Recurrence
3.90e-07 -> 1.56e-06; 1.51e-06 (seesaw x 17, segment 21 ... 30, output.bias of the min network: the plain sum of seeds of both
signs, sum |g| / |sum g| = 24; 1.49e-06 of it is the float32 error of the forward's point, which is l2o_twin_unroll's bit for
bit -- with the seed and that sum in float32 it was 2.19e-06 and missed, so both are double now: DESIGN.md 3.13); zeroing a
recurrent block moves the float64 gradient by 0.14 ... 3.1.  Widths 1.45e-06 -> 5.82e-06; 2.04e-06.  Weights 9.20e-07 ->
3.68e-06; 1.95e-06.  Sign boundary 2.90e-07 -> 1.16e-06; 4.72e-07, min |delta| over the sign iterations 1.2e-02 ... 2.8e-02.
Zero head weight: 4.82e-07 -> 1.93e-06; 1.09e-06.
(The float32 restatement runs on the CPU of the machine at hand, so its worst error moves in the last digits.)"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import twin_train_reference as TT
from open_l2o_amd import _abi, _engine, twin
from test_twin_cpu import make_data

pytestmark = pytest.mark.gpu


@pytest.fixture
def eng():
    e, old = _engine.HipEngine(), _engine._default_engine
    _engine.set_default_engine(e)
    try:
        yield e
    finally:
        _engine.set_default_engine(old)


def spec(kind, n_inst, dim=1, H=(50, 50), n_in=2, optim_it=20, iter0=5, n_iter=4, rescale=1e-4, out_mul=1.0, seed=0,
         keep=None, batch=None):
    """keep: None or the period p of the 0/1 instance weights (instance i is kept iff i % p != 1); batch: batch_size."""
    return (kind, n_inst, dim, H, n_in, optim_it, iter0, n_iter, rescale, out_mul, seed, keep, batch)


# optim_it = 20: n_sign = 3, segment 5 ... 8 of unroll_unit 2.  Rows at, below and above a tile; matrix games whose instances
# would straddle 16-row tiles (tiles of 3, 3, 1 instances; one instance per tile; 5, 5, 1)
ROWS = [spec(3, n) for n in (1, 16, 17)] + [spec(4, n, d) for n, d in ((7, 5), (2, 16), (11, 3))] + [spec(1, 17), spec(2, 17)]
# rescale = 1, unroll_unit 5 of optim_it 100 (n_sign = 19): segment 11 ... 20 (nine sign iterations and one delta step: the
# max network alone gets a gradient) and segment 21 ... 30
RECUR = [spec(k, n, d, optim_it=100, iter0=i0, n_iter=10, rescale=1.0) for k, n, d in ((3, 17, 1), (4, 7, 5)) for i0 in (11, 21)]
# widths: padded (5, 50), two k-step groups of four (80), the largest (96), two different nets, one input column;
# unroll_unit 1: every iteration is a segment's first or last (w_k is 2 then 1)
WIDTHS = [spec(4, 7, 5, H=(5, 5)), spec(4, 7, 5, H=(80, 80)), spec(4, 7, 5, H=(96, 96)), spec(4, 7, 5, H=(50, 80)),
          spec(4, 7, 5, n_in=1), spec(3, 17, n_iter=2), spec(4, 7, 5, n_iter=2)]
# weights: out_mul, 0/1 instance weights (against the gradient of the kept instances alone), batch_size != n_inst
WEIGHTS = [spec(3, 17, out_mul=0.5), spec(3, 17, keep=3), spec(4, 7, 5, keep=2), spec(3, 17, batch=128), spec(4, 7, 5, batch=3)]
# a segment across the end of the sign phase (1 ... 4 of optim_it 20) and one wholly inside it (1 ... 2)
SIGN = [spec(3, 17, iter0=1), spec(4, 7, 5, iter0=1)]
BLOCKS = ("recurs.weight_hh", "recurs2.weight_ih", "recurs2.weight_hh")


@functools.lru_cache(maxsize=None)
def make_case(kind, n_inst, dim, H, n_in, seed):
    prob = twin.problem(kind, make_data(kind, n_inst, dim, 100 + seed), dim)
    mn = twin.Optimizer(H[0], use_second=n_in == 2, seed=1000 + seed)
    mx = twin.Optimizer(H[1], use_second=n_in == 2, seed=2000 + seed)
    theta0, states = twin.draw_start(prob, mn, mx, seed=3000 + seed)
    return prob, mn, mx, theta0, states


def case_of(s):
    return make_case(s[0], s[1], s[2], s[3], s[4], s[10])


def weights_of(s):
    n, keep = s[1], s[11]
    return None if keep is None else np.float32([0.0 if i % keep == 1 else 1.0 for i in range(n)])


def restate(dtype, s, params=None):
    """Autograd in `dtype`.  With 0/1 instance weights: of the kept instances ALONE (their rows of the data, the start and the
    states), divided by the whole batch."""
    kind, n_inst, dim, H, n_in, optim_it, iter0, n_iter, rescale, out_mul, seed, keep, batch = s
    prob, mn, mx, theta0, states = case_of(s)
    pmin, pmax = params or (mn.params, mx.params)
    n_sign, lr = twin.schedule(optim_it)
    data, w = prob.data, weights_of(s)
    if w is not None:
        idx = np.flatnonzero(w)
        rows = (idx[:, None] * dim + np.arange(dim)[None, :]).reshape(-1)
        data, theta0, states = data[idx], theta0[idx], tuple(st[:, :, rows] for st in states)
    return TT.segment_grad(dtype, kind, dim, data, pmin, pmax, lr, n_sign, theta0, states, iter0, n_iter, rescale, out_mul,
                           batch_size=batch or n_inst)


@functools.lru_cache(maxsize=None)
def reference(s):
    """The float64 and the float32 autograd of a case, computed once."""
    return restate(torch.float64, s), restate(torch.float32, s)


def rel(got, want):
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64).reshape(want.shape) - want).max() / max(np.abs(want).max(), 1e-300))


def arrays(grads):
    return {("min", "max")[i] + ":" + k: g for i, gs in enumerate(grads) for k, g in gs.items()}


@functools.lru_cache(maxsize=None)
def group_bound(group):
    worst = 0.0
    for s in group:
        r64, r32 = reference(s)
        a64, a32 = arrays(r64["grads"]), arrays(r32["grads"])
        worst = max([worst] + [rel(a32[k], a64[k]) for k in a64 if a64[k].any()])
    return worst, 4 * worst


def gpu_run(s, mn=None, mx=None, weight="spec"):
    kind, n_inst, dim, H, n_in, optim_it, iter0, n_iter, rescale, out_mul, seed, keep, batch = s
    prob, mn0, mx0, theta0, states = case_of(s)
    return twin.meta_gradient(prob, mn or mn0, mx or mx0, optim_it, iter0, n_iter, theta0, states, rescale=rescale,
                              out_mul=out_mul, batch_size=batch, inst_weight=weights_of(s) if isinstance(weight, str) else weight)


def sign_condition(s):
    """A case that crosses the sign phase: min |delta| over its sign iterations in float64 is >= 1e-3."""
    n_sign = twin.schedule(s[5])[0]
    n_here = min(max(n_sign - s[6] + 1, 0), s[7])
    if n_here:
        smallest = float(np.abs(reference(s)[0]["delta"][:, :n_here]).min())
        print("min |delta| over the %d sign iterations (float64): %.3e" % (n_here, smallest))
        assert smallest >= 1e-3
    return n_here


def check_against_float64(s, group, got=None):
    own, bound = group_bound(tuple(group))
    print("case", s, "float32 torch worst %.3e, bound %.3e" % (own, bound))
    sign_condition(s)
    got = got or gpu_run(s)
    r64, r32 = reference(s)
    a64, a32, ag = arrays(r64["grads"]), arrays(r32["grads"]), arrays(got.grads)
    errs = {}
    for k in a64:
        assert ag[k].shape == a64[k].shape and np.isfinite(ag[k]).all(), k
        if a64[k].any():
            errs[k] = rel(ag[k], a64[k])
            print("  %-24s err %.3e  (float32 torch %.3e)  largest %.3e" % (k, errs[k], rel(a32[k], a64[k]), np.abs(a64[k]).max()))
        else:
            print("  %-24s identically zero in float64" % k)
    print("  kernel worst %.3e" % max(errs.values()))
    for k in a64:
        if a64[k].any():
            assert errs[k] <= bound, (k, errs[k], bound)
        else:
            assert not ag[k].any(), k
    assert got.loss == pytest.approx(r64["loss"], rel=1e-5, abs=1e-6)      # (the kept instances alone give the weighted loss)
    return got


@pytest.mark.parametrize("s", ROWS)
def test_rows_and_tiles(eng, s):
    check_against_float64(s, ROWS)


@pytest.mark.parametrize("s", RECUR)
def test_rescale_one_sees_every_recurrent_block(eng, s):
    own, bound = group_bound(tuple(RECUR))
    prob, mn, mx, _, _ = case_of(s)
    base = arrays(reference(s)[0]["grads"])
    if s[6] == 11:                                               # nine sign iterations, then one max step
        assert sign_condition(s) == 9
        assert all(not g.any() for k, g in base.items() if k.startswith("min:"))
        assert all(g.any() for k, g in base.items() if k.startswith("max:"))
    for which in ((1,) if s[6] == 11 else (0, 1)):
        for block in BLOCKS:
            params = [dict(mn.params), dict(mx.params)]
            params[which][block] = np.zeros_like(params[which][block])
            other = arrays(restate(torch.float64, s, params)["grads"])
            pre = ("min:", "max:")[which]
            moved = max(rel(other[k], base[k]) for k in base if k.startswith(pre) and k != pre + block)
            print("zeroing %s of %s moves its float64 gradient by %.3e (bound %.3e)" % (block, pre[:3], moved, bound))
            assert moved >= 100 * bound, (block, which, moved, bound)
    check_against_float64(s, RECUR)


@pytest.mark.parametrize("s", WIDTHS)
def test_widths(eng, s):
    got = check_against_float64(s, WIDTHS)
    if s[4] == 1:
        assert got.grads[0]["recurs.weight_ih"].shape == (200, 1)


@pytest.mark.parametrize("s", WEIGHTS)
def test_weights(eng, s):
    check_against_float64(s, WEIGHTS)


@pytest.mark.parametrize("s", SIGN)
def test_across_and_inside_the_sign_phase(eng, s):
    assert twin.schedule(20)[0] == 3
    got = check_against_float64(s, SIGN)                          # 1 ... 4: three sign iterations, one max step
    assert all(not g.any() for g in got.grads[0].values())
    inside = gpu_run(s[:7] + (2,) + s[8:])                        # 1 ... 2: wholly in the sign phase
    for gs in inside.grads:
        for k, g in gs.items():
            assert np.array_equal(g, np.zeros_like(g)), k         # all zero, no NaN
    assert np.isfinite(inside.loss) and inside.loss != 0.0


@pytest.mark.parametrize("s", [spec(3, 17), spec(4, 7, 5)])
def test_forward_has_the_bits_of_unroll_and_backward_repeats(eng, s):
    kind, n_inst, dim, H, n_in, optim_it, iter0, n_iter, rescale, out_mul, seed, keep, batch = s
    prob, mn, mx, theta0, states = case_of(s)
    a = gpu_run(s)
    u = twin.unroll(prob, mn, mx, optim_it, rescale=rescale, out_mul=out_mul, theta0=theta0, states=states, iter0=iter0,
                    n_iter=n_iter, record=("curve", "f", "delta"))
    for name in ("theta", "curve", "f", "delta"):
        assert np.array_equal(getattr(a, name), getattr(u, name)), name
    assert all(np.array_equal(x, y) for x, y in zip(a.states, u.states))
    b = gpu_run(s)                                                # twice: the same bits
    ones = gpu_run(s, weight=np.ones(n_inst, np.float32))         # all ones: the bits of NULL
    for other in (b, ones):
        for g0, g1 in zip(a.grads, other.grads):
            for k in twin.PARAM_NAMES:
                assert np.array_equal(g0[k], g1[k]), k
    assert b.loss == a.loss


ZERO_HEAD = [spec(3, 17, rescale=1.0), spec(4, 7, 5, rescale=1.0)]


@functools.lru_cache(maxsize=None)
def zero_head(s):
    """(the case's two networks with output.weight zeroed, its float64 and its float32 autograd)"""
    prob, mn, mx, _, _ = case_of(s)
    zeroed = []
    for o in (mn, mx):
        sd = o.state_dict()
        sd["output.weight"].zero_()
        zeroed.append(twin.Optimizer(o.hidden_size, use_second=o.use_second).load_state_dict(sd))
    params = (zeroed[0].params, zeroed[1].params)
    return zeroed, restate(torch.float64, s, params), restate(torch.float32, s, params)


@pytest.mark.parametrize("s", ZERO_HEAD)
def test_zero_head_weight_stops_the_lstm_gradients(eng, s):
    # the bound: 4 x the float32 restatement's own worst error on the head's gradients of these two cases
    own = max(rel(g32[k], g64[k]) for c in ZERO_HEAD for g64, g32 in zip(zero_head(c)[1]["grads"], zero_head(c)[2]["grads"])
              for k in ("output.weight", "output.bias"))
    bound = 4 * own
    print("float32 torch worst %.3e, bound %.3e" % (own, bound))
    zeroed, r64, _ = zero_head(s)
    got = gpu_run(s, *zeroed)
    for gs, ws in zip(got.grads, r64["grads"]):
        for k in twin.PARAM_NAMES:
            if k.startswith("recurs"):
                assert np.array_equal(gs[k], np.zeros_like(gs[k])) and not ws[k].any(), k
            else:
                print(k, "err %.3e (bound %.3e), largest %.3e" % (rel(gs[k], ws[k]), bound, np.abs(ws[k]).max()))
                assert ws[k].any() and rel(gs[k], ws[k]) <= bound, k


def test_split_calls_stay_inside_the_queried_sizes(eng):
    s = spec(4, 7, 5, H=(50, 80))
    kind, n_inst, dim, H, n_in, optim_it, iter0, n_iter, rescale, out_mul, seed, keep, batch = s
    prob, mn, mx, theta0, states = case_of(s)
    n_sign, lr = twin.schedule(optim_it)
    nets = tuple((o.hidden_size, o.n_in, o.params) for o in (mn, mx))
    dev = _engine.TwinDevice(eng, nets, (kind, n_inst, dim, prob.data),
                             dict(iter0=iter0, n_iter=n_iter, n_sign=n_sign, rescale=rescale, out_mul=out_mul, sign_lr=lr))
    SENTINEL, PAD = -7.25, 4096

    def padded(n, fill=SENTINEL):
        t = torch.full((n + PAD,), fill, dtype=torch.float32, device=eng.device)
        return t, t[:n]
    n_work = dev.work_floats()
    assert n_work == 3 * 4 * (64 + 2 * 20 * 448 + 48 + 2 * 20 * 256)           # 3 tiles, 4 iterations, nt = 20 of H = 80
    work_all, work = padded(n_work)
    outs = [padded(n) for n in (n_iter * n_inst * 2 * dim, n_iter * n_inst, n_iter * n_inst * dim)]
    bufs = [eng.tensor(theta0)] + [eng.tensor(st) for st in states]
    seg = dev.segment(1.0 / n_inst)
    rc = dev.train_forward(seg, *bufs, *(o[1] for o in outs), work, eng._stream())
    assert rc == _abi.L2O_OK, _abi.lib().l2o_last_error()
    grads = [{k: padded(int(np.prod(o.params[k].shape))) for k in twin.PARAM_NAMES} for o in (mn, mx)]
    rc = dev.train_backward(seg, work, [{k: v[1] for k, v in g.items()} for g in grads], eng._stream())
    assert rc == _abi.L2O_OK, _abi.lib().l2o_last_error()
    torch.cuda.synchronize()
    for whole, part in [(work_all, work)] + outs + [v for g in grads for v in g.values()]:
        assert bool((whole[part.numel():] == SENTINEL).all())
        assert not bool((part == SENTINEL).any()) or part is work              # every output entry is written
    want = gpu_run(s)
    for g, w in zip(grads, want.grads):
        for k in twin.PARAM_NAMES:
            assert np.array_equal(g[k][1].cpu().numpy().reshape(w[k].shape), w[k]), k
    # refused descriptors launch nothing: the buffers keep their bits
    before = work_all.clone()
    bad = _abi.TwinSegment(_abi.TwinRun(iter0 + 1, n_iter, n_sign, rescale, out_mul, dev.run.sign_lr), 1.0 / n_inst, None)
    assert dev.train_forward(bad, *bufs, *(o[1] for o in outs), work, eng._stream()) == _abi.L2O_ERR_UNSUPPORTED
    assert dev.train_backward(bad, work, [{k: v[1] for k, v in g.items()} for g in grads], eng._stream()) == _abi.L2O_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.equal(before, work_all)
