"""problems.vgg16_cifar10 on the MI355X: l2o_vgg16_fg (csrc/l2o_vgg16.h) against the float64 torch reference
(vgg16_reference.py) at narrow widths -- (8, 16, 24, 40, 72): no width a multiple of 32 below the last, one just past 64, so
with odd minibatches every tile edge in M, N and K is in play -- and at the reference's widths; the bit contracts of the
entry point; the engine's wiring; short unrolls on the graph's step path against a float64 host unroll; one first-order
meta-gradient; and the RNNProp evaluation driver.

Bounds (the project's, as test_lenet.py): a gradient block within GRAD_TOL (5e-4) of its largest float64 entry, or 3 x the
float32 reference's own distance where that is larger; the loss within 1e-5 relative, or the same 3 x rule.  Every parity
case asserts that the float32 reference is itself within a third of GRAD_TOL, so the bound in force is GRAD_TOL.  Every
case runs at two weight scales: ``sample`` (O(1) activations through all thirteen layers) and ``init`` (the reference's
initialisation, where the float32 loss is exactly log 10 and the first block's gradient entries are of the order 1e-15)."""
import numpy as np
import pytest

import imagenet_harness as H
import oracle as O
import vgg16_reference as R
from helpers import ORACLE_CFGS, block_errors, make_params
from imagenet_harness import eng  # noqa: F401  (the fixture)
from open_l2o_amd import _abi, _engine, meta, problems
from open_l2o_amd.session import Session
from test_meta_api import _net_config
from test_training_gradient import GRAD_TOL, Trainer

pytestmark = pytest.mark.gpu

NET = H.NETS["vgg16"]                  # (its problem factory, unroll and driver run at the narrow widths)
NARROW, REFERENCE = R.NARROW_CHANNELS, R.REFERENCE_CHANNELS
N_DATA = 64
_cache = {}
# The minibatch of every parity case is drawn from default_rng(1000 * seed + batch), with the seed below.  ReLU masks and
# pool arg-maxes are decisions: a pre-activation that float32 rounding carries across one changes a gradient block by about
# 1e-2 / minibatch of its largest entry (seen with float32 torch itself at the reference's widths, minibatch 5: 8.5e-3), so
# a parity case means something only on inputs whose decisions float32 cannot flip.  The seed of a case is the one, of the
# first few hundred, whose float64 pre-activations keep the largest distance from any decision that matters, measured in
# units of a float32 sum's rounding (vgg16_reference._margin); the case asserts that distance to be >= MIN_MARGIN units
# and the float32 reference to be within GRAD_TOL / 3.  Both are conditions on the inputs, fixed before the kernels run.
MIN_MARGIN = 2.0
MINIBATCH_SEED = {
    (NARROW, "sample", 2): 81, (NARROW, "sample", 3): 374, (NARROW, "sample", 37): 1, (NARROW, "sample", 128): 18,
    (NARROW, "init", 2): 390, (NARROW, "init", 3): 186, (NARROW, "init", 37): 71, (NARROW, "init", 128): 3,
    (REFERENCE, "sample", 2): 258, (REFERENCE, "sample", 5): 204, (REFERENCE, "init", 2): 313, (REFERENCE, "init", 5): 271,
    (NARROW, "sample", 1024): 7,
}


_data = H.uniform_cifar                # (n = N_DATA, seed = 0)


def _weights(channels, scale, seed=1):
    return (R.sample_weights if scale == "sample" else R.init_weights)(channels, seed)


def _reference(channels, scale, batch):
    """(rows, float64 loss, float64 gradients, float32 loss, float32 gradients): computed once per case and shared."""
    key = ("ref", channels, scale, batch)
    if key not in _cache:
        data = _data()
        net = R.Vgg16(data["images"], data["labels"], channels)
        w = _weights(channels, scale)
        rows = np.random.default_rng(1000 * MINIBATCH_SEED[channels, scale, batch] + batch).integers(0, N_DATA, batch)
        f64, g64 = net.fg([a.astype(np.float64) for a in w], rows)
        margin = min(net.last_margins)
        print("decision margin %.2f units" % margin)
        assert margin >= MIN_MARGIN, (channels, scale, batch, net.last_margins)
        f32, g32 = net.fg(w, rows)
        _cache[key] = (rows, float(f64), g64, float(f32), g32)
    return _cache[key]


def _desc(eng, channels, batch, data=None):
    data = data or _data()
    return _engine.Vgg16Desc(batch, channels, eng.tensor(data["images"].reshape(len(data["images"]), -1)),
                             eng.int_tensor(data["labels"]))


def _run_fg(eng, d, rows, w, want_grad=True):
    return H.run_fg(eng, NET, d, rows, w, want_grad)


def _check_fg(eng, channels, scale, batch):
    rows, f64, g64, f32, g32 = _reference(channels, scale, batch)
    w = _weights(channels, scale)
    loss, grads = _run_fg(eng, _desc(eng, channels, batch), rows, w)
    got_f = float(loss[0])
    own_f = abs(f32 - f64)
    print("loss", got_f, f64, "rel %.3e (float32 torch %.3e)" % (abs(got_f - f64) / abs(f64), own_f / abs(f64)))
    assert own_f <= 1e-5 / 3 * abs(f64)
    failures = []
    if not abs(got_f - f64) <= max(1e-5 * abs(f64), 3 * own_f):
        failures.append(("loss", got_f, f64))
    for nm, g, want, w32 in zip(R.names(), grads, g64, g32):
        scale64 = float(np.abs(want).max())
        assert scale64 > 1e-30, nm
        err, bnd = H.bound(g.astype(np.float64).reshape(want.shape), want, w32)
        own = float(np.abs(w32 - want).max())
        print("%-24s err %.3e own %.3e of max %.3e" % (nm, err / scale64, own / scale64, scale64))
        assert own <= GRAD_TOL / 3 * scale64, (nm, own, scale64)
        if not err <= bnd:
            failures.append((nm, err / scale64, own / scale64))
    assert not failures, failures
    return loss, grads


# ------------------------------------------------------------------------------------------------------------------
# 1. one evaluation: l2o_vgg16_fg against float64
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", ["sample", "init"])
@pytest.mark.parametrize("batch", [2, 3, 37, 128])
def test_fg_narrow_vs_float64(eng, batch, scale):
    """Minibatch 3 gives M = 12 at the 2 x 2 layers; 37 an odd count of rows in every layer; 128 several reduction splits in
    every weight gradient."""
    _check_fg(eng, NARROW, scale, batch)


@pytest.mark.parametrize("scale", ["sample", "init"])
@pytest.mark.parametrize("batch", [2, 5])
def test_fg_reference_width_vs_float64(eng, batch, scale):
    _check_fg(eng, REFERENCE, scale, batch)


def test_fg_minibatch_1024_narrow(eng):
    """The largest minibatch, for the scratch arithmetic (1024 x 32 x 32 rows, 512 reduction splits in block 1): the loss and
    every gradient block against float64."""
    _check_fg(eng, NARROW, "sample", 1024)


# ------------------------------------------------------------------------------------------------------------------
# 2. the bit contracts of the entry point
# ------------------------------------------------------------------------------------------------------------------
def _raw_call(eng, channels, batch, rows, w, scratch, want_grad=True):
    """l2o_vgg16_fg through the binding with a scratch buffer of the test's own."""
    import ctypes as C
    data = _data()
    images, labels = eng.tensor(data["images"].reshape(N_DATA, -1)), eng.int_tensor(data["labels"])
    c = _abi.Vgg16()
    c.batch, c.n_data, c.flags = batch, N_DATA, 0
    for k, n in enumerate(channels):
        c.channels[k] = n
    c.images, c.labels = C.c_void_p(images.data_ptr()), C.c_void_p(labels.data_ptr())
    idx = eng.int_tensor(rows)
    ws = [eng.tensor(a) for a in w]
    grads = [eng.zeros(*a.shape) for a in w] if want_grad else None
    loss = eng.zeros(1)
    _abi.check(eng.lib.l2o_vgg16_fg(C.byref(c), C.c_void_p(idx.data_ptr()), _engine._ptr_array(ws), _engine._ptr(loss),
                                    _engine._ptr_array(grads), _engine._ptr(scratch), eng._stream()))
    n = int(eng.lib.l2o_vgg16_scratch_floats(C.byref(c)))
    return eng.to_numpy(loss).copy(), None if grads is None else [eng.to_numpy(g).copy() for g in grads], n


def test_bit_contracts(eng):
    import ctypes as C
    import torch
    w = _weights(NARROW, "sample")
    rows128 = np.random.default_rng(5).integers(0, N_DATA, 128)
    rows2 = rows128[:2]
    d128, d2 = _desc(eng, NARROW, 128), _desc(eng, NARROW, 2)
    loss_a, grads_a = _run_fg(eng, d128, rows128, w)
    loss_b, grads_b = _run_fg(eng, d128, rows128, w)
    loss_f, _ = _run_fg(eng, d128, rows128, w, want_grad=False)
    assert loss_a.tobytes() == loss_b.tobytes() == loss_f.tobytes() and np.isfinite(loss_a).all()
    for a, b in zip(grads_a, grads_b):
        assert a.tobytes() == b.tobytes()
    # minibatch 2 after minibatch 128 on the same (cached) scratch buffer: minibatch 2's bits
    loss_2, grads_2 = _run_fg(eng, d2, rows2, w)
    fresh = _engine.HipEngine()
    loss_2f, grads_2f = _run_fg(fresh, _desc(fresh, NARROW, 2), rows2, w)
    assert loss_2.tobytes() == loss_2f.tobytes()
    for a, b in zip(grads_2, grads_2f):
        assert a.tobytes() == b.tobytes()
    # a NaN-filled scratch of exactly scratch_floats: the same bits, and the guard behind it untouched
    c = _abi.Vgg16()
    c.batch, c.n_data = 128, N_DATA
    for k, n in enumerate(NARROW):
        c.channels[k] = n
    n = int(eng.lib.l2o_vgg16_scratch_floats(C.byref(c)))
    guard = 4096
    buf = torch.full((n + guard,), float("nan"), dtype=torch.float32, device=eng.device)
    buf[n:] = 12345.0
    loss_n, grads_n, n_again = _raw_call(eng, NARROW, 128, rows128, w, buf)
    assert n_again == n and loss_n.tobytes() == loss_a.tobytes()
    for a, b in zip(grads_a, grads_n):
        assert a.tobytes() == b.tobytes()
    assert bool((buf[n:] == 12345.0).all())
    loss_nf, _, _ = _raw_call(eng, NARROW, 128, rows128, w, buf.fill_(float("nan")), want_grad=False)
    assert loss_nf.tobytes() == loss_a.tobytes()


# ------------------------------------------------------------------------------------------------------------------
# 3. the engine's wiring
# ------------------------------------------------------------------------------------------------------------------
def test_engine_wiring(eng):
    """Minibatches 4, 2, 8: forward only gives the bits of the call with gradients, the scratch is kept while it is large
    enough and replaced by a larger one when not; then the variable-count, minibatch and width refusals."""
    entry = _engine.STEP_OPTIMIZEES[_abi.PROB_VGG16]
    data = _data(8, seed=1)
    images, labels = eng.tensor(data["images"].reshape(8, -1)), eng.int_tensor(data["labels"])
    w = _weights(NARROW, "sample", seed=2)
    ws = [eng.tensor(a) for a in w]

    def run(batch):
        d = entry.desc(batch, NARROW, images, labels)
        idx = eng.int_tensor(np.arange(batch)[::-1] % 8)
        loss, loss_f, grads = eng.zeros(1), eng.zeros(1), [eng.zeros(*a.shape) for a in w]
        eng.vgg16_fg(d, idx, ws, loss, grads)
        eng.vgg16_fg(d, idx, ws, loss_f, None)
        loss, loss_f = eng.to_numpy(loss), eng.to_numpy(loss_f)
        assert np.isfinite(loss).all() and loss.tobytes() == loss_f.tobytes()
        assert all(np.isfinite(eng.to_numpy(g)).all() for g in grads)
        return getattr(eng, entry.scratch)

    assert entry.scratch not in eng.__dict__
    s4 = run(4)
    assert run(2) is s4
    s8 = run(8)
    assert s8 is not s4 and s8.numel() > s4.numel()
    assert run(4) is s8
    loss = eng.zeros(1)
    idx = eng.int_tensor(np.arange(2))
    with pytest.raises(ValueError) as ei:
        eng.vgg16_fg(entry.desc(2, NARROW, images, labels), idx, ws[:27], loss, None)
    assert str(ei.value) == "l2o_vgg16_fg: 27 variables (it takes 28)"
    with pytest.raises(ValueError) as ei:
        eng.vgg16_fg(entry.desc(2, NARROW, images, labels), idx, ws, loss, ws[:-1])
    assert str(ei.value) == "l2o_vgg16_fg: 28 variables (it takes 28)"
    for batch, channels in ((1, NARROW), (1025, NARROW), (2, (8, 16, 24, 40, 70)), (2, (8, 16, 24, 40))):
        with pytest.raises(_abi.L2OUnsupported) as ei:
            eng.vgg16_fg(entry.desc(batch, channels, images, labels), idx, ws, loss, None)
        assert str(ei.value) == "libl2o_hip error -2: l2o_vgg16_fg: unsupported minibatch %d or channels %r" % (batch,
                                                                                                                 channels)
    assert getattr(eng, entry.scratch) is s8


# ------------------------------------------------------------------------------------------------------------------
# 4. unrolls on the graph's step path
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", ["dm_logsign", "rnnprop"])
def test_unroll_narrow_vs_float64(eng, net):
    """Three steps at narrow widths with a fixed sampler against the float64 host unroll; fx by test_lenet.py's rule.  The
    variables start at O(1)-activation weights (an x the optimizer moves visibly); the graph's own initialisation is what
    test_unroll_reference_width runs from."""
    T, batch = 3, 16
    idx = np.random.default_rng(42).integers(0, N_DATA, size=(T + 1, batch))
    H.check_unroll_vs_float64(eng, NET, net, T, batch, _data(), idx, w0=_weights(NARROW, "sample", seed=45))


def test_unroll_reference_width(eng):
    """Two optimizer steps at the reference's widths (14.7 M coordinates), minibatch 2, as two chained one-step unrolls so
    that x is read after each step.  Each fx is checked against the float64 loss at the x the device held; the update of
    the first and last 256 coordinates of every variable against a float64 LSTM step on those coordinates given the
    device's own gradient (the net is coordinate-wise, so a sample of coordinates is exact): what an addressing error at
    2.36 M coordinates per variable would break."""
    batch, n_steps = 2, 2
    data = _data()
    idx = np.random.default_rng(61).integers(0, N_DATA, size=(2 * n_steps, batch))
    calls = {"n": 0}

    def sampler(ne, b, nd):
        out = idx[calls["n"]:calls["n"] + ne]
        calls["n"] += ne
        return out

    cfg = O.DM_LOGSIGN
    params = make_params(cfg, seed=62, trained_like=True)
    p64 = {m: {v: a.astype(np.float64) for v, a in d.items()} for m, d in params.items()}
    meta.set_random_seed(63)
    problem = problems.vgg16_cifar10("cifar10", batch_size=batch, data=data, sampler=sampler)
    optimizer = meta.MetaOptimizer(**_net_config(cfg, params))
    ml = optimizer.meta_loss(problem, 1)
    ref = R.Vgg16(data["images"], data["labels"], REFERENCE)
    d = _desc(eng, REFERENCE, batch)
    w0 = _weights(REFERENCE, "sample", seed=64)
    with Session() as sess:
        sess.run(ml.reset)
        for v, a in zip(optimizer.graph.x, w0):
            v.load(a)
        x = [np.asarray(v.eval()).copy() for v in optimizer.graph.x]
        sizes = [a.size for a in x]
        assert sum(sizes) == 14719818
        pick = [np.unique(np.r_[np.arange(min(256, n)), np.arange(max(0, n - 256), n)]) for n in sizes]
        states = [O.net_initial_state(cfg, len(pk), np.float64) for pk in pick]
        for k in range(n_steps):
            _, grads = _run_fg(eng, d, idx[2 * k], x)                     # the gradient the step consumes, bit for bit
            res = optimizer.graph.execute({}, True)
            x_new = [np.asarray(a).copy() for a in res["x"]]
            fx = np.asarray(res["fx_array"], np.float64)
            want = [ref.fg([a.astype(np.float64) for a in xs], idx[2 * k + j], False)[0] for j, xs in enumerate((x, x_new))]
            for j in range(2):
                print("step", k, "fx", j, fx[j], want[j])
                assert abs(fx[j] - want[j]) <= 1e-5 * abs(want[j]), (k, j, fx[j], want[j])
            for v, (pk, g, a, b) in enumerate(zip(pick, grads, x, x_new)):
                delta, states[v] = O.net_apply(cfg, p64, g.reshape(-1)[pk].astype(np.float64), states[v])
                got = b.reshape(-1)[pk].astype(np.float64) - a.reshape(-1)[pk].astype(np.float64)
                scale = max(float(np.abs(delta).max()), 1e-30)
                err = float(np.abs(got - delta).max())
                # the update is x + delta in float32: half an ulp of x on top of the net's own float32 rounding
                ulp = float(np.abs(a.reshape(-1)[pk]).max()) * 2.0 ** -24
                assert err <= GRAD_TOL * scale + ulp, (k, R.names()[v], err, scale)
            x = x_new
    assert optimizer.graph.last_path == "steps" and calls["n"] == 2 * n_steps


# ------------------------------------------------------------------------------------------------------------------
# 5. the first-order meta-gradient at narrow widths
# ------------------------------------------------------------------------------------------------------------------
def test_meta_gradient_vs_float64(eng):
    T, batch = 3, 16
    data = _data()
    name = "dm_logsign"
    params = make_params(ORACLE_CFGS[name], seed=52, trained_like=True)
    meta.set_random_seed(53)
    tr = Trainer(eng, name, params, problems.vgg16_cifar10("cifar10", batch_size=batch, data=data, channels=NARROW), T)
    shapes = [tuple(v.shape) for v in tr.graph.x]
    assert shapes == R.shapes(NARROW)
    ref = R.Vgg16(data["images"], data["labels"], NARROW)
    tr.reset()
    for v, a in zip(tr.graph.x, _weights(NARROW, "sample", seed=54)):
        v.load(a)
    snap = tr.snapshot()
    got = tr.train_step()
    assert tr.graph.last_path == "steps"
    idx = eng.to_numpy(tr.graph._mlp_idx[0])
    assert idx.shape == (T + 1, batch)
    fg = ref.flat_fg(shapes, idx)
    want, _ = tr.reference(fg, snap)
    g32, _ = tr.reference(fg, snap, np.float32)
    errs, errs32 = block_errors(got, want), block_errors(g32, want)
    for blk, e in errs.items():
        print("meta-gradient", blk, "err %.3e float32 oracle %.3e" % (e, errs32[blk]))
        assert e < max(GRAD_TOL, 3 * errs32[blk]), (blk, e, errs32[blk])


# ------------------------------------------------------------------------------------------------------------------
# 6. the RNNProp evaluation driver with the shipped MLP-trained optimizer, pointed at the narrow net
# ------------------------------------------------------------------------------------------------------------------
def test_evaluate_rnnprop_driver():
    H.check_driver(NET, 256, 20, 600)
