"""The three conv optimizees (l2o_mnist_conv_fg, l2o_cifar_conv_fg, l2o_lenet_fg) where their own modules do not go: the
edges of the minibatch range the launchers accept (2 .. 1024), scratch and output discipline, pooling windows that tie
exactly, and the graph path at a minibatch other than 128.  References: the float64 torch nets of conv_reference.py and
lenet_reference.py.

Bounds (the project's, as test_lenet.py): the loss within 1e-5 relative; a gradient block within GRAD_TOL = 5e-4 of its
largest float64 entry, or 3 x the float32 torch reference's own distance from float64 where that is larger; a bias that feeds
a batch norm (exactly 0 in exact arithmetic) within max(1e-6, 3 x float32 torch autograd's own ratio) of its layer's
largest weight-gradient entry.  So that the 3 x term cannot hide a failure, every case asserts that the float32 reference
alone is within GRAD_TOL / 3 of float64 in every compared block (a condition on the inputs: the seeds below meet it), which
leaves GRAD_TOL as the bound; and that the bound can see one wrong sample: with the LAST minibatch row (the one a clamped or
dropped tail would get wrong) replaced by another image, some block of the float64 gradient moves by more than its bound.

Pooling ties: the kernels keep the first candidate of a window (strict >), as torch's max_pool2d does.  Sections 1, 2 and 4
use noisy images and assert that no window ties; section 3 gives the images exact constant borders, so that windows whose
four patches are identical tie exactly in float32 and float64 alike, and asserts that the tied windows are the same set in
both precisions: then every weight gradient is independent of the candidate chosen and float64 torch stays a valid reference.

Measured on one MI355X, per net the worst over its 16 evaluation cases of sections 1 and 3 (the case in brackets; a block's
error as a fraction of GRAD_TOL; a batch-norm-fed bias as a fraction of its layer's largest weight-gradient entry, float32
torch autograd's own ratio on the same inputs after the slash).  Nothing failed and no kernel was changed.
    mnist_conv  block 0.0071 (batch_normalization/gamma, 3-bn), loss 4.9e-7 (257-bn), conv_layer1/biases1 1.9e-7 / 1.3e-6
                (2-bn-tied), conv_layer2/biases1 3.1e-7 / 2.2e-7 (257-bn)
    cifar_conv  block 0.0057 (conv_layer1/weights1, 16-bn-tied), loss 9.7e-7 (1024-nobn), conv_layer1/biases1 1.01e-6 / 3.8e-6
                (1023-bn: past the 1e-6 that minibatches 128 and 37 keep, inside 3 x float32 torch's), conv_layer2/biases1
                4.6e-7 / 2.2e-7 (1023-bn)
    lenet       block 0.18 (mlp/batch_norm/beta, 2-bn-tied: err 9.0e-5, float32 torch 1.6e-5; a batch norm over 2 samples),
                loss 1.9e-6 (2-bn), conv_2d_0/b 1.0e-6 / 2.3e-6 (65-bn), conv_2d_1/b 7.4e-7 / 2.2e-6 (1024-bn), linear_0/b
                3.9e-8 / 5.7e-7 (65-bn), linear_1/b 1.2e-7 / 2.5e-7 (65-bn)
At minibatch 257 and above the worst blocks were at 0.13 and 0.11 of GRAD_TOL (lenet, 1023-nobn, conv_2d_0/w and conv_2d_1/w:
err 6.345e-5 and 5.657e-5 where float32 torch has 6.333e-5 and 5.657e-5: a rounding that both float32 evaluations share),
every other one under 0.02.
The unrolls of section 4: fx within 2.8e-7 relative, x within 2.7e-5 of each variable's largest entry (cifar_conv, minibatch
257, batch_normalization/beta; bound 5e-4).  One wrong sample moves some block by 1.3e-3 of its largest entry or more in
every case (cifar_conv, minibatch 1023, no batch norm; O(1) at minibatch 2 and 3)."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

import imagenet_harness as H
import lenet_reference
import oracle as O
from helpers import make_params
from imagenet_harness import eng  # noqa: F401  (the fixture)
from open_l2o_amd import meta
from open_l2o_amd.session import Session
from test_meta_api import _net_config
from test_training_gradient import GRAD_TOL

pytestmark = pytest.mark.gpu

EDGE_BATCHES = [2, 3, 65, 257, 1023, 1024]
SCRATCH_BATCHES = [2, 257, 1024]
GUARD = 4096


def _edge(name, **own):
    return types.SimpleNamespace(**vars(H.NETS[name]), **own)


# imagenet_harness.NETS' entries of the three nets, plus what only these cases need: weights, whether the logits pass through
# a ReLU, the width of section 3's constant border
NETS = {
    "mnist_conv": _edge("mnist_conv", relu_logits=True, border=7,
                        weights=lambda bn, seed: H.NETS["mnist_conv"].R.sample_weights(bn, seed=seed, logit_scale=3.0)),
    "cifar_conv": _edge("cifar_conv", relu_logits=True, border=8,
                        weights=lambda bn, seed: H.NETS["cifar_conv"].R.sample_weights(bn, seed=seed, logit_scale=3.0)),
    "lenet": _edge("lenet", relu_logits=False, border=8,
                   weights=lambda bn, seed: lenet_reference.sample_weights(bn, seed=seed)),
}

# seeds of (weights, minibatch rows) per (net, batch norm, minibatch); where none is listed: the minibatch size itself.
# Chosen on the CPU so that the float32 reference alone is within GRAD_TOL / 3 of float64 (asserted in every case).
SEEDS = {("mnist_conv", True, 1023): 6, ("mnist_conv", True, 1024): 1, ("lenet", True, 2): 11, ("lenet", True, 1023): 1,
         ("lenet", False, 1023): 1}
TIE_SEEDS = {("lenet", True, 2): 4}


@functools.lru_cache(maxsize=None)
def _images(name, n, tied):
    """The data of one case: noisy synthetic images; ``tied``: with an exact constant border (0.0 for the MNIST net, one
    constant per image and channel for the CIFAR nets, one of 1, 1/2, 1/4, 1/8), as real images have."""
    net = NETS[name]
    d = net.data(n, seed=n + (7 if tied else 0))
    if not tied:
        return d
    img, b = d["images"].copy(), net.border
    side = img.shape[1]
    edge = np.zeros((side, side), bool)
    edge[:b] = edge[-b:] = edge[:, :b] = edge[:, -b:] = True
    # the CIFAR nets' constants are powers of two: every product with a float32 weight is exact and a float64 sum of them
    # is too, so the float64 reference ties on identical patches whatever order its GEMM adds them in at each position
    const = np.zeros((n, 1, 1, img.shape[3]), np.float32) if name == "mnist_conv" else \
        (2.0 ** -np.random.default_rng(n + 2000).integers(0, 4, (n, 1, 1, img.shape[3]))).astype(np.float32)
    img = np.where(edge[None, :, :, None], const, img).astype(np.float32)
    return {"images": img, "labels": d["labels"]}


def _own(g32, g64):
    """float32 torch's own distance from float64, of the block's largest float64 entry."""
    return float(np.abs(g32.astype(np.float64) - g64).max()) / float(np.abs(g64).max())


@functools.lru_cache(maxsize=None)
def _case(name, batch, batch_norm, tied=False):
    """Inputs and references of one case, computed once and shared (nothing modifies them): float64 and float32 torch, the
    tie masks of both runs, and the float64 gradient with the last minibatch row replaced by another image."""
    net = NETS[name]
    n = (32 if tied else 96) if batch <= 65 else 2048
    d = _images(name, n, tied)
    seed = (TIE_SEEDS if tied else SEEDS).get((name, batch_norm, batch), batch)
    ref = net.ref(d["images"], d["labels"], batch_norm)
    w = net.weights(batch_norm, seed)
    rows = np.random.default_rng(seed).integers(0, n, batch)
    rows[0], rows[-1] = n - 1, 0                                 # both ends of the data array are gathered
    c = types.SimpleNamespace(name=name, net=net, batch=batch, batch_norm=batch_norm, tied=tied, n=n, data=d, ref=ref, w=w,
                              rows=rows, names=net.R.names(batch_norm), fed=dict(net.fed(batch_norm)))
    c.f64, c.g64 = ref.fg([a.astype(np.float64) for a in w], rows)
    c.ties64 = [lenet_reference.pool_tie_mask(m) for m in ref.last_pre_pool]
    c.sigmoid_ties64 = lenet_reference.pool_ties(ref.last_pool_inputs) if name == "lenet" else 0
    c.logits64 = ref.last_logits.copy()
    c.f32, c.g32 = ref.fg(w, rows)
    c.ties32 = [lenet_reference.pool_tie_mask(m) for m in ref.last_pre_pool]
    c.own = {k: _own(c.g32[k], c.g64[k]) for k in range(len(w)) if k not in c.fed}
    other = rows.copy()
    other[-1] = n // 2
    assert not np.array_equal(ref.images[0], ref.images[n // 2])
    _, g_other = ref.fg([a.astype(np.float64) for a in w], other)
    c.moved = {k: float(np.abs(g_other[k] - c.g64[k]).max()) / float(np.abs(c.g64[k]).max()) for k in c.own}
    return c


def _id(c):
    return "%s-b%d-%s%s" % (c.name, c.batch, "bn" if c.batch_norm else "nobn", "-tied" if c.tied else "")


def check_inputs(c):
    """The conditions on the inputs, on the references alone (no GPU): every one an assertion."""
    nties64, nties32 = [int(m.sum()) for m in c.ties64], [int(m.sum()) for m in c.ties32]
    print("INPUT", _id(c), "tied windows per pooling layer: float64", nties64, "float32", nties32,
          "worst own %.3e worst moved %.3e" % (max(c.own.values()), max(c.moved.values())))
    if c.tied:
        # ties of structure, not of rounding: some in the first pooling layer, and the same windows in both precisions
        assert nties64[0] > 0 and nties32[0] > 0, (nties64, nties32)
        for m64, m32 in zip(c.ties64, c.ties32):
            assert np.array_equal(m64, m32), (nties64, nties32)
    else:
        assert sum(nties64) == 0 and sum(nties32) == 0 and c.sigmoid_ties64 == 0, (nties64, nties32, c.sigmoid_ties64)
    if c.net.relu_logits:
        assert (c.logits64 > 0).any() and (c.logits64 < 0).any()          # both sides of the ReLU on the logits
    for k, own in c.own.items():
        assert own <= GRAD_TOL / 3, (c.names[k], own)
    # the bound in use (GRAD_TOL, by the cap just asserted) sees one wrong sample
    assert any(c.moved[k] > max(GRAD_TOL, 3 * c.own[k]) for k in c.own), c.moved


class Device(object):
    """One case's inputs on the device; fg() is one evaluation into fresh outputs, returned as host arrays."""

    def __init__(self, eng, c):
        self.eng, self.c = eng, c
        self.desc = c.net.desc(c.batch, c.batch_norm, eng.tensor(c.ref.images), eng.int_tensor(c.data["labels"]))
        self.idx = eng.int_tensor(c.rows)
        self.ws = [eng.tensor(a) for a in c.w]

    def scratch_floats(self):
        s = self.c.net.struct()
        s.batch, s.n_data, s.batch_norm, s.flags = self.c.batch, int(self.desc.images.shape[0]), int(self.c.batch_norm), 0
        s.images, s.labels = self.desc.images.data_ptr(), self.desc.labels.data_ptr()
        return int(getattr(self.eng.lib, self.c.net.floats)(C.byref(s)))

    def fg(self, want_grad=True, fill=0.0):
        e = self.eng
        grads = [torch.full(a.shape, fill, dtype=torch.float32, device=e.device) for a in self.c.w] if want_grad else None
        loss = torch.full((1,), fill, dtype=torch.float32, device=e.device)
        getattr(e, self.c.net.fg)(self.desc, self.idx, self.ws, loss, grads)
        return e.to_numpy(loss), None if grads is None else [e.to_numpy(g) for g in grads]


_PLAIN = {}


def plain(eng, c):
    """The case's result through the engine's own scratch and zero-filled outputs: computed once (section 1), compared bit
    for bit by section 2."""
    key = (c.name, c.batch, c.batch_norm, c.tied)
    if key not in _PLAIN:
        _PLAIN[key] = Device(eng, c).fg()
    return _PLAIN[key]


def compare(c, loss, grads):
    """Every figure printed, then the project's bounds."""
    got_f = float(loss[0])
    rel, rel32 = abs(got_f - c.f64) / abs(c.f64), abs(float(c.f32) - c.f64) / abs(c.f64)
    print("FIG", _id(c), "loss", got_f, c.f64, "rel %.3e (float32 torch %.3e)" % (rel, rel32))
    failures = []
    if not rel <= 1e-5:
        failures.append(("loss", got_f, c.f64))
    for k, nm in enumerate(c.names):
        got, want = grads[k].astype(np.float64).reshape(c.g64[k].shape), c.g64[k]
        if k in c.fed:
            wscale = float(np.abs(c.g64[c.fed[k]]).max())
            ratio, r32 = float(np.abs(got).max()) / wscale, float(np.abs(c.g32[k]).max()) / wscale
            print("FIG", _id(c), "%-32s |g| / max|dW| %.3e (float32 torch %.3e)" % (nm, ratio, r32))
            if not ratio <= max(1e-6, 3 * r32):
                failures.append((nm, ratio, r32))
            continue
        scale = float(np.abs(want).max())
        err, own = float(np.abs(got - want).max()) / scale, c.own[k]
        print("FIG", _id(c), "%-32s err %.3e bound %.3e (float32 torch %.3e) of max %.3e, of GRAD_TOL %.4f" %
              (nm, err, max(GRAD_TOL, 3 * own), own, scale, err / GRAD_TOL))
        if not err <= max(GRAD_TOL, 3 * own):
            failures.append((nm, err, own))
    assert not failures, failures


def check_tail(eng, c, loss, grads):
    """test_fg_vs_float64's tail: a second call is bit-identical; forward only gives the same loss bits."""
    dev = Device(eng, c)
    loss2, grads2 = dev.fg()
    loss3, _ = dev.fg(want_grad=False)
    assert loss2.tobytes() == loss.tobytes() and loss3.tobytes() == loss.tobytes()
    for a, b in zip(grads, grads2):
        assert a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------------------------
# 1. one evaluation against float64 at the edges of the minibatch range
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch_norm", [True, False])
@pytest.mark.parametrize("batch", EDGE_BATCHES)
@pytest.mark.parametrize("name", list(NETS))
def test_fg_edge_batches(eng, name, batch, batch_norm):
    """2: the minimum; 3: odd, below every lane count of the cv_* reductions; 65: one past LeNet's 64 sample lanes; 257:
    one past the first 256-sample pass of ln_fc_body (clamped rows live); 1023: tails at full size; 1024: the maximum (full
    LDS tiles, 128-sample dW2 chunks)."""
    c = _case(name, batch, batch_norm)
    check_inputs(c)
    loss, grads = plain(eng, c)
    compare(c, loss, grads)
    check_tail(eng, c, loss, grads)


# ------------------------------------------------------------------------------------------------------------------
# 2. scratch and output discipline
# ------------------------------------------------------------------------------------------------------------------
def poisoned(eng, c, floats=None):
    """A NaN-filled scratch buffer of the size the library asks for (or ``floats``, for a later smaller call) plus a guard of
    GUARD finite floats, installed as the engine's cached scratch (which the engine reuses when it is large enough)."""
    n = Device(eng, c).scratch_floats() if floats is None else floats
    assert n > 0
    buf = torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device=eng.device)
    guard = torch.arange(GUARD, dtype=torch.float32, device=eng.device) * 0.5 + 1.0
    buf[n:] = guard
    assert buf.data_ptr() % 16 == 0                              # l2o_lenet_fg wants 16-byte alignment
    setattr(eng, c.net.scratch, buf)
    return buf, n, eng.to_numpy(guard)


def run_on(eng, c, buf):
    """One evaluation of ``c`` with NaN-filled outputs on the installed scratch ``buf``: every output finite."""
    loss, grads = Device(eng, c).fg(fill=float("nan"))
    assert getattr(eng, c.net.scratch) is buf                    # the engine did use the buffer under test
    assert np.isfinite(loss).all(), loss
    for nm, g in zip(c.names, grads):
        assert np.isfinite(g).all(), (nm, int((~np.isfinite(g)).sum()))
    return loss, grads


@pytest.mark.parametrize("batch", SCRATCH_BATCHES)
@pytest.mark.parametrize("name", list(NETS))
def test_poisoned_scratch(eng, name, batch):
    """Nothing reads scratch it did not write (a NaN would reach an output or change its bits), every output entry is
    written, nothing is written past the size l2o_*_scratch_floats reports."""
    c = _case(name, batch, True)
    want_loss, want_grads = plain(eng, c)
    buf, n, guard = poisoned(eng, c)
    loss, grads = run_on(eng, c, buf)
    assert loss.tobytes() == want_loss.tobytes()
    for nm, a, b in zip(c.names, grads, want_grads):
        assert a.tobytes() == b.tobytes(), nm
    assert eng.to_numpy(buf[n:]).tobytes() == guard.tobytes()


@pytest.mark.parametrize("name", list(NETS))
def test_stale_scratch(eng, name):
    """Minibatch 1024, then minibatch 2 on the same scratch, not poisoned again: nothing beyond the 2 samples leaks in from
    the earlier, larger call (the engine reuses one cached scratch across minibatch sizes)."""
    small, large = _case(name, 2, True), _case(name, 1024, True)
    buf, _, _ = poisoned(eng, small)
    want_loss, want_grads = run_on(eng, small, buf)
    buf, n, guard = poisoned(eng, large)
    run_on(eng, large, buf)
    loss, grads = run_on(eng, small, buf)
    assert loss.tobytes() == want_loss.tobytes()
    for nm, a, b in zip(small.names, grads, want_grads):
        assert a.tobytes() == b.tobytes(), nm
    assert eng.to_numpy(buf[n:]).tobytes() == guard.tobytes()


# ------------------------------------------------------------------------------------------------------------------
# 3. pooling windows that tie exactly
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch_norm", [True, False])
@pytest.mark.parametrize("batch", [2, 16])
@pytest.mark.parametrize("name", list(NETS))
def test_tied_pool_windows(eng, name, batch, batch_norm):
    """Images with an exact constant border: the windows over it tie exactly; the gradient goes to the first candidate, once
    (to all of them, or to none, and dW of the first conv layer is off by O(1))."""
    c = _case(name, batch, batch_norm, tied=True)
    check_inputs(c)
    loss, grads = plain(eng, c)
    compare(c, loss, grads)
    check_tail(eng, c, loss, grads)


# ------------------------------------------------------------------------------------------------------------------
# 4. the graph path at an edge minibatch
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [2, 257])
@pytest.mark.parametrize("name", list(NETS))
def test_unroll_edge_batches(eng, name, batch):
    """test_unroll_vs_float64 of the three nets' own modules (meta_loss on the steps path against a float64 host unroll, the
    same bounds for fx and x), L2O-DM log-sign, T = 3: the graph's own index and scratch plumbing at a minibatch other than
    128."""
    net = NETS[name]
    T, n = 3, 512
    data = net.data(n, seed=41)
    idx = np.random.default_rng(42 + batch).integers(0, n, size=(T + 1, batch))
    cfg = O.DM_LOGSIGN
    params = make_params(cfg, seed=43, trained_like=True)
    meta.set_random_seed(44)
    problem = net.problem(batch_size=batch, data=data, sampler=lambda ne, b, nd: idx[:ne])
    optimizer = meta.MetaOptimizer(**_net_config(cfg, params))
    ml = optimizer.meta_loss(problem, T)
    with Session() as sess:
        sess.run(ml.reset)
        v0 = [v.eval() for v in optimizer.graph.x]
        res = optimizer.graph.execute({}, True)
    assert optimizer.graph.last_path == "steps"
    fx = np.asarray(res["fx_array"], np.float64)
    xT = [np.asarray(a, np.float64) for a in res["x"]]
    ref = net.ref(data["images"], data["labels"], True)
    outs = {}
    for dt in (np.float64, np.float32):
        p = {m: {v: a.astype(dt) for v, a in d.items()} for m, d in params.items()}
        states = [tuple((h.astype(dt), c.astype(dt)) for h, c in O.net_initial_state(cfg, a.size)) for a in v0]
        fx_r, x_r, _ = O.unroll_multi(lambda vs, t, wg: ref.fg(vs, idx[t], wg), cfg, p, [a.astype(dt) for a in v0],
                                      states, T)
        outs[dt] = (np.asarray(fx_r, np.float64), [np.asarray(a, np.float64) for a in x_r])
    (fx64, x64), (fx32, x32) = outs[np.float64], outs[np.float32]
    assert fx.shape == fx64.shape == (T + 1,)
    tag = "%s-b%d-unroll" % (name, batch)
    for t in range(T + 1):
        print("FIG", tag, "fx", t, fx[t], fx64[t], fx32[t], "rel %.3e" % (abs(fx[t] - fx64[t]) / abs(fx64[t])))
        assert abs(fx[t] - fx64[t]) <= max(1e-5 * abs(fx64[t]), 3 * abs(fx32[t] - fx64[t])), (t, fx[t], fx64[t], fx32[t])
    for k, (g, w64, w32) in enumerate(zip(xT, x64, x32)):
        scale = float(np.abs(w64).max())
        err = float(np.abs(g.reshape(w64.shape) - w64).max())
        bound = max(GRAD_TOL * scale, 3 * float(np.abs(w32 - w64).max()))
        print("FIG", tag, "x %-32s err %.3e bound %.3e of max %.3e" % (net.R.names(True)[k], err, bound, scale))
        assert err <= bound, (net.R.names(True)[k], err, bound)
