"""problems.NAS on the MI355X: l2o_nas_fg (csrc/l2o_nas.h) against the float64 torch reference (nas_reference.py) with and
without batch norm at minibatches 2, 3, 37, 128 and 1024 and on images that are zero inside their outermost ring; the bit
contracts of the entry point; a 20-step unroll on the graph's step path against a float64 host unroll; two consecutive
first-order meta-gradients; and the RNNProp evaluation driver.

Bounds (the project's): the loss within 1e-5 relative; a gradient block within GRAD_TOL (5e-4) of its largest float64 entry,
or 3 x the float32 reference's own distance where that is larger.  A conv bias under batch norm has a float64 gradient of
about 1e-17 (0 in exact arithmetic), so those blocks are held to max(1e-6 wscale, 3 x the float32 reference's largest entry
there), wscale the largest entry of the layer's weight gradient (1e-6 wscale: test_cifar_conv.py's bound).

ReLU masks are decisions.  Under batch norm a weight gradient is a sum over B * 1024 positions of terms that cancel down to
about sqrt(B * 1024) of them (the gradient w.r.t. z sums to 0 over a channel), so ONE mask that float32 rounding flips
moves a block by about 1 / sqrt(B * 1024) of its largest entry -- 2.8e-3 at minibatch 128 -- and float32 torch itself is
then 5e-4 ... 8e-3 away from float64 (seen at minibatch 128 with 3 flipped masks of 2 M in node1_onto_node3: 7.6e-3).  A
parity case means something only on inputs that float32 itself gets right.  The minibatch of every parity case is drawn from
default_rng(1000 * seed + batch) with the seed in MINIBATCH_SEED.  With batch norm the seed is the one, of the first 120 (24
at minibatch 1024), whose float64 batch-norm outputs keep the largest distance from 0 in units of a float32 sum's rounding
(nas_reference._margin) among those for which the float32 reference is within GRAD_TOL / 3 of float64 on every block and
within 1e-5 / 3 on the loss -- at 1, 4 and 8 threads and with every weight moved by one ulp at random; without batch norm
(no cancellation: a flipped mask is 1 / (B * 1024) of a block) it is the first seed with that property.  Every case asserts
the float32 condition before the kernel's result is looked at, so the bound in force is GRAD_TOL."""
import ctypes as C

import numpy as np
import pytest

import imagenet_harness as H
import nas_reference as R
from imagenet_harness import eng  # noqa: F401  (the fixture)
from open_l2o_amd import _abi, _engine
from test_training_gradient import GRAD_TOL

pytestmark = pytest.mark.gpu

NET = H.NETS["nas"]
N_DATA = 64
_cache = {}
# (batch norm, weight scale, minibatch, data) -> the seed of the minibatch
MINIBATCH_SEED = {
    (True, "sample", 2, "uniform"): 10, (True, "sample", 3, "uniform"): 97, (True, "sample", 37, "uniform"): 7,
    (True, "sample", 128, "uniform"): 40, (True, "init", 2, "uniform"): 33, (True, "init", 3, "uniform"): 2,
    (True, "init", 37, "uniform"): 79, (True, "init", 128, "uniform"): 10,
    (False, "sample", 2, "uniform"): 1, (False, "sample", 3, "uniform"): 1, (False, "sample", 37, "uniform"): 1,
    (False, "sample", 128, "uniform"): 1, (False, "init", 2, "uniform"): 1, (False, "init", 3, "uniform"): 1,
    (False, "init", 37, "uniform"): 1, (False, "init", 128, "uniform"): 1,
    (True, "sample", 3, "ring"): 44, (True, "sample", 1024, "uniform"): 20,
}


def _data(kind="uniform"):
    """Uniform images and labels; "ring": the same images, zero except for the outermost ring of pixels."""
    if kind not in _cache:
        d = H.uniform_cifar(N_DATA, 0)
        images = d["images"].copy()
        if kind == "ring":
            images[:, 1:31, 1:31, :] = 0.0
        _cache[kind] = {"images": images, "labels": d["labels"]}
    return _cache[kind]


def _weights(batch_norm, scale, seed=1):
    return (R.sample_weights if scale == "sample" else R.init_weights)(batch_norm, seed)


def _reference(batch_norm, scale, batch, kind):
    """(rows, float64 loss, float64 gradients, float32 loss, float32 gradients): computed once per case and shared."""
    key = ("ref", batch_norm, scale, batch, kind)
    if key not in _cache:
        data = _data(kind)
        net = R.Nas(data["images"], data["labels"], batch_norm)
        w = _weights(batch_norm, scale)
        rows = np.random.default_rng(1000 * MINIBATCH_SEED[batch_norm, scale, batch, kind] + batch).integers(0, N_DATA, batch)
        f64, g64 = net.fg([a.astype(np.float64) for a in w], rows)
        print("decision margins per layer (units of a float32 sum's rounding):", ["%.2f" % m for m in net.last_margins])
        f32, g32 = net.fg(w, rows)
        _cache[key] = (rows, float(f64), g64, float(f32), g32)
    return _cache[key]


def _desc(eng, batch_norm, batch, kind="uniform"):
    data = _data(kind)
    return _engine.NasDesc(batch, batch_norm, eng.tensor(data["images"].reshape(N_DATA, -1)), eng.int_tensor(data["labels"]))


def _run_fg(eng, d, rows, w, **kw):
    return H.run_fg(eng, NET, d, rows, w, **kw)


def _check_fg(eng, batch_norm, scale, batch, kind="uniform"):
    rows, f64, g64, f32, g32 = _reference(batch_norm, scale, batch, kind)
    names = R.names(batch_norm)
    # the conditions on the inputs, before the kernels run
    own_f = abs(f32 - f64)
    assert own_f <= 1e-5 / 3 * abs(f64), (f32, f64)
    for k, nm in enumerate(names):
        if batch_norm and nm.endswith("biases1"):
            wscale = float(np.abs(g64[k - 1]).max())
            own = float(np.abs(g32[k]).max())
            print("float32 reference %-28s largest entry %.3e of wscale (float64: %.1e)" %
                  (nm, own / wscale, float(np.abs(g64[k]).max()) / wscale))
            assert own <= GRAD_TOL / 3 * wscale, (nm, own, wscale)
        else:
            scale64 = float(np.abs(g64[k]).max())
            assert scale64 > 1e-30, nm
            assert float(np.abs(g32[k] - g64[k]).max()) <= GRAD_TOL / 3 * scale64, nm
    w = _weights(batch_norm, scale)
    loss, grads = _run_fg(eng, _desc(eng, batch_norm, batch, kind), rows, w, fill=float("nan"))
    got_f = float(loss[0])
    print("loss", got_f, f64, "rel %.3e (float32 torch %.3e)" % (abs(got_f - f64) / abs(f64), own_f / abs(f64)))
    failures = []
    if not abs(got_f - f64) <= 1e-5 * abs(f64):
        failures.append(("loss", got_f, f64))
    for k, (nm, g, want, w32) in enumerate(zip(names, grads, g64, g32)):
        g = g.astype(np.float64).reshape(want.shape)
        if not np.isfinite(g).all():
            failures.append((nm, "not finite"))
            continue
        if batch_norm and nm.endswith("biases1"):
            wscale = float(np.abs(g64[k - 1]).max())
            got, own = float(np.abs(g).max()), float(np.abs(w32).max())
            print("%-28s largest entry %.3e of wscale (float32 torch %.3e)" % (nm, got / wscale, own / wscale))
            if not got <= max(1e-6 * wscale, 3 * own):
                failures.append((nm, got / wscale, own / wscale))
            continue
        scale64 = float(np.abs(want).max())
        err, bnd = H.bound(g, want, w32)
        print("%-28s err %.3e bound %.3e of max %.3e" % (nm, err / scale64, bnd / scale64, scale64))
        if not err <= bnd:
            failures.append((nm, err / scale64, bnd / scale64))
    assert not failures, failures


# ------------------------------------------------------------------------------------------------------------------
# 1. one evaluation: l2o_nas_fg against float64
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", ["sample", "init"])
@pytest.mark.parametrize("batch_norm", [True, False])
@pytest.mark.parametrize("batch", [2, 3, 37, 128])
def test_fg_vs_float64(eng, batch, batch_norm, scale):
    """Minibatch 2 and 3: fewer strips than weight-gradient workgroups allow (8 and 12); 37: 148 strips, an odd count of
    samples in every merge; 128: 512 strips on 256 workgroups, two each."""
    _check_fg(eng, batch_norm, scale, batch)


def test_fg_minibatch_1024(eng):
    """The largest minibatch, with batch norm: 2^20 pixels, 4096 strips, 16 per weight-gradient workgroup."""
    _check_fg(eng, True, "sample", 1024)


def test_fg_border_ring(eng):
    """Images that are zero except for their outermost ring of pixels, minibatch 3: a padding or pool-divisor mistake is
    not diluted by the 900 interior positions."""
    _check_fg(eng, True, "sample", 3, kind="ring")


# ------------------------------------------------------------------------------------------------------------------
# 2. the bit contracts of the entry point
# ------------------------------------------------------------------------------------------------------------------
def _struct(batch, batch_norm, images, labels, n_data=N_DATA, flags=0):
    c = _abi.Nas()
    c.batch, c.n_data, c.batch_norm, c.flags = batch, n_data, batch_norm, flags
    c.images, c.labels = C.c_void_p(images.data_ptr()), C.c_void_p(labels.data_ptr())
    return c


def _raw_call(eng, c, rows, w, scratch, want_grad=True):
    """l2o_nas_fg through the binding with a scratch buffer of the test's own: (return code, loss, gradients)."""
    idx = eng.int_tensor(rows)
    ws = [eng.tensor(a) for a in w]
    grads = [eng.zeros(*a.shape) for a in w] if want_grad else None
    loss = eng.zeros(1)
    rc = eng.lib.l2o_nas_fg(C.byref(c), C.c_void_p(idx.data_ptr()), _engine._ptr_array(ws), _engine._ptr(loss),
                            _engine._ptr_array(grads), _engine._ptr(scratch), eng._stream())
    return rc, eng.to_numpy(loss).copy(), None if grads is None else [eng.to_numpy(g).copy() for g in grads]


@pytest.mark.parametrize("batch_norm", [True, False])
def test_bit_contracts(eng, batch_norm):
    import torch
    w = _weights(batch_norm, "sample")
    rows = np.random.default_rng(5).integers(0, N_DATA, 37)
    d = _desc(eng, batch_norm, 37)
    loss_a, grads_a = _run_fg(eng, d, rows, w)
    loss_b, grads_b = _run_fg(eng, d, rows, w, fill=float("nan"))
    loss_f, _ = _run_fg(eng, d, rows, w, want_grad=False)
    assert loss_a.tobytes() == loss_b.tobytes() == loss_f.tobytes() and np.isfinite(loss_a).all()
    for a, b in zip(grads_a, grads_b):
        assert np.isfinite(a).all() and a.tobytes() == b.tobytes()
    # a NaN-filled scratch of exactly scratch_floats: the same bits, and the guard behind it untouched
    data = _data()
    images, labels = eng.tensor(data["images"].reshape(N_DATA, -1)), eng.int_tensor(data["labels"])
    c = _struct(37, int(batch_norm), images, labels)
    n = int(eng.lib.l2o_nas_scratch_floats(C.byref(c)))
    guard = 4096
    buf = torch.full((n + guard,), float("nan"), dtype=torch.float32, device=eng.device)
    buf[n:] = 12345.0
    rc, loss_n, grads_n = _raw_call(eng, c, rows, w, buf)
    assert rc == 0 and loss_n.tobytes() == loss_a.tobytes()
    for a, b in zip(grads_a, grads_n):
        assert a.tobytes() == b.tobytes()
    assert bool((buf[n:] == 12345.0).all())
    buf[:n] = float("nan")
    rc, loss_nf, _ = _raw_call(eng, c, rows, w, buf, want_grad=False)
    assert rc == 0 and loss_nf.tobytes() == loss_a.tobytes() and bool((buf[n:] == 12345.0).all())
    # an index outside the data set is clamped into it
    out = rows.copy()
    out[0], out[5] = -7, N_DATA + 1000
    clamped = rows.copy()
    clamped[0], clamped[5] = 0, N_DATA - 1
    loss_o, grads_o = _run_fg(eng, d, out, w)
    loss_c, grads_c = _run_fg(eng, d, clamped, w)
    assert loss_o.tobytes() == loss_c.tobytes()
    for a, b in zip(grads_o, grads_c):
        assert a.tobytes() == b.tobytes()
    # unsupported descriptors: the error code, and nothing is launched (the loss and the scratch keep their contents)
    buf.fill_(777.0)
    for batch, bn, flags in ((1, 1, 0), (1025, 1, 0), (37, 2, 0), (37, int(batch_norm), 1)):
        cc = _struct(batch, bn, images, labels, flags=flags)
        assert int(eng.lib.l2o_nas_scratch_floats(C.byref(cc))) == 0
        rc, loss_u, _ = _raw_call(eng, cc, rows, w, buf, want_grad=False)
        assert rc == _abi.L2O_ERR_UNSUPPORTED and loss_u[0] == 0.0
    assert bool((buf == 777.0).all())
    with pytest.raises(_abi.L2OUnsupported):
        eng.nas_fg(_engine.NasDesc(1, batch_norm, images, labels), eng.int_tensor(rows[:1]), [eng.tensor(a) for a in w],
                   eng.zeros(1), None)
    with pytest.raises(ValueError):
        eng.nas_fg(d, eng.int_tensor(rows), [eng.tensor(a) for a in w][:-1], eng.zeros(1), None)


# ------------------------------------------------------------------------------------------------------------------
# 3. the unroll: meta_loss over the cell, T = 20, against a float64 host unroll
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", ["dm_logsign", "rnnprop"])
def test_unroll_vs_float64(eng, net):
    T, batch = 20, 8
    idx = np.random.default_rng(42).integers(0, N_DATA, size=(T + 1, batch))
    H.check_unroll_vs_float64(eng, NET, net, T, batch, _data(), idx)


# ------------------------------------------------------------------------------------------------------------------
# 4. the meta-gradient: two consecutive train steps against helpers.oracle_meta_grad
# ------------------------------------------------------------------------------------------------------------------
def test_meta_gradient_vs_float64(eng):
    """As test_cifar_conv.py: the carry of the conv biases under batch norm is not compared (their gradient is 0 in exact
    arithmetic, so what a float32 implementation feeds the optimizer for them is its own rounding noise)."""
    H.check_meta_gradient_vs_float64(eng, NET, "dm_logsign", 5, 8, _data())


# ------------------------------------------------------------------------------------------------------------------
# 5. the RNNProp evaluation driver with the shipped MLP-trained optimizer, pointed at the NAS cell
# ------------------------------------------------------------------------------------------------------------------
def test_evaluate_rnnprop_driver():
    H.check_driver(NET, 256, 20, 600)
