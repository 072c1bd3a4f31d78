"""The Python host layer of the step-path optimizees (problems.mnist with several hidden layers, mnist_conv, cifar10, LeNet,
confocal_microscopy_3d, vgg16_cifar10, NAS) is one table, _engine.STEP_OPTIMIZEES, and what reads it.  Pinned here, as
literals: every kind's entry and the predicates that read the table, the kinds' symbols and structs in the binding (the
whole of it against the headers: test_abi_headers_cpu.py), the public names and signatures that tests,
scripts and oracle engines use, and the texts of the refusals -- in the factories (no GPU) and in the engine (GPU)."""
import ctypes as C
import inspect

import numpy as np
import pytest

from open_l2o_amd import _abi, _engine, _graph_steps, problems
from open_l2o_amd._engine import STEP_OPTIMIZEES

# kind -> engine method, symbol stem, scratch attribute, draws a minibatch per evaluation
TABLE = {
    5: ("mlp_deep_fg", "l2o_mlp_deep", "_mlp_deep_scratch", True),
    6: ("mnist_conv_fg", "l2o_mnist_conv", "_mnist_conv_scratch", True),
    7: ("cifar_conv_fg", "l2o_cifar_conv", "_cifar_conv_scratch", True),
    8: ("lenet_fg", "l2o_lenet", "_lenet_scratch", True),
    9: ("confocal_fg", "l2o_confocal", "_confocal_scratch", False),
    10: ("vgg16_fg", "l2o_vgg16", "_vgg16_scratch", True),
    11: ("nas_fg", "l2o_nas", "_nas_scratch", True),
}
IMAGE_NETS = {
    "mnist_conv": (6, problems.synthetic_mnist, problems.mnist_conv, "28x28x1"),
    "cifar10": (7, problems.synthetic_cifar10, lambda **kw: problems.cifar10("cifar10", **kw), "32x32x3"),
    "LeNet": (8, problems.synthetic_cifar10,
              lambda **kw: problems.LeNet("cifar10", conv_channels=(6, 16), linear_layers=(120, 84), **kw), "32x32x3"),
}


def test_table_has_each_kind_once():
    """Membership, never equality, for the set of kinds: the kind after these changes no line here."""
    assert (_abi.PROB_MLP, _abi.PROB_MNIST_CONV, _abi.PROB_CIFAR_CONV, _abi.PROB_LENET, _abi.PROB_CONFOCAL, _abi.PROB_VGG16,
            _abi.PROB_NAS) == (5, 6, 7, 8, 9, 10, 11)
    assert set(range(5, 12)) <= set(STEP_OPTIMIZEES)
    assert {k: (e.method, e.stem, e.scratch, e.sampled) for k, e in STEP_OPTIMIZEES.items() if k in TABLE} == TABLE
    assert [STEP_OPTIMIZEES[k].desc for k in (5, 6, 7, 8, 9, 10, 11)] == [
        _engine.MlpDeepDesc, _engine.MnistConvDesc, _engine.CifarConvDesc, _engine.LenetDesc, _engine.ConfocalDesc,
        _engine.Vgg16Desc, _engine.NasDesc]
    assert [STEP_OPTIMIZEES[k].struct for k in (5, 6, 7, 8, 9, 10, 11)] == [
        _abi.MlpDeep, _abi.MnistConv, _abi.CifarConv, _abi.Lenet, _abi.Confocal, _abi.Vgg16, _abi.Nas]
    for k, e in STEP_OPTIMIZEES.items():
        assert type(e) is _engine.StepOptimizee and _engine.step_optimizee(k) is e
        assert (e.struct, e.stem) in _abi.STEP_FG and callable(getattr(_engine.HipEngine, e.method))
    for k in (0, 1, 2, 3, 4, 99):
        assert _engine.step_optimizee(k) is None


def test_variable_counts():
    for kind, with_bn, without in ((6, 10, 6), (7, 10, 6), (8, 14, 10)):
        e = STEP_OPTIMIZEES[kind]
        assert e.nvars(e.desc(2, True, None, None)) == with_bn and e.nvars(e.desc(2, False, None, None)) == without
    assert STEP_OPTIMIZEES[5].nvars(_engine.MlpDeepDesc(784, (20, 20), 10, 128, 0, None, None)) == 6
    assert STEP_OPTIMIZEES[5].nvars(_engine.MlpDeepDesc(784, (20, 20, 20), 10, 128, 0, None, None)) == 8
    assert STEP_OPTIMIZEES[9].nvars(_engine.ConfocalDesc(32, 5, (28, 28, 28))) == 31
    assert STEP_OPTIMIZEES[10].nvars(_engine.Vgg16Desc(2, (8, 8, 8, 8, 8), None, None)) == 28
    e = STEP_OPTIMIZEES[11]
    assert e.nvars(e.desc(2, True, None, None)) == 18 and e.nvars(e.desc(2, False, None, None)) == 10


def test_derived_kind_tuples():
    """What used to be tuples derived from the table are the two predicates the graph and meta.py ask."""
    kinds = tuple(range(12)) + (99,)
    assert tuple(k for k in kinds if _graph_steps.is_multivar(k)) == (5, 6, 7, 8, 9, 10, 11)
    assert tuple(k for k in kinds if _graph_steps.is_sampled(k)) == (5, 6, 7, 8, 10, 11)
    assert all(type(f(k)) is bool for f in (_graph_steps.is_multivar, _graph_steps.is_sampled) for k in kinds)


def test_symbols_are_declared():
    import __graft_entry__  # noqa: F401
    lib = _abi.lib()
    home = {k: _abi.PROTOTYPES["l2o_abi.h"] for k in (5, 6, 7, 8, 9)}         # (the header that declares the kind's two symbols)
    home.update({10: _abi.PROTOTYPES["l2o_vgg16_abi.h"], 11: _abi.PROTOTYPES["l2o_nas_abi.h"]})
    for k, e in STEP_OPTIMIZEES.items():
        floats, fg = e.stem + "_scratch_floats", e.stem + "_fg"
        assert k not in home or (floats in home[k] and fg in home[k])
        assert getattr(lib, floats).restype is C.c_size_t and getattr(lib, floats).argtypes == [C.POINTER(e.struct)]
        assert getattr(lib, fg).restype is C.c_int and getattr(lib, fg).argtypes == [C.POINTER(e.struct)] + [C.c_void_p] * 6


def test_image_net_structs():
    for S, doc in ((_abi.MnistConv, "struct l2o_mnist_conv"), (_abi.CifarConv, "struct l2o_cifar_conv"),
                   (_abi.Lenet, "struct l2o_lenet")):
        assert C.sizeof(S) == 32 and S.__doc__ == doc
        assert [n for n, _ in S._fields_] == ["batch", "n_data", "batch_norm", "flags", "images", "labels"]
        assert [t for _, t in S._fields_] == [C.c_int32] * 4 + [C.c_void_p] * 2
        s = S()
        s.batch, s.n_data, s.batch_norm, s.flags, s.images, s.labels = 2, 8, 1, 0, 16, 32
        assert (s.batch, s.n_data, s.batch_norm, s.flags, s.images, s.labels) == (2, 8, 1, 0, 16, 32)
    assert len({_abi.MnistConv, _abi.CifarConv, _abi.Lenet}) == 3


def test_public_names_and_signatures():
    for name, sig in (("mlp_deep_fg", "(self, d: 'MlpDeepDesc', indices, ws, loss, grads)"),
                      ("mnist_conv_fg", "(self, d: 'MnistConvDesc', indices, ws, loss, grads)"),
                      ("cifar_conv_fg", "(self, d: 'CifarConvDesc', indices, ws, loss, grads)"),
                      ("lenet_fg", "(self, d: 'LenetDesc', indices, ws, loss, grads)"),
                      ("confocal_fg", "(self, d: 'ConfocalDesc', theta, sim, loss, grads)")):
        assert str(inspect.signature(getattr(_engine.HipEngine, name))) == sig, name
    image_net = "(batch: 'int', batch_norm: 'bool', images: 'torch.Tensor', labels: 'torch.Tensor') -> None"
    for name, sig in (("MnistConvDesc", image_net), ("CifarConvDesc", image_net), ("LenetDesc", image_net),
                      ("MlpDeepDesc", "(n_in: 'int', hidden: 'tuple', n_out: 'int', batch: 'int', activation: 'int', "
                                      "images: 'torch.Tensor', labels: 'torch.Tensor') -> None"),
                      ("ConfocalDesc", "(batch: 'int', num_points: 'int', roi: 'tuple', img: 'torch.Tensor' = None) -> None")):
        assert str(inspect.signature(getattr(_engine, name))) == sig, name
    for cls in (_engine.MnistConvDesc, _engine.CifarConvDesc, _engine.LenetDesc):
        d = cls(4, True, "images", "labels")                     # positionally, as tests and scripts build them
        assert (d.batch, d.batch_norm, d.images, d.labels) == (4, True, "images", "labels") and type(d) is cls
        assert d == cls(4, True, "images", "labels") and d != cls(2, True, "images", "labels")
    assert _engine.MnistConvDesc(4, True, 0, 0) != _engine.CifarConvDesc(4, True, 0, 0)


@pytest.mark.parametrize("name", list(IMAGE_NETS))
def test_factory_refusals(name):
    kind, synthetic, factory, pixels = IMAGE_NETS[name]
    data = synthetic(8, seed=0)
    bad = {"images": np.zeros((8, 5, 5, 2), np.float32), "labels": data["labels"]}
    with pytest.raises(ValueError) as ei:
        factory(data=bad)
    assert str(ei.value) == "problems.%s takes %s images (got (8, 5, 5, 2))" % (name, pixels)
    for batch in (1, 1025):
        with pytest.raises(NotImplementedError) as ei:
            factory(data=data, batch_size=batch)
        assert str(ei.value) == "problems.%s is implemented for minibatches of 2 to 1024 (got %d)" % (name, batch)
    (term,) = factory(data=data, batch_size=2, batch_norm=0)().terms
    assert term.kind == kind and list(term.hyper) == ["images", "labels", "batch_size", "batch_norm", "sampler"]
    assert term.hyper["batch_norm"] is False and term.hyper["batch_size"] == 2 and term.hyper["sampler"] is None
    images = term.hyper["images"]
    assert images.dtype == np.float32 and images.flags["C_CONTIGUOUS"] and images.shape == (8, images.size // 8)
    assert term.hyper["labels"].dtype == np.int32


# -- the engine (GPU) --------------------------------------------------------------------------------------------------
@pytest.fixture
def eng():
    return _engine.HipEngine()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(IMAGE_NETS))
def test_engine_image_net_wiring(eng, name):
    """Minibatches 4, 2, 8 on 8 synthetic images: forward only gives the bits of the call with gradients, the scratch is
    kept while it is large enough and replaced by a larger one when not; then the two refusals, with their texts."""
    kind, synthetic, factory, _ = IMAGE_NETS[name]
    entry = STEP_OPTIMIZEES[kind]
    data = synthetic(8, seed=1)
    build = factory(data=data, batch_size=2)
    shapes = [v.shape for v in build().variables]
    term = build().terms[0]
    images, labels = eng.tensor(term.hyper["images"]), eng.int_tensor(term.hyper["labels"])
    rng = np.random.default_rng(2)
    ws = [eng.tensor(rng.normal(0, 0.1, sh)) for sh in shapes]
    fg = getattr(eng, entry.method)

    def run(batch):
        d = entry.desc(batch, True, images, labels)
        idx = eng.int_tensor(np.arange(batch)[::-1] % 8)
        loss, loss_f, grads = eng.zeros(1), eng.zeros(1), [eng.zeros(*sh) for sh in shapes]
        fg(d, idx, ws, loss, grads)
        fg(d, idx, ws, loss_f, None)
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
    for bn, n in ((True, len(ws) - 1), (False, len(ws))):
        with pytest.raises(ValueError) as ei:
            fg(entry.desc(2, bn, images, labels), idx, ws[:n], loss, None)
        assert str(ei.value) == "%s_fg: %d variables for batch_norm=%r" % (entry.stem, n, bn)
    with pytest.raises(ValueError) as ei:                        # the gradients' count is checked as well
        fg(entry.desc(2, True, images, labels), idx, ws, loss, ws[:-1])
    assert str(ei.value) == "%s_fg: %d variables for batch_norm=True" % (entry.stem, len(ws))
    with pytest.raises(_abi.L2OUnsupported) as ei:
        fg(entry.desc(1, True, images, labels), idx, ws, loss, None)
    assert str(ei.value) == "libl2o_hip error -2: %s_fg: unsupported minibatch 1" % entry.stem
    assert getattr(eng, entry.scratch) is s8


@pytest.mark.gpu
def test_engine_confocal_refusals(eng):
    """Batch 1, one point, ROI 2 x 2 x 2: the variable-count and the sim / img mismatch refusals, with their texts."""
    theta = [eng.tensor(np.full(1, 0.5, np.float32)) for _ in range(7)]
    loss = eng.zeros(1)
    d = _engine.ConfocalDesc(1, 1, (2, 2, 2))
    eng.confocal_fg(d, theta, theta, loss, None)
    assert np.isfinite(eng.to_numpy(loss)).all()
    with pytest.raises(ValueError) as ei:
        eng.confocal_fg(d, theta[:6], theta[:6], loss, None)
    assert str(ei.value) == "l2o_confocal_fg: 6 variables for 1 points"
    with pytest.raises(ValueError) as ei:                        # simulation mode without the simulation parameters
        eng.confocal_fg(d, theta, None, loss, None)
    assert str(ei.value) == "l2o_confocal_fg: 7 variables for 1 points"
    with pytest.raises(ValueError) as ei:                        # inference mode with them
        eng.confocal_fg(_engine.ConfocalDesc(1, 1, (2, 2, 2), eng.zeros(1, 8)), theta, theta, loss, None)
    assert str(ei.value) == "l2o_confocal_fg: 7 variables for 1 points"
