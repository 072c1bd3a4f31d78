"""problems.vgg16_cifar10 (DM/problems.py:637-694, DM/vgg16.py, util.get_config("vgg16")) without a GPU: the variables the
factory declares, its refusals and the missing-data error, the float64 reference's own correctness (central differences),
the library's new symbols and scratch sizes, the companion table of later step-path kinds, and the host wiring -- meta_loss
/ meta_minimize over the net on an oracle engine whose vgg16_fg is the float32 torch reference (vgg16_reference.py)."""
import ctypes as C
import math

import numpy as np
import pytest

import imagenet_harness as H
import vgg16_reference as R
from open_l2o_amd import _abi, _engine, _graph_steps, problems, util
from test_training_gradient import GRAD_TOL

NARROW = R.NARROW_CHANNELS
NET = H.NETS["vgg16"]


@pytest.fixture
def engine():
    with H.as_default(H.oracle_engine(NET)) as e:
        yield e


def _data(n=64, seed=0):
    return problems.synthetic_cifar10(n, seed=seed)


# 1. the factory
def test_variables_names_shapes_order_initialisers():
    loss = problems.vgg16_cifar10("cifar10", data=_data())()
    assert [v.name for v in loss.variables] == R.names()
    assert [tuple(v.shape) for v in loss.variables] == R.shapes()
    assert len(loss.variables) == 28 and all(v.trainable for v in loss.variables)
    assert sum(int(np.prod(v.shape)) for v in loss.variables) == 14719818
    assert loss.variables[0].name == "block1_conv1/weights" and tuple(loss.variables[0].shape) == (3, 3, 3, 64)
    assert loss.variables[24].name == "block5_conv3/weights" and tuple(loss.variables[24].shape) == (3, 3, 512, 512)
    assert loss.variables[26].name == "fc/weights" and tuple(loss.variables[26].shape) == (512, 10)
    for v in loss.variables:
        if v.name == "fc/biases":
            assert v.initializer == ("ones",)
        elif v.name.endswith("biases"):
            assert v.initializer == ("zeros",), v.name
        else:
            assert v.initializer == ("normal", 0.0, 0.01), v.name
    (term,) = loss.terms
    assert term.kind == _abi.PROB_VGG16 == 10 and term.hyper["batch_size"] == 128
    assert term.hyper["channels"] == (64, 128, 256, 512, 512) and term.hyper["images"].shape == (64, 3072)
    # batch_norm is accepted and changes nothing
    other = problems.vgg16_cifar10("cifar10", batch_norm=True, data=_data())()
    assert [v.name for v in other.variables] == R.names() and other.terms[0].hyper["batch_norm"] is False
    narrow = problems.vgg16_cifar10("cifar10", data=_data(), channels=NARROW, batch_size=2)()
    assert [tuple(v.shape) for v in narrow.variables] == R.shapes(NARROW)


def test_refusals():
    data = _data(8)
    for channels in ((8, 16, 24, 40, 70), (4, 16, 24, 40, 72), (0, 16, 24, 40, 72), (8, 16, 24, 40, 520),
                     (8, 16, 24, 40), (8, 16, 24, 40, 72, 72), 64):
        with pytest.raises(NotImplementedError) as ei:
            problems.vgg16_cifar10("cifar10", data=data, channels=channels)
        assert str(ei.value).startswith("problems.vgg16_cifar10 is implemented for five channels, each a multiple of 8 in "
                                        "[8, 512] (got channels=")
    for batch in (1, 1025):
        with pytest.raises(NotImplementedError) as ei:
            problems.vgg16_cifar10("cifar10", data=data, batch_size=batch)
        assert str(ei.value) == "problems.vgg16_cifar10 is implemented for minibatches of 2 to 1024 (got %d)" % batch
    bad = {"images": np.zeros((8, 5, 5, 2), np.float32), "labels": data["labels"]}
    with pytest.raises(ValueError) as ei:
        problems.vgg16_cifar10("cifar10", data=bad)
    assert str(ei.value) == "problems.vgg16_cifar10 takes 32x32x3 images (got (8, 5, 5, 2))"
    problems.vgg16_cifar10("cifar10", data=data, batch_size=2, channels=[8, 8, 8, 8, 8])
    problems.vgg16_cifar10("cifar10", data=data, batch_size=1024, channels=(512,) * 5)


def test_missing_data_error(tmp_path, monkeypatch):
    monkeypatch.delenv("L2O_CIFAR10_DIR", raising=False)
    monkeypatch.chdir(tmp_path)
    for make in (lambda: util.get_config("vgg16"), lambda: problems.vgg16_cifar10("cifar10")):
        with pytest.raises(FileNotFoundError) as ei:
            make()
        assert isinstance(ei.value, NotImplementedError) and isinstance(ei.value, problems.Cifar10DataMissing)
        assert "L2O_CIFAR10_DIR" in str(ei.value)


# 2. util.get_config
def test_get_config():
    problem, net_config, na = util.get_config("vgg16", problem_options={"data": _data()})
    loss = problem()
    assert [v.name for v in loss.variables] == R.names() and loss.terms[0].hyper["batch_size"] == 128
    assert loss.terms[0].kind == _abi.PROB_VGG16
    assert net_config["cw"]["net_options"]["preprocess_name"] == "LogAndSign" and na is None
    problem, net_config, _ = util.get_config("vgg16", net_name="RNNprop",
                                             problem_options={"data": _data(), "batch_size": 16, "channels": NARROW})
    assert "rp" in net_config and problem().terms[0].hyper["batch_size"] == 16
    assert [tuple(v.shape) for v in problem().variables] == R.shapes(NARROW)


# 3. the table entry
def test_later_kinds_table():
    """vgg16 is kind 10 of the one table, with the entry type of the kinds before it; everything that looks a kind up reads
    that table."""
    assert set(range(5, 11)) <= set(_engine.STEP_OPTIMIZEES)
    e = _engine.STEP_OPTIMIZEES[_abi.PROB_VGG16]
    assert type(e) is _engine.StepOptimizee and _engine.step_optimizee(10) is e
    assert (e.method, e.stem, e.scratch, e.sampled) == ("vgg16_fg", "l2o_vgg16", "_vgg16_scratch", True)
    assert e.desc is _engine.Vgg16Desc and e.struct is _abi.Vgg16 and (e.struct, e.stem) in _abi.STEP_FG
    assert e.nvars(_engine.Vgg16Desc(2, NARROW, None, None)) == 28
    assert _engine._ENTRY_OF_METHOD["vgg16_fg"] is e and callable(_engine.HipEngine.vgg16_fg)
    kinds = tuple(range(11)) + (99,)
    assert tuple(k for k in kinds if _graph_steps.is_multivar(k)) == (5, 6, 7, 8, 9, 10)
    assert tuple(k for k in kinds if _graph_steps.is_sampled(k)) == (5, 6, 7, 8, 10)
    assert C.sizeof(_abi.Vgg16) == 48 and _abi.Vgg16.__doc__.startswith("struct l2o_vgg16")


# 4. the float64 reference itself
def test_reference_central_differences():
    """The float64 reference's gradient against central differences on a few coordinates of every variable, at O(1)
    activations.  (Not at the reference's initialisation: the pre-activations there are of the order 1e-8 deep in the net,
    so any step a difference can resolve crosses ReLU kinks.)"""
    d = _data(16, seed=3)
    net = R.Vgg16(d["images"], d["labels"], NARROW)
    w = [a.astype(np.float64) for a in R.sample_weights(NARROW, 5)]
    rng = np.random.default_rng(4)
    rows = rng.integers(0, 16, 3)
    f, g = net.fg(w, rows)
    assert np.isfinite(f) and 1.46 < f < 2.47
    for nm, a in zip(R.names(), g):
        assert np.abs(a).max() > 0, nm
    H.check_central_differences(net, w, rows, R.names(), g, rng, coords=3, rtol=1e-5)


def test_reference_at_the_initialisation():
    """At the reference's initialisation the signal shrinks by about 6e-8 through the thirteen layers: the float32 logits
    are exactly fc/biases and the loss exactly log 10, while every gradient block is non-zero and far above float32
    subnormals."""
    d = _data(16, seed=3)
    net = R.Vgg16(d["images"], d["labels"], NARROW)
    w = R.init_weights(NARROW, 5)
    f32, g32 = net.fg(w, np.arange(3))
    assert np.array_equal(net.last_logits, np.ones((3, 10), np.float32)) and f32 == np.float32(math.log(10))
    f64, g64 = net.fg([a.astype(np.float64) for a in w], np.arange(3))
    assert abs(f64 - math.log(10)) < 1e-6
    for nm, a in zip(R.names(), g64):
        assert np.abs(a).max() > 1e-30, nm


def test_float32_reference_within_a_third_of_the_bound():
    """The bound the GPU tests hold the kernels to is GRAD_TOL of a block's largest float64 entry unless the float32
    reference is itself further off than a third of that: it is not, at either weight scale."""
    d = _data(64, seed=6)
    net = R.Vgg16(d["images"], d["labels"], NARROW)
    rows = np.random.default_rng(7).integers(0, 64, 3)
    for make in (R.sample_weights, R.init_weights):
        w = make(NARROW, 8)
        f64, g64 = net.fg([a.astype(np.float64) for a in w], rows)
        f32, g32 = net.fg(w, rows)
        assert abs(f32 - f64) <= 1e-5 / 3 * abs(f64)
        for nm, a, b in zip(R.names(), g32, g64):
            assert np.abs(a - b).max() <= GRAD_TOL / 3 * np.abs(b).max(), nm


# 5. the library
def test_library_symbols_header_and_scratch():
    import __graft_entry__  # noqa: F401
    lib = _abi.lib()
    assert lib.l2o_abi_version() == 15 == _abi.L2O_ABI_VERSION
    assert _abi.source_build_id() == _abi.build_id()
    assert lib.l2o_vgg16_scratch_floats.restype is C.c_size_t and lib.l2o_vgg16_fg.argtypes == [C.POINTER(_abi.Vgg16)] + \
        [C.c_void_p] * 6
    m = _abi.Vgg16()
    m.n_data = 100

    def floats(batch, channels):
        m.batch = batch
        for k in range(5):
            m.channels[k] = channels[k]
        return int(lib.l2o_vgg16_scratch_floats(C.byref(m)))

    for batch, ok in ((1, False), (2, True), (128, True), (1024, True), (1025, False)):
        assert (floats(batch, NARROW) > 0) == ok, batch
    for channels in ((8, 16, 24, 40, 70), (0, 16, 24, 40, 72), (8, 16, 24, 40, 520), (4, 8, 8, 8, 8)):
        assert floats(2, channels) == 0, channels
    sizes = [floats(b, NARROW) for b in (2, 3, 37, 128, 1024)]
    assert sizes == sorted(set(sizes))
    ref = [floats(b, R.REFERENCE_CHANNELS) for b in (2, 128, 1024)]
    assert ref == sorted(set(ref)) and ref[0] > sizes[0]
    # what a sample needs at the least: its image, every layer's output and two gradient buffers of the largest one
    per_sample = 3072 + 2 * 65536 + 16384 + 2 * 32768 + 8192 + 3 * 16384 + 4096 + 3 * 8192 + 2048 + 3 * 2048 + 512 + 2 * 65536
    assert ref[1] >= 128 * per_sample and ref[1] < 128 * per_sample * 1.5
    assert floats(128, R.REFERENCE_CHANNELS) and lib.l2o_vgg16_fg(C.byref(m), None, None, None, None, None, None) == \
        _abi.L2O_ERR_ARG
    for batch in (1, 1025):
        m.batch = batch
        assert lib.l2o_vgg16_fg(C.byref(m), None, None, None, None, None, None) == _abi.L2O_ERR_UNSUPPORTED


# 6. host wiring
def _check_v0(v0):
    assert np.array_equal(v0[27], np.ones(10, np.float32)) and not v0[1].any() and v0[0].any()


@pytest.mark.parametrize("net", ["dm_logsign", "rnnprop"])
def test_meta_loss_wiring(engine, net):
    """meta_loss over util.get_config("vgg16") at narrow widths on the step-granular path == the oracle's multi-variable
    unroll over the same float32 evaluations, two chained unrolls."""
    H.check_meta_loss_wiring(engine, NET, net, n_data=32, T=2, batch=4, check_v0=_check_v0)


def test_meta_minimize_and_refusals(engine):
    """One first-order training step on the narrow net runs on the recording step path; second derivatives refuse it."""
    H.check_meta_minimize_and_refusals(engine, NET, n_data=32, batch=4, replicas=False)
