"""problems.mnist_conv (DM/problems.py:291-352, util.get_config("mnist_conv")) without a GPU: the variables the factory
declares, the missing-data error, the float64 reference's own correctness (central differences), the library's new
symbols, and the host wiring -- meta_loss / meta_minimize over the conv net on an oracle engine whose mnist_conv_fg is
the float32 torch reference (conv_reference.py)."""
import ctypes as C

import numpy as np
import pytest

import imagenet_harness as H
import oracle as O
from conv_reference import MNIST as R
from helpers import spec_of
from open_l2o_amd import _abi, problems, util

NET = H.NETS["mnist_conv"]


@pytest.fixture
def engine():
    with H.as_default(H.oracle_engine(NET)) as e:
        yield e


def _data(n=64, seed=0):
    return problems.synthetic_mnist(n, seed=seed)


@pytest.mark.parametrize("batch_norm", [True, False])
def test_variables_names_shapes_order(batch_norm):
    loss = problems.mnist_conv(batch_norm=batch_norm, data=_data())()
    assert [v.name for v in loss.variables] == R.names(batch_norm)
    assert [v.shape for v in loss.variables] == R.shapes(batch_norm)
    assert all(v.trainable for v in loss.variables)
    assert sum(int(np.prod(v.shape)) for v in loss.variables) == (18218 if batch_norm else 18122)
    (term,) = loss.terms
    assert term.kind == _abi.PROB_MNIST_CONV == 6 and term.hyper["batch_size"] == 128
    inits = [v.initializer for v in loss.variables]
    assert inits[0] == ("normal", 0.0, 0.01) and inits[-2] == ("normal", 0.0, 0.01)
    assert inits[1] == ("zeros",) and inits[-1] == ("zeros",)
    if batch_norm:
        assert inits[2] == ("ones",) and inits[3] == ("zeros",)


def test_get_config():
    problem, net_config, na = util.get_config("mnist_conv", problem_options={"data": _data()})
    assert [v.name for v in problem().variables] == R.names(True)
    assert net_config["cw"]["net_options"]["preprocess_name"] == "LogAndSign" and na is None
    problem, net_config, _ = util.get_config("mnist_conv", net_name="RNNprop",
                                             problem_options={"data": _data(), "batch_size": 16})
    assert "rp" in net_config and problem().terms[0].hyper["batch_size"] == 16
    for name in ("cifar_conv", "lenet", "nas", "vgg16"):
        with pytest.raises(NotImplementedError):
            util.get_config(name)


def test_missing_data_error(monkeypatch):
    monkeypatch.delenv("L2O_MNIST_NPZ", raising=False)
    for make in (lambda: util.get_config("mnist_conv"), lambda: problems.mnist_conv()):
        with pytest.raises(FileNotFoundError) as ei:
            make()
        assert isinstance(ei.value, NotImplementedError) and "L2O_MNIST_NPZ" in str(ei.value)
    with pytest.raises(FileNotFoundError):                # problems.mnist: the same message and class
        problems.mnist(layers=(20,))


def test_unsupported_batch():
    with pytest.raises(NotImplementedError):
        problems.mnist_conv(batch_size=1, data=_data())
    with pytest.raises(NotImplementedError):
        problems.mnist_conv(batch_size=1025, data=_data())


@pytest.mark.parametrize("batch_norm", [True, False])
def test_reference_central_differences(batch_norm):
    """The float64 reference's gradient against central differences on a handful of coordinates of every variable; the
    conv biases under batch norm have gradient 0."""
    d = _data(64, seed=3)
    rng = np.random.default_rng(4)
    images = d["images"].reshape(64, -1) + 0.05 * rng.random((64, 784))
    net = R.ConvNet(images, d["labels"], batch_norm)
    w = [a.astype(np.float64) for a in R.sample_weights(batch_norm, 5, logit_scale=3.0)]
    rows = rng.integers(0, 64, 12)
    f, g = net.fg(w, rows)
    assert np.isfinite(f)
    H.check_central_differences(net, w, rows, R.names(batch_norm), g, rng, coords=4, rtol=1e-6)
    if batch_norm:
        assert np.abs(g[1]).max() < 1e-12 * np.abs(g[0]).max()
        assert np.abs(g[5]).max() < 1e-12 * np.abs(g[4]).max()


def test_library_symbols_and_unroll_support():
    import __graft_entry__  # noqa: F401
    lib = _abi.lib()
    for name in ("l2o_mnist_conv_fg", "l2o_mnist_conv_scratch_floats"):
        assert name in _abi.PROTOTYPES["l2o_abi.h"]
        getattr(lib, name)
    assert lib.l2o_abi_version() == 15
    cc = spec_of(O.DM_LOGSIGN).to_c()
    p = _abi.Problem()
    p.kind, p.B_local, p.B_global, p.D, p.M = _abi.PROB_MNIST_CONV, 1, 1, 18218, 18218
    assert lib.l2o_unroll_supported(C.byref(cc), C.byref(p)) == 0
    assert lib.l2o_unroll_record_supported(C.byref(cc), C.byref(p)) == 0
    H.check_batch_bounds(lib, NET)


@pytest.mark.parametrize("net", ["dm_logsign", "rnnprop"])
def test_meta_loss_wiring(engine, net):
    """meta_loss over util.get_config("mnist_conv") on the step-granular path == the oracle's multi-variable unroll over
    the same float32 evaluations, two chained unrolls."""
    H.check_meta_loss_wiring(engine, NET, net, n_data=96, T=3, batch=8)


def test_meta_minimize_and_refusals(engine):
    """One first-order training step on the conv net runs on the recording step path; second derivatives and the
    replicas' training step refuse it."""
    H.check_meta_minimize_and_refusals(engine, NET, n_data=64, batch=8)


def test_replicas_run_one_at_a_time(engine):
    """Replicas.run over conv-net instances: no multi-instance kernel applies, so they run one after the other ("chip")."""
    H.check_replicas_one_at_a_time(engine, NET)
