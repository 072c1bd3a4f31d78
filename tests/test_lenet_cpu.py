"""problems.LeNet (DM/problems.py:461-537, util.get_config("lenet")) without a GPU: the variables the factory declares, the
unsupported shapes and the missing-data error, the float64 reference's own correctness (central differences), the
library's new symbols, and the host wiring -- meta_loss / meta_minimize over the net on an oracle engine whose lenet_fg is
the float32 torch reference (lenet_reference.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import imagenet_harness as H
import lenet_reference as R
import oracle as O
from helpers import spec_of
from open_l2o_amd import _abi, problems, util

NET = H.NETS["lenet"]


@pytest.fixture
def engine():
    with H.as_default(H.oracle_engine(NET)) as e:
        yield e


def _data(n=64, seed=0):
    return problems.synthetic_cifar10(n, seed=seed)


_lenet = NET.problem                   # problems.LeNet("cifar10", ...) at conv_channels (6, 16), linear_layers (120, 84)


# 1. the factory
@pytest.mark.parametrize("batch_norm", [True, False])
def test_variables_names_shapes_order(batch_norm):
    loss = _lenet(batch_norm=batch_norm, data=_data())()
    assert [v.name for v in loss.variables] == R.names(batch_norm)
    assert [v.shape for v in loss.variables] == R.shapes(batch_norm)
    assert len(loss.variables) == (14 if batch_norm else 10)
    assert all(v.trainable for v in loss.variables)
    assert sum(int(np.prod(v.shape)) for v in loss.variables) == (62232 if batch_norm else 62006)
    (term,) = loss.terms
    assert term.kind == _abi.PROB_LENET == 8 and term.hyper["batch_size"] == 128
    assert term.hyper["batch_norm"] is batch_norm and term.hyper["images"].shape == (64, 3072)
    for v in loss.variables:                       # every w AND b from N(0, 0.01^2), every beta zero
        assert v.initializer == (("zeros",) if v.name.endswith("beta") else ("normal", 0.0, 0.01)), v.name
    if batch_norm:
        assert [v.name for v in loss.variables][:3] == ["conv_net_2d/conv_2d_0/w", "conv_net_2d/conv_2d_0/b",
                                                        "conv_net_2d/batch_norm_0/beta"]
        assert loss.variables[8].name == "mlp/batch_norm/beta" and loss.variables[11].name == "mlp/batch_norm_1/beta"
        assert loss.variables[6].shape == (400, 120) and loss.variables[13].shape == (10,)


def test_unsupported_shapes_and_batches():
    for kw in ({"conv_channels": None, "linear_layers": None}, {"conv_channels": (6, 8)}, {"linear_layers": (120,)},
               {"conv_channels": (6, 16, 32)}, {"linear_layers": (100, 84)}):
        with pytest.raises(NotImplementedError, match=r"\(6, 16\).*\(120, 84\)"):
            _lenet(data=_data(), **kw)
    with pytest.raises(NotImplementedError):
        problems.LeNet("cifar10", data=_data())          # the reference's None defaults
    for batch in (1, 1025):
        with pytest.raises(NotImplementedError):
            _lenet(batch_size=batch, data=_data())
    _lenet(batch_size=2, data=_data())
    _lenet(conv_channels=[6, 16], linear_layers=[120, 84], batch_size=1024, data=_data())


def test_missing_data_error(tmp_path, monkeypatch):
    monkeypatch.delenv("L2O_CIFAR10_DIR", raising=False)
    monkeypatch.chdir(tmp_path)
    for make in (lambda: util.get_config("lenet"), lambda: _lenet()):
        with pytest.raises(FileNotFoundError) as ei:
            make()
        assert isinstance(ei.value, NotImplementedError) and isinstance(ei.value, problems.Cifar10DataMissing)
        assert "L2O_CIFAR10_DIR" in str(ei.value)


# 2. util.get_config
def test_get_config():
    problem, net_config, na = util.get_config("lenet", problem_options={"data": _data()})
    loss = problem()
    assert [v.name for v in loss.variables] == R.names(True) and loss.terms[0].hyper["batch_size"] == 128
    assert loss.terms[0].kind == _abi.PROB_LENET
    assert net_config["cw"]["net_options"]["preprocess_name"] == "LogAndSign" and na is None
    problem, net_config, _ = util.get_config("lenet", net_name="RNNprop",
                                             problem_options={"data": _data(), "batch_size": 16, "batch_norm": False})
    assert "rp" in net_config and problem().terms[0].hyper["batch_size"] == 16
    assert [v.name for v in problem().variables] == R.names(False)


# 3. the float64 reference itself
@pytest.mark.parametrize("batch_norm", [True, False])
def test_reference_central_differences(batch_norm):
    """The float64 reference's gradient against central differences on a handful of coordinates of every variable; the
    biases that feed a batch norm have gradient 0."""
    d = _data(64, seed=3)
    rng = np.random.default_rng(4)
    images = d["images"].reshape(64, -1) + 0.05 * rng.random((64, 3072))
    net = R.LeNet(images, d["labels"], batch_norm)
    w = [a.astype(np.float64) for a in R.sample_weights(batch_norm, 5)]
    rows = rng.integers(0, 64, 12)
    f, g = net.fg(w, rows)
    assert np.isfinite(f) and (net.last_logits > 0).any() and (net.last_logits < 0).any()
    assert R.pool_ties(net.last_pre_pool) == 0 and R.pool_ties(net.last_pool_inputs) == 0
    H.check_central_differences(net, w, rows, R.names(batch_norm), g, rng, coords=4, rtol=1e-6)
    assert len(R.bn_fed_biases(batch_norm)) == (4 if batch_norm else 0)
    for kb, kw in R.bn_fed_biases(batch_norm):
        assert R.names(batch_norm)[kb].endswith("/b") and R.names(batch_norm)[kw].endswith("/w")
        assert np.abs(g[kb]).max() < 1e-12 * np.abs(g[kw]).max(), R.names(batch_norm)[kb]


def test_reference_pools_like_the_kernel():
    """max-pool(sigmoid(x)) == sigmoid(max-pool(x)) with the same argmax: the order the kernels and lenet_reference.py use
    is the reference's net."""
    d = _data(32, seed=5)
    net = R.LeNet(d["images"], d["labels"], True)
    w = [a.astype(np.float64) for a in R.sample_weights(True, 6)]
    net.fg(w, np.arange(16), want_grad=False)
    pool = torch.nn.functional.max_pool2d
    for pre, post in zip(net.last_pre_pool, net.last_pool_inputs):
        a, ia = pool(torch.tensor(pre), 2, 2, return_indices=True)
        b, ib = pool(torch.tensor(post), 2, 2, return_indices=True)
        assert torch.equal(torch.sigmoid(a), b) and torch.equal(ia, ib)


# 4. the library
def test_library_symbols_and_unroll_support():
    import __graft_entry__  # noqa: F401
    lib = _abi.lib()
    for name in ("l2o_lenet_fg", "l2o_lenet_scratch_floats"):
        assert name in _abi.PROTOTYPES["l2o_abi.h"]
        getattr(lib, name)
    assert lib.l2o_abi_version() == 15
    cc = spec_of(O.DM_LOGSIGN).to_c()
    p = _abi.Problem()
    p.kind, p.B_local, p.B_global, p.D, p.M = _abi.PROB_LENET, 1, 1, 62232, 62232
    assert lib.l2o_unroll_supported(C.byref(cc), C.byref(p)) == 0
    assert lib.l2o_unroll_record_supported(C.byref(cc), C.byref(p)) == 0
    H.check_batch_bounds(lib, NET)


# 5. host wiring
@pytest.mark.parametrize("net", ["dm_logsign", "rnnprop"])
def test_meta_loss_wiring(engine, net):
    """meta_loss over util.get_config("lenet") on the step-granular path == the oracle's multi-variable unroll over the same
    float32 evaluations, two chained unrolls."""
    H.check_meta_loss_wiring(engine, NET, net, n_data=96, T=3, batch=8)


def test_meta_minimize_and_refusals(engine):
    """One first-order training step on LeNet runs on the recording step path; second derivatives and the replicas' training
    step refuse it."""
    H.check_meta_minimize_and_refusals(engine, NET, n_data=64, batch=8, refusal=r"second_derivatives.*problems\.LeNet")


def test_replicas_run_one_at_a_time(engine):
    """Replicas.run over LeNet instances: no multi-instance kernel applies, so they run one after the other ("chip")."""
    H.check_replicas_one_at_a_time(engine, NET)
