"""problems.NAS (DM/problems.py:540-634, util.get_config("nas")) without a GPU: the variables the factory declares, its
refusals and the missing-data error, the open registry of step-path kinds, the library's new symbols and scratch sizes, the
float64 reference's own correctness (central differences, the average pool by hand, the two facts the kernels' backward pass
rests on), and the host wiring -- meta_loss / meta_minimize over the net on an oracle engine whose nas_fg is the float32
torch reference (nas_reference.py)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import imagenet_harness as H
import nas_reference as R
from open_l2o_amd import _abi, _engine, _graph_steps, problems, util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NET = H.NETS["nas"]


@pytest.fixture
def engine():
    with H.as_default(H.oracle_engine(NET)) as e:
        yield e


def _data(n=64, seed=0):
    return problems.synthetic_cifar10(n, seed=seed)


# 1. the factory
@pytest.mark.parametrize("batch_norm", [True, False])
def test_variables_names_shapes_order_initialisers(batch_norm):
    loss = problems.NAS("cifar10", batch_norm=batch_norm, data=_data())()
    assert [v.name for v in loss.variables] == R.names(batch_norm)
    assert [tuple(v.shape) for v in loss.variables] == R.shapes(batch_norm)
    assert len(loss.variables) == (18 if batch_norm else 10) and all(v.trainable for v in loss.variables)
    assert sum(int(np.prod(v.shape)) for v in loss.variables) == (7706 if batch_norm else 7578)
    assert loss.variables[0].name == "node0/weights1" and tuple(loss.variables[0].shape) == (3, 3, 3, 16)
    per = 4 if batch_norm else 2
    assert [loss.variables[per * i].name for i in range(4)] == [
        "node0/weights1", "node0_onto_node2/weights1", "node1/weights1", "node1_onto_node3/weights1"]
    assert tuple(loss.variables[per].shape) == (3, 3, 16, 16)
    if batch_norm:
        assert [loss.variables[4 * i + 2].name for i in range(4)] == [
            "batch_normalization/gamma", "batch_normalization_1/gamma", "batch_normalization_2/gamma",
            "batch_normalization_3/gamma"]
    assert [v.name for v in loss.variables[-2:]] == ["fc_weights", "fc_bias"]
    for v in loss.variables:
        if v.name.endswith("weights1") or v.name == "fc_weights":
            assert v.initializer == ("normal", 0.0, 0.01), v.name
        elif v.name.endswith("gamma"):
            assert v.initializer == ("ones",), v.name
        else:
            assert v.initializer == ("zeros",), v.name
    (term,) = loss.terms
    assert term.kind == _abi.PROB_NAS == 11 and term.hyper["batch_size"] == 128
    assert term.hyper["batch_norm"] is batch_norm and term.hyper["images"].shape == (64, 3072)


def test_signature_and_refusals():
    import inspect
    assert str(inspect.signature(problems.NAS)) == (
        "(path, batch_norm=True, batch_size=128, num_threads=4, min_queue_examples=1000, mode='train', data=None, "
        "sampler=None)")
    data = _data(8)
    for batch in (1, 1025):
        with pytest.raises(NotImplementedError) as ei:
            problems.NAS("cifar10", data=data, batch_size=batch)
        assert str(ei.value) == "problems.NAS is implemented for minibatches of 2 to 1024 (got %d)" % batch
    bad = {"images": np.zeros((8, 5, 5, 2), np.float32), "labels": data["labels"]}
    with pytest.raises(ValueError):
        problems.NAS("cifar10", data=bad)
    problems.NAS("cifar10", data=data, batch_size=2, num_threads=9, min_queue_examples=3)
    problems.NAS("cifar10", data=data, batch_size=1024)


# 2. util.get_config
def test_get_config():
    problem, net_config, na = util.get_config("nas", problem_options={"data": _data()})
    loss = problem()
    assert [v.name for v in loss.variables] == R.names(True) and loss.terms[0].hyper["batch_size"] == 128
    assert loss.terms[0].kind == _abi.PROB_NAS
    assert net_config["cw"]["net_options"]["preprocess_name"] == "LogAndSign" and na is None
    problem, net_config, _ = util.get_config("nas", net_name="RNNprop",
                                             problem_options={"data": _data(), "batch_size": 16, "batch_norm": False})
    assert "rp" in net_config and problem().terms[0].hyper["batch_size"] == 16
    assert [v.name for v in problem().variables] == R.names(False)


def test_missing_data_error_and_cifar_multi(tmp_path, monkeypatch):
    monkeypatch.delenv("L2O_CIFAR10_DIR", raising=False)
    monkeypatch.chdir(tmp_path)
    for make in (lambda: util.get_config("nas"), lambda: problems.NAS("cifar10")):
        with pytest.raises(FileNotFoundError) as ei:
            make()
        assert isinstance(ei.value, NotImplementedError) and isinstance(ei.value, problems.Cifar10DataMissing)
    with pytest.raises(NotImplementedError) as ei:
        util.get_config("cifar-multi")
    assert "conv_channels" in str(ei.value) and not isinstance(ei.value, FileNotFoundError)


# 3. the registry
def test_registry_membership():
    """Membership, never equality: the kind after this one changes no line here."""
    e = _engine.step_optimizee(_abi.PROB_NAS)
    assert type(e) is _engine.StepOptimizee and _engine.STEP_OPTIMIZEES[11] is e
    assert (e.method, e.stem, e.scratch, e.sampled) == ("nas_fg", "l2o_nas", "_nas_scratch", True)
    assert e.desc is _engine.NasDesc and issubclass(_engine.NasDesc, _engine.ImageNetDesc)
    assert e.struct is _abi.Nas and issubclass(_abi.Nas, _abi.ImageNet) and (e.struct, e.stem) in _abi.STEP_FG
    assert e.nvars(_engine.NasDesc(2, True, None, None)) == 18 and e.nvars(_engine.NasDesc(2, False, None, None)) == 10
    assert _engine._ENTRY_OF_METHOD["nas_fg"] is e and callable(_engine.HipEngine.nas_fg)
    assert _graph_steps.is_multivar(11) and _graph_steps.is_sampled(11)
    # every kind answers through the same functions as the table says
    for kind, entry in _engine.STEP_OPTIMIZEES.items():
        assert _engine.step_optimizee(kind) is entry
        assert _graph_steps.is_multivar(kind) and _graph_steps.is_sampled(kind) == entry.sampled
        assert _engine._ENTRY_OF_METHOD[entry.method] is entry
    assert set(range(5, 12)) <= set(_engine.STEP_OPTIMIZEES)
    kinds = tuple(range(12)) + (99,)
    assert tuple(k for k in kinds if _graph_steps.is_multivar(k)) == (5, 6, 7, 8, 9, 10, 11)
    assert tuple(k for k in kinds if _graph_steps.is_sampled(k)) == (5, 6, 7, 8, 10, 11)
    assert _graph_steps.is_sampled(_abi.PROB_CONFOCAL) is False and _graph_steps.is_multivar(_abi.PROB_CONFOCAL)
    for kind in (0, 1, 2, 3, 4, 99):
        assert _engine.step_optimizee(kind) is None
        assert not _graph_steps.is_multivar(kind) and not _graph_steps.is_sampled(kind)
    assert _engine._ENTRY_OF_METHOD["vgg16_fg"] is _engine.STEP_OPTIMIZEES[_abi.PROB_VGG16]


# 4. the library
def test_library_symbols_header_and_scratch():
    import __graft_entry__  # noqa: F401
    lib = _abi.lib()
    with open(os.path.join(ROOT, "include", "l2o_nas_abi.h")) as f:
        raw = f.read()
    assert lib.l2o_abi_version() == 15 == _abi.L2O_ABI_VERSION and _abi.PROB_NAS == 11
    assert _abi.source_build_id() == _abi.build_id()
    assert lib.l2o_nas_scratch_floats.restype is C.c_size_t and lib.l2o_nas_fg.argtypes == [C.POINTER(_abi.Nas)] + \
        [C.c_void_p] * 6
    assert [n for n, _ in _abi.Nas._fields_] == ["batch", "n_data", "batch_norm", "flags", "images", "labels"]
    m = _abi.Nas()
    m.n_data = 100

    def floats(batch, batch_norm=1, flags=0, n_data=100):
        m.batch, m.batch_norm, m.flags, m.n_data = batch, batch_norm, flags, n_data
        return int(lib.l2o_nas_scratch_floats(C.byref(m)))

    for batch, ok in ((1, False), (2, True), (128, True), (1024, True), (1025, False), (0, False), (-3, False)):
        assert (floats(batch) > 0) == ok, batch
    assert floats(2, batch_norm=2) == 0 and floats(2, batch_norm=-1) == 0 and floats(2, flags=1) == 0
    assert floats(2, n_data=0) == 0 and floats(2, batch_norm=0) == floats(2, batch_norm=1) > 0
    assert int(lib.l2o_nas_scratch_floats(None)) == 0

    # the header's formula
    def formula(b):
        return b * (3072 + 6 * 16384) + 448 + 2 * 64 * b + 3 * 16 * b + (b + 3) // 4 * 4 + min(4 * b, 256) * 4608

    assert "min(4 batch, 256) * 4608" in raw
    for b in (2, 3, 37, 128, 1024):
        assert floats(b) == formula(b), b
    m.batch, m.batch_norm, m.flags = 128, 1, 0
    assert lib.l2o_nas_fg(C.byref(m), None, None, None, None, None, None) == _abi.L2O_ERR_ARG
    for batch, bn, flags in ((1, 1, 0), (1025, 1, 0), (2, 2, 0), (2, 1, 4)):
        m.batch, m.batch_norm, m.flags = batch, bn, flags
        assert lib.l2o_nas_fg(C.byref(m), None, None, None, None, None, None) == _abi.L2O_ERR_UNSUPPORTED


# 5. the float64 reference itself
@pytest.mark.parametrize("batch_norm", [True, False])
def test_reference_central_differences(batch_norm):
    d = _data(16, seed=3)
    net = R.Nas(d["images"], d["labels"], batch_norm)
    w = [a.astype(np.float64) for a in R.sample_weights(batch_norm, 5)]
    rng = np.random.default_rng(4)
    rows = rng.integers(0, 16, 3)
    f, g = net.fg(w, rows)
    assert np.isfinite(f) and f > 0
    for k, nm in enumerate(R.names(batch_norm)):
        gmax = np.abs(g[k]).max()
        if batch_norm and nm.endswith("biases1"):
            assert gmax < 1e-12, nm                               # batch norm removes a per-channel shift
        else:
            assert gmax > 0, nm
    H.check_central_differences(net, w, rows, R.names(batch_norm), g, rng, coords=3, rtol=1e-5)


def test_reference_average_pool_by_hand():
    """4 x 4, values 0..15: a corner divides by 4, an edge by 6, the interior by 9."""
    x = torch.arange(16, dtype=torch.float64).reshape(1, 1, 4, 4)
    p = R.avg_pool(x)[0, 0].numpy()
    assert p[0, 0] == (0 + 1 + 4 + 5) / 4.0
    assert p[0, 1] == (0 + 1 + 2 + 4 + 5 + 6) / 6.0
    assert p[1, 0] == (0 + 1 + 4 + 5 + 8 + 9) / 6.0
    assert abs(p[1, 1] - (0 + 1 + 2 + 4 + 5 + 6 + 8 + 9 + 10) / 9.0) < 1e-15
    assert p[3, 3] == (10 + 11 + 14 + 15) / 4.0
    assert p[3, 2] == (9 + 10 + 11 + 13 + 14 + 15) / 6.0


def test_reference_backward_facts():
    """What csrc/l2o_nas.h rests on: dL/dnode3 is u / 1024 at every position (u = dL/dnf), and the average pool's adjoint
    applied to a position-constant field is that constant times k(y) k(x), k = 5/6, 7/6, 1, ..., 1, 7/6, 5/6."""
    d = _data(16, seed=3)
    net = R.Nas(d["images"], d["labels"], True)
    vs = [torch.tensor(a.astype(np.float64)).requires_grad_(True) for a in R.sample_weights(True, 5)]
    x = torch.tensor(net.images[:3], dtype=torch.float64).reshape(-1, 32, 32, 3).permute(0, 3, 1, 2)
    keep = {}
    loss = net.forward(vs, x, torch.tensor(net.labels[:3]), keep)
    dnode3, u = torch.autograd.grad(loss, [keep["node3"], keep["nf"]])
    assert float(u.abs().max()) > 0
    want = (u / 1024.0).reshape(3, 16, 1, 1).expand(3, 16, 32, 32)
    assert float((dnode3 - want).abs().max()) <= 1e-15 * float(want.abs().max())
    k = np.ones(32)
    k[[0, 31]], k[[1, 30]] = 5.0 / 6.0, 7.0 / 6.0
    a = torch.zeros(2, 3, 32, 32, dtype=torch.float64, requires_grad=True)
    const = torch.tensor([[0.5, -2.0, 3.0], [1.0, 7.0, -0.25]], dtype=torch.float64).reshape(2, 3, 1, 1)
    (da,) = torch.autograd.grad((R.avg_pool(a) * const).sum(), a)
    want = const.numpy() * (k[:, None] * k[None, :])[None, None]
    assert np.abs(da.numpy() - want).max() < 1e-14
    # ... and so the mean of the pooled array is the k k-weighted mean of the array
    b = torch.tensor(np.random.default_rng(0).random((2, 3, 32, 32)))
    lhs = R.avg_pool(b).mean(dim=(2, 3)).numpy()
    rhs = (b.numpy() * (k[:, None] * k[None, :])[None, None]).sum(axis=(2, 3)) / 1024.0
    assert np.abs(lhs - rhs).max() < 1e-14


# 6. host wiring
def _check_v0(v0):
    assert np.array_equal(v0[2], np.ones(16, np.float32)) and not v0[1].any() and not v0[3].any() and v0[0].any()


@pytest.mark.parametrize("net", ["dm_logsign", "rnnprop"])
def test_meta_loss_wiring(engine, net):
    """meta_loss over util.get_config("nas") on the step-granular path == the oracle's multi-variable unroll over the same
    float32 evaluations, two chained unrolls of two steps: the graph builds a NasDesc and draws a minibatch per
    evaluation."""
    H.check_meta_loss_wiring(engine, NET, net, n_data=32, T=2, batch=4, check_v0=_check_v0)


def test_meta_minimize_and_refusals(engine):
    """One first-order training step runs on the recording step path; second derivatives refuse the net at graph build."""
    H.check_meta_minimize_and_refusals(engine, NET, n_data=32, batch=4, replicas=False)
