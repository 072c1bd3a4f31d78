"""problems.cifar10 (DM/problems.py:369-458, util.get_config("cifar_conv")) without a GPU: the variables the factory
declares, the binary-file loader and the missing-data error, the float64 reference's own correctness (central
differences), the library's new symbols, and the host wiring -- meta_loss / meta_minimize over the conv net on an oracle
engine whose cifar_conv_fg is the float32 torch reference (conv_reference.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import imagenet_harness as H
import oracle as O
from conv_reference import CIFAR as R
from helpers import spec_of
from open_l2o_amd import _abi, problems, util

NET = H.NETS["cifar_conv"]


@pytest.fixture
def engine():
    with H.as_default(H.oracle_engine(NET)) as e:
        yield e


def _data(n=64, seed=0):
    return problems.synthetic_cifar10(n, seed=seed)


@pytest.mark.parametrize("batch_norm", [True, False])
def test_variables_names_shapes_order(batch_norm):
    loss = problems.cifar10("cifar10", batch_norm=batch_norm, data=_data())()
    assert [v.name for v in loss.variables] == R.names(batch_norm)
    assert [v.shape for v in loss.variables] == R.shapes(batch_norm)
    assert all(v.trainable for v in loss.variables)
    assert sum(int(np.prod(v.shape)) for v in loss.variables) == (13706 if batch_norm else 13610)
    (term,) = loss.terms
    assert term.kind == _abi.PROB_CIFAR_CONV == 7 and term.hyper["batch_size"] == 128
    assert term.hyper["images"].shape == (64, 3072)
    inits = [v.initializer for v in loss.variables]
    k2 = 4 if batch_norm else 2
    assert inits[0] == inits[k2] == inits[-2] == ("normal", 0.0, 0.01)
    assert inits[1] == inits[k2 + 1] == inits[-1] == ("zeros",)
    if batch_norm:
        assert inits[2] == inits[6] == ("ones",) and inits[3] == inits[7] == ("zeros",)


def test_synthetic_cifar10():
    a, b = problems.synthetic_cifar10(200, seed=3), problems.synthetic_cifar10(200, seed=3)
    assert a["images"].shape == (200, 32, 32, 3) and a["images"].dtype == np.float32 and a["labels"].shape == (200,)
    assert np.array_equal(a["images"], b["images"]) and np.array_equal(a["labels"], b["labels"])
    assert a["images"].min() >= 0.0 and a["images"].max() <= 1.0 and set(a["labels"]) <= set(range(10))
    # class-separable: every image is nearer its own class mean than any other
    x = a["images"].reshape(200, -1)
    means = np.stack([x[a["labels"] == c].mean(0) for c in range(10)])
    d = ((x[:, None, :] - means[None]) ** 2).sum(-1)
    assert (d.argmin(1) == a["labels"]).all()
    noisy = problems.synthetic_cifar10(200, seed=3, label_noise=0.5)
    assert np.array_equal(noisy["images"], a["images"]) and not np.array_equal(noisy["labels"], a["labels"])


def test_get_config():
    problem, net_config, na = util.get_config("cifar_conv", problem_options={"data": _data()})
    loss = problem()
    assert [v.name for v in loss.variables] == R.names(True) and loss.terms[0].hyper["batch_size"] == 128
    assert net_config["cw"]["net_options"]["preprocess_name"] == "LogAndSign" and na is None
    problem, net_config, _ = util.get_config("cifar_conv", net_name="RNNprop",
                                             problem_options={"data": _data(), "batch_size": 16})
    assert "rp" in net_config and problem().terms[0].hyper["batch_size"] == 16


def test_others_still_unimplemented():
    for name in ("lenet", "nas", "vgg16", "cifar-multi"):
        with pytest.raises(NotImplementedError) as ei:
            util.get_config(name)
    # cifar-multi has its own stub: the reference calls cifar10 with arguments its own cifar10 does not take
    assert "conv_channels" in str(ei.value)


def _write_batches(root, counts, seed):
    """A tiny cifar-10-batches-bin under root: {file name: (labels, CHW uint8 images)}."""
    rng = np.random.default_rng(seed)
    folder = os.path.join(root, "cifar-10-batches-bin")
    os.makedirs(folder)
    out = {}
    for name, n in counts.items():
        labels = rng.integers(0, 10, n).astype(np.uint8)
        chw = rng.integers(0, 256, (n, 3, 32, 32)).astype(np.uint8)
        rec = np.concatenate([labels[:, None], chw.reshape(n, -1)], axis=1)
        rec.tofile(os.path.join(folder, name))
        out[name] = (labels, chw)
    return out


def test_binary_loader(tmp_path, monkeypatch):
    monkeypatch.delenv("L2O_CIFAR10_DIR", raising=False)
    counts = {"data_batch_%d.bin" % i: i + 1 for i in range(1, 6)}
    counts["test_batch.bin"] = 3
    files = _write_batches(str(tmp_path), counts, seed=1)
    loss = problems.cifar10(str(tmp_path), batch_size=2)()
    hyper = loss.terms[0].hyper
    labels = np.concatenate([files["data_batch_%d.bin" % i][0] for i in range(1, 6)])
    chw = np.concatenate([files["data_batch_%d.bin" % i][1] for i in range(1, 6)])
    assert hyper["images"].shape == (len(labels), 3072) and hyper["images"].dtype == np.float32
    np.testing.assert_array_equal(hyper["labels"], labels)
    want = chw.transpose(0, 2, 3, 1).astype(np.float32) / 255.0             # CHW -> HWC, / 255
    np.testing.assert_array_equal(hyper["images"].reshape(-1, 32, 32, 3), want)
    assert hyper["images"].reshape(-1, 32, 32, 3)[0, 1, 2, 0] == chw[0, 0, 1, 2] / np.float32(255.0)
    # mode="test" reads test_batch.bin only; L2O_CIFAR10_DIR replaces the path
    monkeypatch.setenv("L2O_CIFAR10_DIR", str(tmp_path))
    hyper = problems.cifar10("nowhere", mode="test", batch_size=2)().terms[0].hyper
    np.testing.assert_array_equal(hyper["labels"], files["test_batch.bin"][0])
    np.testing.assert_array_equal(hyper["images"].reshape(-1, 32, 32, 3),
                                  files["test_batch.bin"][1].transpose(0, 2, 3, 1).astype(np.float32) / 255.0)
    with pytest.raises(ValueError):
        problems.cifar10("nowhere", mode="validation")


def test_missing_data_error(tmp_path, monkeypatch):
    monkeypatch.delenv("L2O_CIFAR10_DIR", raising=False)
    monkeypatch.chdir(tmp_path)
    for make in (lambda: util.get_config("cifar_conv"), lambda: problems.cifar10("cifar10")):
        with pytest.raises(FileNotFoundError) as ei:
            make()
        assert isinstance(ei.value, NotImplementedError) and isinstance(ei.value, problems.Cifar10DataMissing)
        msg = str(ei.value)
        assert "L2O_CIFAR10_DIR" in msg and "synthetic_cifar10" in msg
        assert os.path.join("cifar10", "cifar-10-batches-bin", "data_batch_1.bin") in msg


def test_unsupported_batch():
    with pytest.raises(NotImplementedError):
        problems.cifar10("cifar10", batch_size=1, data=_data())
    with pytest.raises(NotImplementedError):
        problems.cifar10("cifar10", batch_size=1025, data=_data())


@pytest.mark.parametrize("batch_norm", [True, False])
def test_reference_central_differences(batch_norm):
    """The float64 reference's gradient against central differences on a handful of coordinates of every variable; the
    conv biases under batch norm have gradient 0."""
    d = _data(64, seed=3)
    rng = np.random.default_rng(4)
    images = d["images"].reshape(64, -1) + 0.05 * rng.random((64, 3072))
    net = R.ConvNet(images, d["labels"], batch_norm)
    w = [a.astype(np.float64) for a in R.sample_weights(batch_norm, 5, logit_scale=3.0)]
    rows = rng.integers(0, 64, 12)
    f, g = net.fg(w, rows)
    assert np.isfinite(f) and (net.last_logits > 0).any() and (net.last_logits < 0).any()
    H.check_central_differences(net, w, rows, R.names(batch_norm), g, rng, coords=4, rtol=1e-6)
    if batch_norm:
        assert np.abs(g[1]).max() < 1e-12 * np.abs(g[0]).max()
        assert np.abs(g[5]).max() < 1e-12 * np.abs(g[4]).max()


def test_library_symbols_and_unroll_support():
    import __graft_entry__  # noqa: F401
    lib = _abi.lib()
    for name in ("l2o_cifar_conv_fg", "l2o_cifar_conv_scratch_floats"):
        assert name in _abi.PROTOTYPES["l2o_abi.h"]
        getattr(lib, name)
    assert lib.l2o_abi_version() == 15
    cc = spec_of(O.DM_LOGSIGN).to_c()
    p = _abi.Problem()
    p.kind, p.B_local, p.B_global, p.D, p.M = _abi.PROB_CIFAR_CONV, 1, 1, 13706, 13706
    assert lib.l2o_unroll_supported(C.byref(cc), C.byref(p)) == 0
    assert lib.l2o_unroll_record_supported(C.byref(cc), C.byref(p)) == 0
    H.check_batch_bounds(lib, NET)


@pytest.mark.parametrize("net", ["dm_logsign", "rnnprop"])
def test_meta_loss_wiring(engine, net):
    """meta_loss over util.get_config("cifar_conv") on the step-granular path == the oracle's multi-variable unroll over
    the same float32 evaluations, two chained unrolls."""
    H.check_meta_loss_wiring(engine, NET, net, n_data=96, T=3, batch=8)


def test_meta_minimize_and_refusals(engine):
    """One first-order training step on the conv net runs on the recording step path; second derivatives and the
    replicas' training step refuse it."""
    H.check_meta_minimize_and_refusals(engine, NET, n_data=64, batch=8)


def test_replicas_run_one_at_a_time(engine):
    """Replicas.run over conv-net instances: no multi-instance kernel applies, so they run one after the other ("chip")."""
    H.check_replicas_one_at_a_time(engine, NET)
