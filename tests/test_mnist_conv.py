"""problems.mnist_conv on the MI355X: l2o_mnist_conv_fg (csrc/l2o_mnist_conv.h) against the float64 torch reference
(conv_reference.py), the unroll of meta_loss over the conv net against a float64 host unroll, the first-order
meta-gradient against helpers.oracle_meta_grad, and the RNNProp evaluation driver on it.

Bounds (imagenet_harness.py holds them): a gradient block within 5e-4 of its largest entry, or 3 x the float32 reference's
own distance from float64 where that is larger (test_mlp_training_gradient's rule); the conv biases under batch norm
(exactly 0 in exact arithmetic) within 1e-6 of the largest entry of that layer's weight gradient.  The images carry a little
uniform noise on top of problems.synthetic_mnist, so that no two pooling candidates tie exactly (a tie broken differently by
rounding moves a gradient to another pixel)."""
import numpy as np
import pytest

import imagenet_harness as H
from conv_reference import MNIST as R
from imagenet_harness import eng  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

NET = H.NETS["mnist_conv"]


# ------------------------------------------------------------------------------------------------------------------
# 1. one evaluation: l2o_mnist_conv_fg against float64
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch_norm", [True, False])
@pytest.mark.parametrize("batch", [128, 37])
def test_fg_vs_float64(eng, batch, batch_norm):
    n = 300
    data = H.noisy_mnist(n, seed=batch + batch_norm)
    net = R.ConvNet(data["images"], data["labels"], batch_norm)
    w = R.sample_weights(batch_norm, seed=batch, logit_scale=3.0)
    rows = np.random.default_rng(batch).integers(0, n, batch)
    f64, g64 = net.fg([a.astype(np.float64) for a in w], rows)
    f32, g32 = net.fg(w, rows)
    assert (net.last_logits > 0).any() and (net.last_logits < 0).any()          # both sides of the ReLU on the logits
    H.check_fg_vs_float64(eng, NET, net, rows, w, f64, g64, f32, g32)


# ------------------------------------------------------------------------------------------------------------------
# 2. the unroll: meta_loss over the conv net, T = 20, against a float64 host unroll
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", ["dm_logsign", "rnnprop"])
def test_unroll_vs_float64(eng, net):
    T, batch, n = 20, 128, 512
    data = H.noisy_mnist(n, seed=41)
    idx = np.random.default_rng(42).integers(0, n, size=(T + 1, batch))
    H.check_unroll_vs_float64(eng, NET, net, T, batch, data, idx)


# ------------------------------------------------------------------------------------------------------------------
# 3. the meta-gradient: two consecutive train steps against helpers.oracle_meta_grad
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dm_logsign", "rnnprop"])
def test_meta_gradient_vs_float64(eng, name):
    H.check_meta_gradient_vs_float64(eng, NET, name, 10, 128, H.noisy_mnist(1024, seed=51))


# ------------------------------------------------------------------------------------------------------------------
# 4. the RNNProp evaluation driver with the shipped MLP-trained optimizer, pointed at the conv net
# ------------------------------------------------------------------------------------------------------------------
def test_evaluate_rnnprop_driver():
    H.check_driver(NET, 1024, 40, 900)
