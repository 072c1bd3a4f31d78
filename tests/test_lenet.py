"""problems.LeNet on the MI355X: l2o_lenet_fg (csrc/l2o_lenet.h) against the float64 torch reference (lenet_reference.py),
the unroll of meta_loss over the net against a float64 host unroll, the first-order meta-gradient against
helpers.oracle_meta_grad, and the RNNProp evaluation driver on it.

Bounds (the project's, as test_cifar_conv.py; imagenet_harness.py holds them): a gradient block within 5e-4 of its largest
entry, or 3 x the float32 reference's own distance from float64 where that is larger (test_training_gradient's rule); the
loss within 1e-5 relative; the four biases that feed a batch norm (exactly 0 in exact arithmetic) within 1e-6 of the largest
entry of their layer's weight gradient.  The images carry a little uniform noise on top of problems.synthetic_cifar10, and
the test asserts on the float64 and float32 reference activations that no two pooling candidates tie exactly (a tie broken
differently by rounding moves a gradient to another pixel): a condition on the inputs that excludes nothing.  Kernel and
reference both pool the normalised pre-activation and apply the sigmoid after (lenet_reference.py says why that is the same
net).

The carry of the four batch-norm-fed biases into the second meta-training step is not compared: their gradient is 0 in
exact arithmetic, so what any implementation feeds the optimizer for them is its own rounding noise (test_fg_vs_float64
bounds it), and under RNNProp's g / sqrt(v) that noise steers their trajectories.  Every other carried quantity, the
RNNProp LSTM state included, and every meta-gradient block keeps the 3 x rule (of the float32 oracle's own distance from
float64): the 5 x that test_cifar_conv.py needed for the RNNProp state is not needed here.  Measured on one MI355X, over
both optimizers and the ten compared variables: wherever a carried array was further than CARRY_TOL from float64 (up to
3.2e-4 of its largest entry, the LSTM state of linear_1/w under RNNProp), it was at most 1.65 x the float32 oracle's own
distance; the larger multiples (up to 4.6 x) all belong to arrays within 3e-6, inside CARRY_TOL."""
import numpy as np
import pytest

import imagenet_harness as H
import lenet_reference as R
from imagenet_harness import eng  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

NET = H.NETS["lenet"]


# ------------------------------------------------------------------------------------------------------------------
# 1. one evaluation: l2o_lenet_fg against float64
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("point", ["sample", "init"])
@pytest.mark.parametrize("batch_norm", [True, False])
@pytest.mark.parametrize("batch", [128, 37])
def test_fg_vs_float64(eng, batch, batch_norm, point):
    """``sample``: O(1) activations, non-zero beta and biases; ``init``: the reference's own initialisation scale (all w,
    b ~ N(0, 0.01^2), beta 0), where the normalised signal comes from 1e-2-scale pre-activations.

    Measured on one MI355X: every block within 3e-7 of its largest float64 entry (float32 torch on the CPU: 4e-7), the
    loss within 3.2e-7 relative.  The batch-norm-fed biases, as a fraction of their layer's largest weight-gradient entry,
    over the four batch-norm cases (float32 torch autograd's own ratio on the same inputs in brackets): conv_2d_0/b
    0.8-4.4e-7 (0.6-1.5e-6), conv_2d_1/b 1.2-5.5e-7 (0.4-1.5e-6), linear_0/b 1.5-3.9e-8 (3.6-8.6e-7), linear_1/b
    0.1-1.9e-7 (1.8-4.9e-7): all inside the 1e-6.  With a single float for the linear layers' batch mean linear_0/b was
    at 2.6e-6 at [128-True-sample], which is why k_ln_fc keeps that mean as two floats."""
    n = 300
    data = H.noisy_cifar(n, seed=batch + batch_norm)
    net = R.LeNet(data["images"], data["labels"], batch_norm)
    w = R.sample_weights(batch_norm, seed=batch) if point == "sample" else R.init_weights(batch_norm, seed=batch)
    rows = np.random.default_rng(batch).integers(0, n, batch)
    f64, g64 = net.fg([a.astype(np.float64) for a in w], rows)
    # no pooling window ties: in float64 neither among the pre-activations nor among their sigmoids (so the reference's
    # order, pool after the sigmoid, routes the same gradient), in float32 among the pre-activations both the kernel and
    # the float32 reference rank.  The float32 SIGMOIDS are not asserted on: at [init, no batch norm] 29 (minibatch 128)
    # and 3 (minibatch 37) windows tie there, so "no ties in either precision" does not hold for the post-sigmoid values
    # (lenet_reference.py)
    assert R.pool_ties(net.last_pre_pool) == 0 and R.pool_ties(net.last_pool_inputs) == 0
    f32, g32 = net.fg(w, rows)
    assert R.pool_ties(net.last_pre_pool) == 0
    H.check_fg_vs_float64(eng, NET, net, rows, w, f64, g64, f32, g32)


# ------------------------------------------------------------------------------------------------------------------
# 2. the unroll: meta_loss over the net, T = 20, against a float64 host unroll
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", ["dm_logsign", "rnnprop"])
def test_unroll_vs_float64(eng, net):
    T, batch, n = 20, 128, 512
    data = H.noisy_cifar(n, seed=41)
    idx = np.random.default_rng(42).integers(0, n, size=(T + 1, batch))
    H.check_unroll_vs_float64(eng, NET, net, T, batch, data, idx)


# ------------------------------------------------------------------------------------------------------------------
# 3. the meta-gradient: two consecutive train steps against helpers.oracle_meta_grad
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dm_logsign", "rnnprop"])
def test_meta_gradient_vs_float64(eng, name):
    H.check_meta_gradient_vs_float64(eng, NET, name, 10, 128, H.noisy_cifar(1024, seed=51))


# ------------------------------------------------------------------------------------------------------------------
# 4. the RNNProp evaluation driver with the shipped MLP-trained optimizer, pointed at LeNet
# ------------------------------------------------------------------------------------------------------------------
def test_evaluate_rnnprop_driver():
    H.check_driver(NET, 1024, 40, 900)
