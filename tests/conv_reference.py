"""The reference's two conv-net optimizees in torch on the CPU, float64 or float32: problems.mnist_conv
(DM/problems.py:291-352; 28x28x1 images, stride-1 convs, [512, 10] fc weights with rows in NHWC flatten order) and
problems.cifar10 (DM/problems.py:369-458; 32x32x3 images, stride-2 convs, [32, 10] fc weights).
One net over a shape description: loss and gradients of one minibatch in the project's layout (HWIO conv weights), through
torch's autograd.  Not a test module: the tests import ``MNIST`` or ``CIFAR``, each with the four names below bound to its
shape.

    R = conv_reference.MNIST                    # or CIFAR
    net = R.ConvNet(images [N, side * side * c_in] or [N, side, side, c_in], labels [N], batch_norm=True)
    f, grads = net.fg(variables, rows)          # variables / grads: the graph's order (10 with batch norm, 6 without)
    fg = net.flat_fg(shapes, idx)               # fg(x, t) of helpers.oracle_meta_grad, like helpers.mnist_fg
    R.shapes(batch_norm), R.names(batch_norm), R.sample_weights(batch_norm, seed, logit_scale)

After fg(): net.last_pre_pool holds the two [B, C, H, W] arrays in front of the ReLUs and max-pools (ReLU is non-decreasing, so
a window's first maximum before it is the window's first maximum after it wherever that maximum is positive, and elsewhere
the ReLU stops the gradient), for the tests' tie checks (lenet_reference.pool_ties / pool_tie_mask).
"""
import collections
import functools
import types

import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-3           # tf.layers.batch_normalization's default epsilon

# side x side x c_in images; both convs (3x3 to 16 channels, 5x5 to 32, VALID, each followed by a 2x2 max-pool) at
# ``stride``; fc_in: what is left for the [fc_in, 10] layer (MNIST 28 -> 26 -> 13 -> 9 -> 4: 4 * 4 * 32; CIFAR 32 -> 15 -> 7
# -> 2 -> 1: 32)
Shape = collections.namedtuple("Shape", "side c_in stride fc_in")


def shapes(shape, batch_norm=True):
    out = [(3, 3, shape.c_in, 16), (16,)]
    if batch_norm:
        out += [(16,), (16,)]
    out += [(5, 5, 16, 32), (32,)]
    if batch_norm:
        out += [(32,), (32,)]
    return out + [(shape.fc_in, 10), (10,)]


def names(batch_norm=True):
    out = ["conv_layer1/weights1", "conv_layer1/biases1"]
    if batch_norm:
        out += ["batch_normalization/gamma", "batch_normalization/beta"]
    out += ["conv_layer2/weights1", "conv_layer2/biases1"]
    if batch_norm:
        out += ["batch_normalization_1/gamma", "batch_normalization_1/beta"]
    return out + ["fc_weights", "fc_bias"]


class ConvNet(object):
    def __init__(self, shape, images, labels, batch_norm=True):
        self.shape = shape
        self.images = np.asarray(images, np.float32).reshape(-1, shape.side * shape.side * shape.c_in)
        self.labels = np.asarray(labels).astype(np.int64)
        self.batch_norm = bool(batch_norm)

    def fg(self, variables, rows, want_grad=True):
        """(loss, [gradient per variable]) on the minibatch ``rows``, in the dtype of ``variables``."""
        s = self.shape
        dt = torch.float64 if np.asarray(variables[0]).dtype == np.float64 else torch.float32
        vs = [torch.tensor(np.asarray(v), dtype=dt).reshape(sh).requires_grad_(want_grad)
              for v, sh in zip(variables, shapes(s, self.batch_norm))]
        rows = np.asarray(rows).reshape(-1)
        x = torch.tensor(self.images[rows], dtype=dt).reshape(-1, s.side, s.side, s.c_in).permute(0, 3, 1, 2)  # NHWC -> NCHW
        y = torch.tensor(self.labels[rows])
        it = iter(vs)
        self.last_pre_pool = []

        def layer(h, c_out):
            w, b = next(it), next(it)
            h = F.conv2d(h, w.permute(3, 2, 0, 1), stride=s.stride) + b.view(1, c_out, 1, 1)      # HWIO -> OIHW, VALID
            if self.batch_norm:
                gamma, beta = next(it), next(it)
                h = F.batch_norm(h, None, None, gamma, beta, training=True, eps=EPS)
            self.last_pre_pool.append(h.detach().numpy())
            return F.max_pool2d(F.relu(h), 2, 2)

        h = layer(x, 16)
        h = layer(h, 32)
        flat = h.permute(0, 2, 3, 1).reshape(h.shape[0], -1)                                     # NHWC flatten
        wf, bf = next(it), next(it)
        self.last_logits = (flat @ wf + bf).detach().numpy()                                   # (before the ReLU)
        logits = F.relu(flat @ wf + bf)
        loss = F.cross_entropy(logits, y)
        if not want_grad:
            return float(loss), None
        grads = torch.autograd.grad(loss, vs)
        npdt = np.float64 if dt == torch.float64 else np.float32
        return npdt(loss.detach().numpy()), [g.detach().numpy().astype(npdt) for g in grads]

    def flat_fg(self, shps, idx, scales=None):
        """``fg(x, t)`` over the flat concatenation of the variables (helpers.oracle_meta_grad): evaluation t uses minibatch
        row idx[t]; with scales (one array per variable) f(x * s) and s * grad f(x * s)."""
        sizes = [int(np.prod(sh)) for sh in shps]
        offs = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
        s = None if scales is None else np.concatenate([np.asarray(a, np.float64).reshape(-1) for a in scales])

        def fg(x, t):
            sc = None if s is None else s.astype(x.dtype)
            xs = x if sc is None else x * sc
            vs = [xs[offs[i]:offs[i + 1]].reshape(sh) for i, sh in enumerate(shps)]
            f, grads = self.fg(vs, np.asarray(idx[t]))
            g = np.concatenate([a.reshape(-1) for a in grads])
            return f, (g if sc is None else g * sc)
        return fg


def sample_weights(shape, batch_norm, seed, logit_scale=1.0):
    """Weights at which the net's pieces all matter: conv weights of N(0, 1 / fan-in)-like scale so that the activations are
    O(1) without batch norm too, non-trivial gamma / beta / biases, and fc weights large enough that the logits take both
    signs (both sides of the ReLU on the logits)."""
    rng = np.random.default_rng(seed)
    out = [rng.normal(0, 1.0 / np.sqrt(9 * shape.c_in), (3, 3, shape.c_in, 16)), rng.normal(0, 0.1, 16)]
    if batch_norm:
        out += [rng.uniform(0.5, 1.5, 16), rng.normal(0, 0.2, 16)]
    out += [rng.normal(0, 1.0 / np.sqrt(400), (5, 5, 16, 32)), rng.normal(0, 0.1, 32)]
    if batch_norm:
        out += [rng.uniform(0.5, 1.5, 32), rng.normal(0, 0.2, 32)]
    out += [rng.normal(0, logit_scale / np.sqrt(shape.fc_in), (shape.fc_in, 10)), rng.normal(0, 0.2, 10)]
    return [a.astype(np.float32) for a in out]


def _bound_to(shape):
    return types.SimpleNamespace(shape=shape, names=names, shapes=functools.partial(shapes, shape),
                                 ConvNet=functools.partial(ConvNet, shape),
                                 sample_weights=functools.partial(sample_weights, shape))


MNIST = _bound_to(Shape(side=28, c_in=1, stride=1, fc_in=512))
CIFAR = _bound_to(Shape(side=32, c_in=3, stride=2, fc_in=32))
