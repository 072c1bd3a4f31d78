"""The reference's CIFAR-10 conv-net optimizee (problems.cifar10, DM/problems.py:369-458) in torch on the CPU, float64 or
float32: loss and gradients of one minibatch in the project's layout (HWIO conv weights, [32, 10] fc weights), through
torch's autograd.  Not a test module: the tests import it.

    net = ConvNet(images [N, 3072] or [N, 32, 32, 3], labels [N], batch_norm=True)
    f, grads = net.fg(variables, rows)          # variables / grads: the graph's order (10 with batch norm, 6 without)
    fg = net.flat_fg(shapes, idx)               # fg(x, t) of helpers.oracle_meta_grad, like helpers.mnist_fg

After fg(): net.last_pre_pool holds the two [B, C, H, W] arrays in front of the ReLUs and max-pools (ReLU is non-decreasing, so
a window's first maximum before it is the window's first maximum after it wherever that maximum is positive, and elsewhere
the ReLU stops the gradient), for the tests' tie checks (lenet_reference.pool_ties / pool_tie_mask).
"""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-3           # tf.layers.batch_normalization's default epsilon


def shapes(batch_norm=True):
    out = [(3, 3, 3, 16), (16,)]
    if batch_norm:
        out += [(16,), (16,)]
    out += [(5, 5, 16, 32), (32,)]
    if batch_norm:
        out += [(32,), (32,)]
    return out + [(32, 10), (10,)]


def names(batch_norm=True):
    out = ["conv_layer1/weights1", "conv_layer1/biases1"]
    if batch_norm:
        out += ["batch_normalization/gamma", "batch_normalization/beta"]
    out += ["conv_layer2/weights1", "conv_layer2/biases1"]
    if batch_norm:
        out += ["batch_normalization_1/gamma", "batch_normalization_1/beta"]
    return out + ["fc_weights", "fc_bias"]


class ConvNet(object):
    def __init__(self, images, labels, batch_norm=True):
        self.images = np.asarray(images, np.float32).reshape(-1, 32 * 32 * 3)
        self.labels = np.asarray(labels).astype(np.int64)
        self.batch_norm = bool(batch_norm)

    def fg(self, variables, rows, want_grad=True):
        """(loss, [gradient per variable]) on the minibatch ``rows``, in the dtype of ``variables``."""
        dt = torch.float64 if np.asarray(variables[0]).dtype == np.float64 else torch.float32
        vs = [torch.tensor(np.asarray(v), dtype=dt).reshape(sh).requires_grad_(want_grad)
              for v, sh in zip(variables, shapes(self.batch_norm))]
        rows = np.asarray(rows).reshape(-1)
        x = torch.tensor(self.images[rows], dtype=dt).reshape(-1, 32, 32, 3).permute(0, 3, 1, 2)    # NHWC -> NCHW
        y = torch.tensor(self.labels[rows])
        it = iter(vs)
        self.last_pre_pool = []

        def layer(h, c_out):
            w, b = next(it), next(it)
            h = F.conv2d(h, w.permute(3, 2, 0, 1), stride=2) + b.view(1, c_out, 1, 1)           # HWIO -> OIHW, VALID
            if self.batch_norm:
                gamma, beta = next(it), next(it)
                h = F.batch_norm(h, None, None, gamma, beta, training=True, eps=EPS)
            self.last_pre_pool.append(h.detach().numpy())
            return F.max_pool2d(F.relu(h), 2, 2)

        h = layer(x, 16)                                                                         # [B, 16, 7, 7]
        h = layer(h, 32)                                                                         # [B, 32, 1, 1]
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


def sample_weights(batch_norm, seed, logit_scale=1.0):
    """Weights at which the net's pieces all matter: conv weights of N(0, 0.3^2 / fan-in)-like scale so that the activations
    are O(1) without batch norm too, non-trivial gamma / beta / biases, and fc weights large enough that the logits take
    both signs (both sides of the ReLU on the logits)."""
    rng = np.random.default_rng(seed)
    out = [rng.normal(0, 1.0 / np.sqrt(27), (3, 3, 3, 16)), rng.normal(0, 0.1, 16)]
    if batch_norm:
        out += [rng.uniform(0.5, 1.5, 16), rng.normal(0, 0.2, 16)]
    out += [rng.normal(0, 1.0 / np.sqrt(400), (5, 5, 16, 32)), rng.normal(0, 0.1, 32)]
    if batch_norm:
        out += [rng.uniform(0.5, 1.5, 32), rng.normal(0, 0.2, 32)]
    out += [rng.normal(0, logit_scale / np.sqrt(32), (32, 10)), rng.normal(0, 0.2, 10)]
    return [a.astype(np.float32) for a in out]
