"""The reference's VGG-16 optimizee (problems.vgg16_cifar10, DM/problems.py:637-694 with DM/vgg16.py:44-98) in torch on the
CPU, float64 or float32: loss and gradients of one minibatch in the project's layout (HWIO conv weights, [in, out] linear
weights), through torch's autograd.  Written from the net's description; not a test module: the tests import it.

    net = Vgg16(images [N, 3072] or [N, 32, 32, 3], labels [N], channels=(64, 128, 256, 512, 512))
    f, grads = net.fg(variables, rows)          # variables / grads: the graph's order, 28 arrays
    fg = net.flat_fg(shapes, idx)               # fg(x, t) of helpers.oracle_meta_grad, like helpers.mnist_fg

Five blocks of (2, 2, 3, 3, 3) layers, each conv 3x3 SAME + bias -> ReLU, max-pool 2 after each block, linear x10, softmax,
and cross_entropy ON THE PROBABILITIES (the reference hands its softmax output to
sparse_softmax_cross_entropy_with_logits).  No batch norm, no dropout.

Dead pooling windows need no special inputs: a window whose four post-ReLU values are all 0 sends its gradient to the first
candidate in torch's max_pool2d and in the kernels alike, and the ReLU's mask (y > 0) zeroes it in both."""
import numpy as np
import torch
import torch.nn.functional as F

REFERENCE_CHANNELS = (64, 128, 256, 512, 512)
NARROW_CHANNELS = (8, 16, 24, 40, 72)
_PER_BLOCK = (2, 2, 3, 3, 3)


def names():
    out = []
    for b, n in enumerate(_PER_BLOCK):
        for i in range(n):
            out += ["block%d_conv%d/weights" % (b + 1, i + 1), "block%d_conv%d/biases" % (b + 1, i + 1)]
    return out + ["fc/weights", "fc/biases"]


def shapes(channels=REFERENCE_CHANNELS):
    out, c_in = [], 3
    for n, c in zip(_PER_BLOCK, channels):
        for _ in range(n):
            out += [(3, 3, c_in, c), (c,)]
            c_in = c
    return out + [(c_in, 10), (10,)]


class Vgg16(object):
    def __init__(self, images, labels, channels=REFERENCE_CHANNELS):
        self.images = np.asarray(images, np.float32).reshape(-1, 32 * 32 * 3)
        self.labels = np.asarray(labels).astype(np.int64)
        self.channels = tuple(channels)

    def fg(self, variables, rows, want_grad=True):
        """(loss, [gradient per variable]) on the minibatch ``rows``, in the dtype of ``variables``."""
        dt = torch.float64 if np.asarray(variables[0]).dtype == np.float64 else torch.float32
        vs = [torch.tensor(np.asarray(v), dtype=dt).reshape(sh).requires_grad_(want_grad)
              for v, sh in zip(variables, shapes(self.channels))]
        rows = np.asarray(rows).reshape(-1)
        h = torch.tensor(self.images[rows], dtype=dt).reshape(-1, 32, 32, 3).permute(0, 3, 1, 2)    # NHWC -> NCHW
        y = torch.tensor(self.labels[rows])
        it = iter(vs)
        self.last_margins = []
        for n in _PER_BLOCK:
            for i in range(n):
                w, b = next(it), next(it)
                z = F.conv2d(h, w.permute(3, 2, 0, 1), b, padding=1)                               # HWIO -> OIHW, SAME
                self.last_margins.append(_margin(z.detach(), pooled=i == n - 1, k=9 * w.shape[2]))
                h = F.relu(z)
            h = F.max_pool2d(h, 2)
        w, b = next(it), next(it)
        z = h.reshape(h.shape[0], -1) @ w + b
        self.last_logits = z.detach().numpy()
        loss = F.cross_entropy(F.softmax(z, dim=1), y)                                             # the reference's quirk
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


def _margin(z, pooled, k):
    """How far the layer's pre-activations z [B, C, H, W] are from changing a decision -- a ReLU mask that matters, or a
    pool's arg-max --, in units of the rounding of a float32 sum of k products of this layer's scale, 2^-24 sqrt(k) rms(z)
    (a random walk of k roundings).  A unit that feeds a pool matters only as its window's maximum: the distance is then
    min(|z_max|, z_max - max(z_second, 0))."""
    unit = 2.0 ** -24 * np.sqrt(k) * float(z.pow(2).mean().sqrt())
    if not pooled:
        return float(z.abs().min()) / unit
    b, c, hh, ww = z.shape
    win = z.reshape(b, c, hh // 2, 2, ww // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(b, c, hh // 2, ww // 2, 4)
    top = win.sort(dim=-1).values
    zmax, second = top[..., 3], top[..., 2].clamp(min=0)
    return float(torch.minimum(zmax.abs(), torch.where(zmax > 0, zmax - second, zmax.abs())).min()) / unit


def sample_weights(channels, seed):
    """O(1) activations through all thirteen layers: conv weights of std sqrt(2 / (9 C_in)), fc weights of std 1 / sqrt(C),
    every bias from N(0, 0.1^2)."""
    rng = np.random.default_rng(seed)
    out = []
    for sh in shapes(channels):
        if len(sh) == 4:
            out.append(rng.normal(0, np.sqrt(2.0 / (9 * sh[2])), sh))
        elif len(sh) == 2:
            out.append(rng.normal(0, 1.0 / np.sqrt(sh[0]), sh))
        else:
            out.append(rng.normal(0, 0.1, sh))
    return [a.astype(np.float32) for a in out]


def init_weights(channels, seed):
    """The reference's own initialisation: weights from N(0, 0.01^2), conv biases 0, fc/biases 1."""
    rng = np.random.default_rng(seed)
    out = [rng.normal(0, 0.01, sh).astype(np.float32) if len(sh) > 1 else np.zeros(sh, np.float32)
           for sh in shapes(channels)]
    out[-1] = np.ones(10, np.float32)
    return out
