"""The reference's LeNet optimizee (problems.LeNet, DM/problems.py:461-537, as util.get_config("lenet") builds it) in torch
on the CPU, float64 or float32: loss and gradients of one minibatch in the project's layout (HWIO conv weights, [in, out]
linear weights, NHWC flatten), through torch's autograd.  Written from the net's description (Sonnet 1.11's ConvNet2D / MLP /
BatchNorm defaults); not a test module: the tests import it.

    net = LeNet(images [N, 3072] or [N, 32, 32, 3], labels [N], batch_norm=True)
    f, grads = net.fg(variables, rows)          # variables / grads: the graph's order (14 with batch norm, 10 without)
    fg = net.flat_fg(shapes, idx)               # fg(x, t) of helpers.oracle_meta_grad, like helpers.mnist_fg

The reference pools the sigmoid's outputs; sigmoid is strictly increasing, so this module pools the normalised
pre-activation and applies the sigmoid to the pooled value: the same function and the same gradient unless two candidates
of a window tie exactly, and free of the ties that the sigmoid's compression creates in float32 (pre-activations of 1e-2
scale land on the same float next to 0.5: measured at the reference's initialisation scale without batch norm, 29 windows
of a minibatch of 128 and 3 of one of 37 tie among the float32 sigmoids, none among the pre-activations and none in float64
in either form -- so "no ties in either precision" holds for the pre-activations only, not for the float32 values the
reference itself ranks).  The float32 yardstick therefore shares this choice with the kernels; the float64 one is checked
for both orders (tests/test_lenet_cpu.py::test_reference_pools_like_the_kernel, and the tie assertions of test_lenet.py on
the float64 sigmoids too).  After fg(): net.last_pre_pool holds the two [B, C, H, W] arrays the max-pools
ranked and net.last_pool_inputs their sigmoids (what the reference ranks), for the tests' tie check.
"""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-3           # snt.BatchNorm's default epsilon

_CONV = [(5, 5, 3, 6), (5, 5, 6, 16)]
_WIDTHS = [400, 120, 84, 10]


def shapes(batch_norm=True):
    out = []
    for sh in _CONV:
        out += [sh, (sh[3],)] + ([(sh[3],)] if batch_norm else [])
    for i in range(3):
        out += [(_WIDTHS[i], _WIDTHS[i + 1]), (_WIDTHS[i + 1],)]
        if batch_norm and i < 2:
            out.append((_WIDTHS[i + 1],))
    return out


def names(batch_norm=True):
    out = []
    for i in range(2):
        out += ["conv_net_2d/conv_2d_%d/w" % i, "conv_net_2d/conv_2d_%d/b" % i]
        if batch_norm:
            out.append("conv_net_2d/batch_norm_%d/beta" % i)
    for i in range(3):
        out += ["mlp/linear_%d/w" % i, "mlp/linear_%d/b" % i]
        if batch_norm and i < 2:
            out.append("mlp/batch_norm%s/beta" % ("" if i == 0 else "_1"))
    return out


def bn_fed_biases(batch_norm=True):
    """(index of the bias, index of its layer's weight) for the biases that feed a batch norm: gradient 0 in exact
    arithmetic."""
    return [(1, 0), (4, 3), (7, 6), (10, 9)] if batch_norm else []


class LeNet(object):
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
        h = torch.tensor(self.images[rows], dtype=dt).reshape(-1, 32, 32, 3).permute(0, 3, 1, 2)    # NHWC -> NCHW
        y = torch.tensor(self.labels[rows])
        it = iter(vs)
        self.last_pool_inputs, self.last_pre_pool = [], []
        for _ in range(2):
            w, b = next(it), next(it)
            h = F.conv2d(h, w.permute(3, 2, 0, 1)) + b.view(1, -1, 1, 1)                            # HWIO -> OIHW, VALID
            if self.batch_norm:
                h = F.batch_norm(h, None, None, None, next(it), training=True, eps=EPS)           # an offset, no scale
            self.last_pre_pool.append(h.detach().numpy())
            self.last_pool_inputs.append(torch.sigmoid(h).detach().numpy())
            h = torch.sigmoid(F.max_pool2d(h, 2, 2))
        h = h.permute(0, 2, 3, 1).reshape(h.shape[0], -1)                                         # NHWC flatten
        for i in range(3):
            w, b = next(it), next(it)
            h = h @ w + b
            if i < 2:
                if self.batch_norm:
                    h = F.batch_norm(h, None, None, None, next(it), training=True, eps=EPS)
                h = torch.sigmoid(h)
        self.last_logits = h.detach().numpy()
        loss = F.cross_entropy(h, y)
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


def pool_tie_mask(m):
    """[B, C, H // 2, W // 2] booleans: the 2x2 pooling windows of the [B, C, H, W] array whose two largest entries are
    equal (a last odd row / column belongs to no window, as in VALID pooling)."""
    b, c, hh, ww = m.shape
    m = m[:, :, :hh // 2 * 2, :ww // 2 * 2]
    win = m.reshape(b, c, hh // 2, 2, ww // 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(b, c, hh // 2, ww // 2, 4)
    top = np.sort(win, axis=-1)
    return top[..., 3] == top[..., 2]


def pool_ties(maps):
    """Number of 2x2 pooling windows of the [B, C, H, W] arrays whose two largest entries are equal."""
    return sum(int(pool_tie_mask(m).sum()) for m in maps)


def sample_weights(batch_norm, seed):
    """Weights at which the net's pieces all matter: weights of 1 / sqrt(fan-in)-like scale so that the pre-activations are
    O(1) without batch norm too (the sigmoids leave their linear range), non-zero biases and beta, logits of both signs."""
    rng = np.random.default_rng(seed)
    out = []
    for sh in _CONV:
        fan = sh[0] * sh[1] * sh[2]
        out += [rng.normal(0, 2.0 / np.sqrt(fan), sh), rng.normal(0, 0.2, sh[3])]
        if batch_norm:
            out.append(rng.normal(0, 0.3, sh[3]))
    for i in range(3):
        out += [rng.normal(0, 3.0 / np.sqrt(_WIDTHS[i]), (_WIDTHS[i], _WIDTHS[i + 1])), rng.normal(0, 0.2, _WIDTHS[i + 1])]
        if batch_norm and i < 2:
            out.append(rng.normal(0, 0.3, _WIDTHS[i + 1]))
    return [a.astype(np.float32) for a in out]


def init_weights(batch_norm, seed):
    """The reference's own initialisation: every w and b from N(0, 0.01^2), every beta 0."""
    rng = np.random.default_rng(seed)
    return [np.zeros(sh, np.float32) if nm.endswith("beta") else rng.normal(0, 0.01, sh).astype(np.float32)
            for nm, sh in zip(names(batch_norm), shapes(batch_norm))]
