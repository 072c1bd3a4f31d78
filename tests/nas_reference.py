"""The reference's NAS-cell optimizee (problems.NAS, DM/problems.py:583-632) in torch on the CPU, float64 or float32: loss
and gradients of one minibatch in the project's layout (HWIO conv weights, [in, out] fc weights), through torch's autograd.
Written from the net's description; not a test module: the tests import it.

    net = Nas(images [N, 3072] or [N, 32, 32, 3], labels [N], batch_norm=True)
    f, grads = net.fg(variables, rows)          # variables / grads: the graph's order, 18 (10) arrays
    fg = net.flat_fg(shapes, idx)               # fg(x, t) of helpers.oracle_meta_grad, like helpers.mnist_fg

With L(x; name) = relu([batch norm](conv 3x3 stride 1 SAME (x, name/weights1) + name/biases1)):
    node0 = L(x; node0), n02 = L(node0; node0_onto_node2), node1 = L(node0; node1), n13 = L(node1; node1_onto_node3),
    node2 = avg_pool 3x3 stride 1 SAME (node1) + n02      (TF divides by the number of VALID cells: count_include_pad=False)
    node3 = node2 + n13 + node0,  nf = mean over the 1024 positions,  out = relu(nf fc_weights + fc_bias),
    loss = mean_b cross_entropy(out_b, label_b).
Batch norm is tf.layers.batch_normalization(training=True): per channel over all B * 1024 values, biased variance, eps 1e-3,
written out by hand (no torch batch_norm: its eps placement and its running statistics are not in question then).

Under batch norm a weight gradient is a sum over B * 1024 positions of terms that cancel down to about sqrt(B * 1024) of
them, so ONE ReLU mask that float32 rounding flips moves a block by about 1 / sqrt(B * 1024) of its largest entry: 2.8e-3
at minibatch 128.  ``fg`` therefore records ``last_margins``: per layer, how far the nearest batch-norm output is from 0 in
units of the rounding of a float32 sum of 9 C_in products at the scale of that layer's z, carried through the batch norm's
slope (:func:`_margin`)."""
import numpy as np
import torch
import torch.nn.functional as F

LAYERS = ("node0", "node0_onto_node2", "node1", "node1_onto_node3")
EPS = 1e-3


def names(batch_norm=True):
    out = []
    for i, nm in enumerate(LAYERS):
        out += [nm + "/weights1", nm + "/biases1"]
        if batch_norm:
            bn = "batch_normalization" + ("_%d" % i if i else "")
            out += [bn + "/gamma", bn + "/beta"]
    return out + ["fc_weights", "fc_bias"]


def shapes(batch_norm=True):
    out = []
    for i in range(4):
        out += [(3, 3, 3 if i == 0 else 16, 16), (16,)]
        if batch_norm:
            out += [(16,), (16,)]
    return out + [(16, 10), (10,)]


def avg_pool(x):
    """tf.nn.avg_pool(ksize 3, stride 1, SAME) of an NCHW tensor: the mean over the window's cells INSIDE the image."""
    return F.avg_pool2d(x, 3, stride=1, padding=1, count_include_pad=False)


class Nas(object):
    def __init__(self, images, labels, batch_norm=True):
        self.images = np.asarray(images, np.float32).reshape(-1, 32 * 32 * 3)
        self.labels = np.asarray(labels).astype(np.int64)
        self.batch_norm = bool(batch_norm)

    def forward(self, vs, x, y, keep=None):
        """The mean loss of NCHW images x with labels y under the torch variables vs; ``keep``: a dict that receives the
        intermediate tensors (pre-activations z_i, bn outputs y_i, node3, nf, out)."""
        it = iter(vs)

        def layer(h, i):
            w, b = next(it), next(it)
            z = F.conv2d(h, w.permute(3, 2, 0, 1), b, padding=1)                                   # HWIO -> OIHW, SAME
            yv, slope = z, torch.ones(1, z.shape[1], 1, 1, dtype=z.dtype)
            if self.batch_norm:
                gamma, beta = next(it), next(it)
                mean = z.mean(dim=(0, 2, 3), keepdim=True)
                var = ((z - mean) ** 2).mean(dim=(0, 2, 3), keepdim=True)
                slope = gamma.reshape(1, -1, 1, 1) / torch.sqrt(var + EPS)
                yv = gamma.reshape(1, -1, 1, 1) * (z - mean) / torch.sqrt(var + EPS) + beta.reshape(1, -1, 1, 1)
            if keep is not None:
                keep["z%d" % i], keep["y%d" % i] = z, yv
                keep.setdefault("margins", []).append(_margin(z.detach(), yv.detach(), slope.detach(), 9 * w.shape[2]))
            return F.relu(yv)

        node0 = layer(x, 0)
        n02 = layer(node0, 1)
        node1 = layer(node0, 2)
        n13 = layer(node1, 3)
        node2 = avg_pool(node1) + n02
        node3 = node2 + n13 + node0
        nf = node3.reshape(node3.shape[0], 16, -1).mean(dim=2)
        w, b = next(it), next(it)
        out = F.relu(nf @ w + b)
        if keep is not None:
            keep.update(node3=node3, nf=nf, out=out)
        return F.cross_entropy(out, y)

    def fg(self, variables, rows, want_grad=True):
        """(loss, [gradient per variable]) on the minibatch ``rows``, in the dtype of ``variables``."""
        dt = torch.float64 if np.asarray(variables[0]).dtype == np.float64 else torch.float32
        vs = [torch.tensor(np.asarray(v), dtype=dt).reshape(sh).requires_grad_(want_grad)
              for v, sh in zip(variables, shapes(self.batch_norm))]
        rows = np.asarray(rows).reshape(-1)
        x = torch.tensor(self.images[rows], dtype=dt).reshape(-1, 32, 32, 3).permute(0, 3, 1, 2)    # NHWC -> NCHW
        y = torch.tensor(self.labels[rows])
        keep = {}
        loss = self.forward(vs, x, y, keep)
        self.last_out = keep["out"].detach().numpy()
        self.last_margins = keep["margins"]
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


def _margin(z, y, slope, k):
    """How far the layer's ReLU inputs y = slope z + shift are from changing a mask, per channel in units of the rounding of
    a float32 sum of k products at the scale of z (its mean included: the images are positive), carried through the slope
    gamma / sqrt(var + eps) of the batch norm: 2^-24 sqrt(k) rms_c(z) |slope_c| (a random walk of k roundings).  The
    smallest over the channels."""
    unit = 2.0 ** -24 * np.sqrt(k) * z.pow(2).mean(dim=(0, 2, 3), keepdim=True).sqrt() * slope.abs()
    return float((y.abs() / unit.clamp(min=1e-300)).min())


def sample_weights(batch_norm, seed):
    """O(1) activations through the cell: conv weights of std sqrt(2 / (9 C_in)), fc weights of std 1, conv and fc biases
    from N(0, 0.1^2), gamma from N(1, 0.1^2) and beta from N(0, 0.1^2)."""
    rng = np.random.default_rng(seed)
    out = []
    for nm, sh in zip(names(batch_norm), shapes(batch_norm)):
        if len(sh) == 4:
            out.append(rng.normal(0, np.sqrt(2.0 / (9 * sh[2])), sh))
        elif len(sh) == 2:
            out.append(rng.normal(0, 1.0, sh))
        elif nm.endswith("gamma"):
            out.append(rng.normal(1.0, 0.1, sh))
        else:
            out.append(rng.normal(0, 0.1, sh))
    return [a.astype(np.float32) for a in out]


def init_weights(batch_norm, seed):
    """The reference's own initialisation: weights from N(0, 0.01^2), biases 0, gamma 1, beta 0."""
    rng = np.random.default_rng(seed)
    out = []
    for nm, sh in zip(names(batch_norm), shapes(batch_norm)):
        if len(sh) > 1:
            out.append(rng.normal(0, 0.01, sh))
        else:
            out.append(np.ones(sh) if nm.endswith("gamma") else np.zeros(sh))
    return [a.astype(np.float32) for a in out]
