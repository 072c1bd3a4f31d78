"""Reference for the second derivatives of the MLP optimizee (problems.mnist): the loss and its Hessian-vector product in
torch (double backward; float64 unless asked otherwise), the unroll of MetaOptimizer.meta_minimize restated in torch float64
with a per-step minibatch f(x, t) -- tests/test_second_derivatives.py::_torch_grad, plus RNNProp's Adam-normalised inputs --
and an oracle-backed engine with ``mlp_hvp``, so that the host logic of the coupled BPTT runs in the CPU suite."""
import numpy as np
import torch

from oracle_engine import OracleEngine


def widths_of(n_in, hidden, n_out=10):
    return [int(n_in)] + [int(h) for h in hidden] + [int(n_out)]


def shapes_of(n_in, hidden, n_out=10):
    """[w0, b0, w1, b1, ...] shapes in Sonnet's order (the graph's variable order)."""
    w = widths_of(n_in, hidden, n_out)
    return [sh for l in range(len(w) - 1) for sh in ((w[l], w[l + 1]), (w[l + 1],))]


def mlp_loss(ws, X, y, activation):
    """Mean softmax cross-entropy of the MLP [w0, b0, ..., wL, bL] on the rows X [B, n_in] with labels y [B] (torch)."""
    a = X
    L = len(ws) // 2 - 1
    for l in range(L + 1):
        a = a @ ws[2 * l] + ws[2 * l + 1]
        if l < L:
            a = torch.sigmoid(a) if activation == "sigmoid" else torch.relu(a)
    return torch.nn.functional.cross_entropy(a, y, reduction="mean")


def hvp(ws, us, images, labels, rows, activation, dtype=torch.float64):
    """H(ws; rows) us by double backward, in ``dtype``; arrays in, float64 arrays out."""
    X = torch.tensor(np.asarray(images, np.float64).reshape(len(labels), -1)[np.asarray(rows)]).to(dtype)
    y = torch.tensor(np.asarray(labels)[np.asarray(rows)].astype(np.int64))
    wt = [torch.tensor(np.asarray(w, np.float64)).to(dtype).requires_grad_(True) for w in ws]
    ut = [torch.tensor(np.asarray(u, np.float64)).to(dtype) for u in us]
    g = torch.autograd.grad(mlp_loss(wt, X, y, activation), wt, create_graph=True)
    dot = sum((gi * ui).sum() for gi, ui in zip(g, ut))
    out = torch.autograd.grad(dot, wt, allow_unused=True)
    return [np.zeros(w.shape) if o is None else o.detach().double().numpy() for o, w in zip(out, wt)]


def split(x, shapes):
    """The flat concatenation x (torch) -> one tensor per shape."""
    out, off = [], 0
    for sh in shapes:
        n = int(np.prod(sh))
        out.append(x[off:off + n].reshape(sh))
        off += n
    return out


def mnist_f(images, labels, idx, shapes, activation, scales=None, weight=1.0):
    """``f(x, t)`` for torch_meta_grad over the MLP: x the flat float64 concatenation of its variables, evaluation t on the
    minibatch rows idx[t]; with per-coordinate scales (one array per variable) the loss at x * s; times ``weight``."""
    X = torch.tensor(np.asarray(images, np.float64).reshape(len(labels), -1))
    y = torch.tensor(np.asarray(labels).astype(np.int64))
    s = None if scales is None else torch.tensor(np.concatenate([np.asarray(a, np.float64).reshape(-1) for a in scales]))

    def f(x, t):
        rows = torch.tensor(np.asarray(idx[t]).astype(np.int64))
        xs = x if s is None else x * s
        return weight * mlp_loss(split(xs, shapes), X[rows], y[rows], activation)
    return f


def torch_meta_grad(cfg, params, f, x0, T, second, step0=1, beta1=0.95, beta2=0.95):
    """dL/dtheta of L = sum_{t = 0..T} f(x_t, t) for the unroll x_{t+1} = x_t + net(grad f(x_t, t)) from the zero state,
    restated in torch float64.  x0: the flat concatenation of every variable the ONE coordinate-wise net steps.  second: the
    graph is kept through g_t (second_derivatives=True); otherwise g_t is a constant.  cfg: an oracle NetConfig -- "cw" with
    identity or LogAndSign, or "rnnprop" (fc + ELU on the Adam-normalised inputs m^ / (sqrt(v^) + 1e-8), g / (sqrt(v^) +
    1e-8), tanh output; the square root's derivative is taken as 0 where v^ = 0, as the BPTT takes it)."""
    tp = {k: {v: torch.tensor(np.asarray(a, np.float64), requires_grad=True) for v, a in d.items()} for k, d in params.items()}
    x = torch.tensor(np.asarray(x0, np.float64).reshape(-1), requires_grad=True)
    n, H = x.numel(), 20
    st = [[torch.zeros(n, h, dtype=torch.float64), torch.zeros(n, h, dtype=torch.float64)] for h in cfg.layers]
    rn = cfg.kind == "rnnprop"
    m = v = torch.zeros(n, dtype=torch.float64)

    def cell(inp, h, c, p):
        z = torch.cat([inp, h], 1) @ p["w_gates"] + p["b_gates"]
        i, j, fg, o = torch.sigmoid(z[:, :H]), torch.tanh(z[:, H:2 * H]), torch.sigmoid(z[:, 2 * H:3 * H] + 1), torch.sigmoid(z[:, 3 * H:])
        cn = fg * c + i * j
        return torch.tanh(cn) * o, cn

    loss = 0
    for t in range(T):
        fx = f(x, t)
        g = torch.autograd.grad(fx, x, create_graph=second, retain_graph=True)[0]
        if not second:
            g = g.detach()
        loss = loss + fx
        if rn:
            k = step0 + t
            m = beta1 * m + (1.0 - beta1) * g
            v = beta2 * v + (1.0 - beta2) * g * g
            mh, vh = m / (1.0 - beta1 ** k), v / (1.0 - beta2 ** k)
            pos = vh > 0
            den = torch.where(pos, torch.sqrt(torch.where(pos, vh, torch.ones_like(vh))), torch.zeros_like(vh)) + 1e-8
            a = torch.stack([mh / den, g / den], 1) @ tp["input_projection"]["w"] + tp["input_projection"]["b"]
            a = torch.where(a > 0, a, torch.exp(torch.clamp(a, max=0.0)) - 1.0)
        elif cfg.preprocess_name == "LogAndSign":
            gf = g.reshape(-1, 1)
            kk = float(cfg.preprocess_options["k"])
            eps = float(np.finfo(np.float32).eps)
            a = torch.cat([torch.clamp(torch.log(gf.abs() + eps) / kk, min=-1.0), torch.clamp(gf * float(np.exp(kk)), -1.0, 1.0)], 1)
        else:
            a = g.reshape(-1, 1)
        out = a
        for li in range(len(cfg.layers)):
            h, c = cell(out, st[li][0], st[li][1], tp["lstm_%d" % (li + 1)])
            st[li] = [h, c]
            out = h
        d = out @ tp["linear"]["w"] + tp["linear"]["b"]
        d = (torch.tanh(d) if cfg.tanh_output else d) * cfg.scale
        x = x + d.reshape(x.shape)
    loss = loss + f(x, T)
    loss.backward()
    return {k: {v: t.grad.numpy() for v, t in d.items()} for k, d in tp.items()}


class HvpOracleEngine(OracleEngine):
    """OracleEngine with the MLP Hessian-vector product (HipEngine.mlp_hvp's contract) in float32 torch."""

    def mlp_hvp(self, d, indices, ws, us, outs):
        self.calls.append("mlp_hvp")
        self._dense(*ws, *us, *outs)
        hidden = (d.n_hidden,) if hasattr(d, "n_hidden") else tuple(d.hidden)
        shapes = shapes_of(d.n_in, hidden, d.n_out)
        assert len(ws) == len(us) == len(outs) == len(shapes)
        res = hvp([w.numpy().reshape(sh) for w, sh in zip(ws, shapes)], [u.numpy().reshape(sh) for u, sh in zip(us, shapes)],
                  d.images.numpy(), d.labels.numpy(), indices.numpy(), "sigmoid" if d.activation == 0 else "relu",
                  dtype=torch.float32)
        for o, r in zip(outs, res):
            o.copy_(torch.from_numpy(np.ascontiguousarray(r, np.float32)).view_as(o))
