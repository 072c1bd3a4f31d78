"""The Twin-L2O evaluation unroll restated in torch (float64 or float32) -- the oracle of tests/test_twin*.py.  Not a test
module.  Written from the formulas of the reference's ``Model_Free_L2O/L2O-Minimax/Twin-L2O.py`` (cited by line), on
``torch.nn.LSTMCell`` itself: the cell is the reference's own arithmetic.

One function per piece: ``gradients`` / ``objective`` (ToyLoss, lines 612-651), ``make_net`` / ``iteration`` (Optimizer
lines 676-719, do_fit lines 152-251), ``run`` (do_fit with should_train=False), ``schedule`` (line 94 and the tests of lines
201 / 241), ``curve_info`` (lines 140-150, 338-342), ``distances`` (lines 347-376).  ``TorchTwinEngine.twin_unroll`` runs
the float32 restatement behind the engine seam of ``open_l2o_amd.twin``.
"""
import math

import numpy as np
import torch

NAMES = ("recurs.weight_ih", "recurs.weight_hh", "recurs.bias_ih", "recurs.bias_hh",
         "recurs2.weight_ih", "recurs2.weight_hh", "recurs2.bias_ih", "recurs2.bias_hh", "output.weight", "output.bias")


def objective(kind, data, u, v):
    """f(u, v) per instance (ToyLoss.get_loss).  u, v [n, dim]; data [n, 2] or [n, dim, dim]."""
    if kind == 4:
        return (u * torch.matmul(data, v.unsqueeze(-1)).squeeze(-1)).sum(dim=1)
    a, b = data[:, 0:1], data[:, 1:2]
    if kind == 1:
        f = a * u * u - b * v * v
    elif kind == 2:
        f = a * u * u - b * v * v + 2 * v * u
    else:
        f = (-1) * b * v * torch.sin(math.pi * u * a)
    return f.sum(dim=1)


def gradients(kind, data, u, v):
    """(df/du, df/dv), the closed forms of ToyLoss.get_grad_u / get_grad_v."""
    if kind == 4:
        return (torch.matmul(data, v.unsqueeze(-1)).squeeze(-1),
                torch.matmul(data.transpose(1, 2), u.unsqueeze(-1)).squeeze(-1))
    a, b = data[:, 0:1], data[:, 1:2]
    if kind == 1:
        return 2 * u * a, (-2) * b * v
    if kind == 2:
        return 2 * u * a + 2 * v, (-2) * b * v + 2 * u
    return (-1) * b * v * torch.cos(a * math.pi * u) * a * math.pi, (-1) * b * torch.sin(a * math.pi * u)


class Net(object):
    """The reference's Optimizer on torch.nn.LSTMCell, in `dtype`, from a dict of arrays under its parameter names."""

    def __init__(self, params, dtype):
        w = {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in params.items()}
        H, n_in = w["recurs.weight_hh"].shape[1], w["recurs.weight_ih"].shape[1]
        self.hidden, self.n_in = H, n_in
        self.recurs = torch.nn.LSTMCell(n_in, H, dtype=dtype)
        self.recurs2 = torch.nn.LSTMCell(H, H, dtype=dtype)
        self.output = torch.nn.Linear(H, 1, dtype=dtype)
        with torch.no_grad():
            for mod, pre in ((self.recurs, "recurs."), (self.recurs2, "recurs2.")):
                for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                    getattr(mod, n).copy_(w[pre + n])
            self.output.weight.copy_(w["output.weight"].reshape(1, H))
            self.output.bias.copy_(w["output.bias"].reshape(1))

    def __call__(self, g, s, state):
        """(delta [rows], new state) of one call on rows [g, s]; state = [h1, c1, h2, c2], each [rows, H]."""
        x = torch.cat((g, s), 1) if self.n_in == 2 else g
        h1, c1 = self.recurs(x, (state[0], state[1]))
        h2, c2 = self.recurs2(h1, (state[2], state[3]))
        return self.output(h2)[:, 0], [h1, c1, h2, c2]


def schedule(optim_it):
    """(n_sign, sche_lr in float64): the reference's expression; iteration k takes the sign rule iff k < 0.2 * optim_it."""
    sche_lr = list(np.arange(1e-4, 1e-1, (1e-1 - 1e-4) / int(0.2 * optim_it)))
    return sum(1 for k in range(1, optim_it + 1) if k < 0.2 * optim_it), sche_lr


def iteration(k, kind, data, nets, u, v, states, rescale, out_mul, n_sign, sign_lr):
    """Iteration k (1-based) in place of do_fit's loop body: returns (u, v, delta [n, dim]); states[which] is replaced."""
    which = (k + 1) % 2                                    # odd k: 0 = min, even k: 1 = max
    n, dim = u.shape
    gu, gv = gradients(kind, data, u, v)
    g, s = (gu, gv) if which == 0 else (gv, gu)
    st = [rescale * t for t in states[which]]
    delta, states[which] = nets[which](g.reshape(n * dim, 1), s.reshape(n * dim, 1), st)
    delta = delta.reshape(n, dim)
    step = torch.sign(delta) * sign_lr[k - 1] if k <= n_sign else delta * out_mul
    if which == 0:
        u = u + step
    else:
        v = v + step
    return u, v, delta


def run(dtype, kind, dim, data, params_min, params_max, sign_lr, n_sign, theta0, states, iter0, n_iter, rescale, out_mul):
    """Iterations iter0 .. iter0 + n_iter - 1 in `dtype` from float32 inputs.  Returns a dict of NumPy arrays in `dtype`:
    theta [n, 2, dim], states ([4, H, rows] x 2), curve [n, n_iter + 1, 2 dim], f [n, n_iter], delta [n, n_iter, dim]."""
    with torch.no_grad():
        nets = (Net(params_min, dtype), Net(params_max, dtype))
        data = torch.as_tensor(np.asarray(data, dtype=np.float32)).to(dtype)
        theta0 = torch.as_tensor(np.asarray(theta0, dtype=np.float32)).to(dtype)
        n = theta0.shape[0]
        u, v = theta0[:, 0].clone(), theta0[:, 1].clone()
        st = [[torch.as_tensor(np.asarray(s, dtype=np.float32)[j]).to(dtype).T.contiguous() for j in range(4)] for s in states]
        lr = [float(np.float32(x)) for x in sign_lr]
        rescale, out_mul = float(np.float32(rescale)), float(np.float32(out_mul))
        curve, fs, deltas = [torch.cat((u, v), 1)], [], []
        for k in range(iter0, iter0 + n_iter):
            u, v, dl = iteration(k, kind, data, nets, u, v, st, rescale, out_mul, n_sign, lr)
            curve.append(torch.cat((u, v), 1))
            fs.append(objective(kind, data, u, v))
            deltas.append(dl)
        return dict(theta=torch.stack((u, v), 1).numpy(),
                    states=tuple(torch.stack([t.T for t in s]).contiguous().numpy() for s in st),
                    curve=torch.stack(curve, 1).numpy(),
                    f=torch.stack(fs, 1).numpy() if fs else np.zeros((n, 0)),
                    delta=torch.stack(deltas, 1).numpy() if deltas else np.zeros((n, 0, dim)))


def curve_info(curve, optim_it, dim):
    """The reference's test-mode array, filled as its loop fills it (lines 338-342), from curve [n, optim_it + 1, 2 dim]."""
    info = np.zeros((curve.shape[0], optim_it // 2 + 1, 2 * dim))
    info[:, 0] = curve[:, 0]
    for iteration_ in range(1, optim_it + 1):
        if iteration_ % 2 == 1 and iteration_ // 2 + 1 < info.shape[1]:
            info[:, iteration_ // 2 + 1, :dim] = curve[:, iteration_, :dim]
        elif iteration_ % 2 == 0:
            info[:, iteration_ // 2, dim:] = curve[:, iteration_, dim:]
    return info


def distances(kind, data, curve, dim):
    """(all_distance_ever_u, all_distance_ever_v) [n, n_iter] by the reference's code, the seesaw's search loop included."""
    curve = np.asarray(curve, dtype=np.float32)
    n, T = curve.shape[0], curve.shape[1] - 1
    du, dv = np.zeros((n, T), np.float32), np.zeros((n, T), np.float32)
    for i in range(n):
        for t in range(T):
            sol_u, sol_v = curve[i, t + 1, :dim], curve[i, t + 1, dim:]
            dv[i, t] = np.sum(np.abs(sol_v))
            if kind != 3:
                du[i, t] = np.sum(np.abs(sol_u))
                continue
            a = np.float32(data[i][0])
            best, initial, k = 100000, np.sum(np.abs(sol_u)), 0
            while True:
                gt = np.float32(k) / a
                dist = abs(np.sum(np.abs(sol_u)) - gt)
                if dist < best:
                    best = dist
                elif dist > initial:
                    break
                k = k + 1
            du[i, t] = best
    return du, dv


class TorchTwinEngine(object):
    """The engine seam of open_l2o_amd.twin on the float32 restatement (CPU tests of the host logic)."""

    name = "torch-twin"
    dtype = torch.float32

    def twin_unroll(self, nets, problem, run_, theta, states, record=()):
        kind, dim, data = problem
        n_iter = int(run_["n_iter"])
        r = run(self.dtype, kind, dim, data, nets[0][2], nets[1][2], run_["sign_lr"], run_["n_sign"], theta, states,
                run_["iter0"], n_iter, run_["rescale"], run_["out_mul"])
        return dict(theta=r["theta"].astype(np.float32), states=tuple(s.astype(np.float32) for s in r["states"]),
                    curve=np.ascontiguousarray(r["curve"][:, 1:].transpose(1, 0, 2)).astype(np.float32) if "curve" in record else None,
                    f=np.ascontiguousarray(r["f"].T).astype(np.float32) if "f" in record else None,
                    delta=np.ascontiguousarray(r["delta"].transpose(1, 0, 2)).astype(np.float32) if "delta" in record else None)
