"""The Twin-L2O meta-training restated in torch -- the oracle of tests/test_twin_train*.py.  Not a test module.  Written
from the reference's ``Model_Free_L2O/L2O-Minimax/Twin-L2O.py`` (cited by line) on ``TR.Net`` (``torch.nn.LSTMCell``): the
segment's loss is BUILT with the reference's detach points and differentiated by autograd -- no closed form is taken on
trust.

``segment`` builds one segment's graph (do_fit lines 152-426), ``segment_grad`` differentiates it (lines 287-296),
``closed_form_seed`` is the formula the kernels implement, ``get_index`` / ``sche_ratio`` are utils/metrics.py lines 18-38
and Twin-L2O.py lines 84-88, ``train_loop`` is do_fit(should_train=True) with ``torch.optim.Adam``, and
``TorchTwinTrainEngine`` puts the float32 autograd restatement behind the engine seam of ``open_l2o_amd.twin``.
"""
import math

import numpy as np
import torch

import twin_reference as TR

NAMES = TR.NAMES


def net_params(net):
    """The parameters of a TR.Net under the reference's names, in NAMES' order."""
    out = {}
    for mod, pre in ((net.recurs, "recurs."), (net.recurs2, "recurs2."), (net.output, "output.")):
        for n, p in mod.named_parameters():
            out[pre + n] = p
    return {k: out[k] for k in NAMES}


def segment(nets, kind, data, u, v, states, iter0, n_iter, n_sign, lr, rescale, out_mul, batch_size):
    """Iterations iter0 .. iter0 + n_iter - 1 with the graph of do_fit.  u, v [n, dim] and states[which] = [h1, c1, h2, c2]
    enter detached (lines 304-311).  Returns (reward [n]: the instance's batch_reward_min + batch_reward_max, u, v, states,
    points: the list of (u, v) after each iteration, fs, deltas: the list of the attached delta [n, dim])."""
    n, dim = u.shape
    states = [list(s) for s in states]
    reward = torch.zeros(n, dtype=u.dtype)
    loss_previous = torch.zeros(n, dtype=u.dtype)                          # line 312 (and 379-382)
    points, fs, deltas = [], [], []
    for k in range(iter0, iter0 + n_iter):
        which = (k + 1) % 2
        gu, gv = TR.gradients(kind, data, u.detach(), v.detach())          # lines 170-175 / 216-221: clone().detach()
        g, s = (gu, gv) if which == 0 else (gv, gu)
        st = [rescale * t for t in states[which]]                          # lines 184-186 / 226-228
        delta, states[which] = nets[which](g.reshape(n * dim, 1), s.reshape(n * dim, 1), st)
        delta = delta.reshape(n, dim)
        deltas.append(delta)
        step = torch.sign(delta) * lr[k - 1] if k <= n_sign else delta * out_mul    # lines 201-207: sign has derivative 0
        if which == 0:
            u = u + step
        else:
            v = v + step
        f = TR.objective(kind, data, u, v)
        loss_temp = f if which == 0 else (-1) * f                          # lines 385-389
        reward = reward + (loss_temp + loss_previous) / batch_size         # lines 391-400
        loss_previous = loss_temp.clone()                                  # line 402: keeps its graph
        if which == 0:                                                     # lines 405-426: the stepped variable is detached
            u = u.detach()
        else:
            v = v.detach()
        points.append(torch.cat((u, v), 1))
        fs.append(f.detach())
    return reward, u, v, states, points, fs, deltas


def segment_grad(dtype, kind, dim, data, params_min, params_max, sign_lr, n_sign, theta0, states, iter0, n_iter, rescale,
                 out_mul, batch_size=None, inst_weight=None):
    """One segment in `dtype` from float32 inputs, its loss and autograd's gradient.  Returns a dict of NumPy arrays: theta,
    states, curve [n, n_iter + 1, 2 dim], f, delta (as TR.run), loss, grads (min, max: {name: array}, zeros where autograd
    finds no path) and g_delta [n, n_iter, dim], d loss / d delta of every iteration."""
    nets = (TR.Net(params_min, dtype), TR.Net(params_max, dtype))
    data = torch.as_tensor(np.asarray(data, dtype=np.float32)).to(dtype)
    theta0 = torch.as_tensor(np.asarray(theta0, dtype=np.float32)).to(dtype)
    n = theta0.shape[0]
    batch_size = n if batch_size is None else batch_size
    u, v = theta0[:, 0].clone(), theta0[:, 1].clone()
    st = [[torch.as_tensor(np.asarray(s, dtype=np.float32)[j]).to(dtype).T.contiguous() for j in range(4)] for s in states]
    lr = [float(np.float32(x)) for x in sign_lr]
    rescale, out_mul = float(np.float32(rescale)), float(np.float32(out_mul))
    reward, u1, v1, st1, points, fs, deltas = segment(nets, kind, data, u, v, st, iter0, n_iter, n_sign, lr, rescale, out_mul,
                                                      batch_size)
    m = torch.ones(n, dtype=dtype) if inst_weight is None else torch.as_tensor(np.asarray(inst_weight, np.float32)).to(dtype)
    total = (reward * m).sum()
    ps = [net_params(nets[0]), net_params(nets[1])]
    flat = [p for d in ps for p in d.values()]
    got = torch.autograd.grad(total, flat + deltas, allow_unused=True)
    got = [torch.zeros_like(t) if g is None else g for g, t in zip(got, flat + deltas)]
    grads = tuple({k: got[i * len(NAMES) + j].numpy() for j, k in enumerate(NAMES)} for i in range(2))
    return dict(theta=torch.stack((u1, v1), 1).detach().numpy(),
                states=tuple(torch.stack([t.detach().T for t in s]).contiguous().numpy() for s in st1),
                curve=torch.stack([torch.cat((u, v), 1)] + points, 1).detach().numpy(),
                f=torch.stack(fs, 1).numpy(), delta=torch.stack(deltas, 1).detach().numpy(),
                loss=float(total.detach()), grads=grads, g_delta=torch.stack(got[len(flat):], 1).numpy())


def closed_form_seed(kind, data, curve, iter0, n_iter, n_sign, out_mul, batch_size, inst_weight=None):
    """g_delta [n, n_iter, dim] = w_k s_k out_mul (df / d own variable)(point after iteration k) m / batch_size for
    k > n_sign, else 0: s_k = +1 (min step) / -1 (max step), w_k = 2, 1 at the segment's last iteration.  float64; curve
    [n, n_iter + 1, 2 dim]."""
    data = torch.as_tensor(np.asarray(data, dtype=np.float32)).to(torch.float64)
    curve = torch.as_tensor(np.asarray(curve, dtype=np.float64))
    n, dim = curve.shape[0], curve.shape[2] // 2
    m = np.ones(n) if inst_weight is None else np.asarray(inst_weight, np.float64)
    out = np.zeros((n, n_iter, dim))
    for j in range(n_iter):
        k = iter0 + j
        if k <= n_sign:
            continue
        gu, gv = TR.gradients(kind, data, curve[:, j + 1, :dim], curve[:, j + 1, dim:])
        own, s_k = (gu, 1.0) if k % 2 == 1 else (gv, -1.0)
        w_k = 1.0 if j == n_iter - 1 else 2.0
        out[:, j] = w_k * s_k * out_mul * own.numpy() * m[:, None] / batch_size
    return out


def sche_ratio(epoch_index):
    """Twin-L2O.py lines 84-88."""
    if 0 <= epoch_index <= 80:
        return 0.2 + epoch_index/100
    else:
        return 1


def get_index(all_distance_ever1, iteration_index=-1, unroll_unit=-1, batch_data=None, ratio=0.8):
    """utils/metrics.py lines 18-38, statement by statement (a, b as Python floats of the float32 data, so that the sums are
    Python floats under every NumPy)."""
    result = []
    k = int(ratio * len(all_distance_ever1))
    curve_info = all_distance_ever1
    flag = iteration_index//10
    curve_v = curve_info[:, 0:flag * 2 * unroll_unit - 1, 1]
    curve_u = curve_info[:, 0:flag * 2 * unroll_unit - 1, 0]
    for i in range(len(curve_v)):
        a = float(batch_data[i, 0])
        b = float(batch_data[i, 1])
        grad_v = [(-1) * b * math.sin(a * math.pi * float(u)) for u in curve_u[i]]
        grad_v_squared = [d ** 2 for d in grad_v]
        result.append(sum(grad_v_squared))
    return sorted(range(len(result)), key=lambda i: result[i], reverse=True)[-k:]


def train_loop(kind, dim, data, params_min, params_max, meta_lr, optim_it, unroll_unit, theta0, states, rescale, out_mul=1.0,
               CL=False, epoch_index=0, adams=None, nets=None):
    """do_fit(should_train=True) on one batch in float32: the loop of lines 152-426 with ``total_loss.backward()`` and the two
    ``torch.optim.Adam`` of fit_optimizer (lines 481-482).  Returns a dict: params (min, max: {name: array}), steps (Adam's
    step counts), distances (v, u), curve_info [n, optim_it, 2 dim], weights (per segment: None or the 0/1 vector of the
    instances get_index picked) and nets / adams to continue with."""
    dtype = torch.float32
    if nets is None:
        nets = (TR.Net(params_min, dtype), TR.Net(params_max, dtype))
        adams = tuple(torch.optim.Adam(list(net_params(net).values()), lr=meta_lr) for net in nets)
    n_sign, sche = TR.schedule(optim_it)
    lr = [float(np.float32(x)) for x in sche]
    data_t = torch.as_tensor(np.asarray(data, dtype=np.float32))
    theta0 = torch.as_tensor(np.asarray(theta0, dtype=np.float32))
    n = theta0.shape[0]
    u, v = theta0[:, 0].clone(), theta0[:, 1].clone()
    st = [[torch.as_tensor(np.asarray(s, dtype=np.float32)[j]).T.contiguous() for j in range(4)] for s in states]
    rescale, out_mul = float(np.float32(rescale)), float(np.float32(out_mul))
    curve_info = np.zeros((n, optim_it, 2 * dim))
    weights, L, iter0 = [], 2 * unroll_unit, 1
    while iter0 <= optim_it:
        n_iter = L if iter0 + L - 1 <= optim_it else optim_it - iter0 + 1
        reward, u, v, st, points, _, _ = segment(nets, kind, data_t, u, v, st, iter0, n_iter, n_sign, lr, rescale, out_mul, n)
        pts = torch.stack(points, 1).detach().numpy()
        if n_iter == L:                                                    # line 253: iteration % (unroll_unit * 2) == 0
            curve_info[:, iter0 - 1:iter0 + L - 2] = pts[:, :L - 1]        # (line 344 stores an iteration after line 259 reads)
            for a in adams:
                a.zero_grad()
            if CL:
                index = get_index(curve_info, iteration_index=iter0 + L - 1, unroll_unit=unroll_unit, batch_data=data,
                                  ratio=sche_ratio(epoch_index))
                m = np.zeros(n, np.float32)
                for b_temp in index:
                    m[b_temp] += 1
                weights.append(m)
                if len(index) > 0:
                    (reward * torch.as_tensor(m)).sum().backward()
                    for a in adams:
                        a.step()
            else:
                weights.append(None)
                reward.sum().backward()
                for a in adams:
                    a.step()
        curve_info[:, iter0 - 1:iter0 - 1 + n_iter] = pts
        u, v = u.detach(), v.detach()                                      # lines 304-311
        st = [[t.detach() for t in s] for s in st]
        iter0 += n_iter
    curve = np.concatenate([np.zeros((n, 1, 2 * dim)), curve_info], axis=1)
    du, dv = TR.distances(kind, np.asarray(data), curve, dim)
    return dict(params=tuple({k: p.detach().numpy().copy() for k, p in net_params(net).items()} for net in nets),
                steps=tuple(int(next(iter(a.state.values()))["step"]) if a.state else 0 for a in adams),
                distances=(dv, du), curve_info=curve_info, weights=weights, nets=nets, adams=adams)


class TorchTwinTrainEngine(TR.TorchTwinEngine):
    """TR.TorchTwinEngine with the segment's forward and backward of the meta-training: float32 autograd on the CPU."""

    name = "torch-twin-train"

    def twin_segment_forward(self, nets, problem, run_, theta, states, loss_scale):
        out = self.twin_unroll(nets, problem, run_, theta, states, record=("curve", "f", "delta"))
        return out, (nets, problem, dict(run_), np.array(theta, np.float32), tuple(np.array(s, np.float32) for s in states),
                     loss_scale)

    def twin_segment_backward(self, handle, inst_weight=None):
        nets, (kind, dim, data), run_, theta, states, loss_scale = handle
        r = segment_grad(self.dtype, kind, dim, data, nets[0][2], nets[1][2], run_["sign_lr"], run_["n_sign"], theta, states,
                         run_["iter0"], int(run_["n_iter"]), run_["rescale"], run_["out_mul"], batch_size=1.0 / loss_scale,
                         inst_weight=inst_weight)
        return tuple({k: np.asarray(v, np.float32).copy() for k, v in g.items()} for g in r["grads"])

    def twin_segment_grad(self, nets, problem, run_, theta, states, loss_scale, inst_weight=None):
        res, handle = self.twin_segment_forward(nets, problem, run_, theta, states, loss_scale)
        return res, self.twin_segment_backward(handle, inst_weight)
