"""Reference for networks.KernelDeepLSTM (one LSTM per convolution filter), restated in torch from the formulas: a variable
[kw, kh, c_in, c_out] is the [K = kw kh, N = c_in c_out] matrix it is in memory (row j = a kh + b, column n = ci c_out + co);
the LSTM of filter n reads the K gradients of its patch (identity) or their 2K LogAndSign features (column 2j:
max(log(|g| + eps) / k, -1), column 2j + 1: clip(g e^k, -1, 1)), runs Sonnet LSTM layers (gates i, j, f, o; forget bias 1)
and a Linear [H_L, K]; delta[j, n] = scale * out[n, j] (scale * tanh(out) with tanh_output).

Not a test module.  It holds the step and the unroll in any torch dtype, an oracle-backed engine with ``klstm_step`` /
``klstm_bwd_step`` in float32 torch (so that the host logic of the step path and of the BPTT runs in the CPU suite), and the
unroll of a graph with mixed nets (kernel nets and coordinate-wise nets) with its autograd meta-gradient."""
import types

import numpy as np
import torch

from oracle_engine import OracleEngine

EPS = float(np.finfo(np.float32).eps)


def cfg_of(net):
    """What the restatement needs to know about a networks.KernelDeepLSTM."""
    return types.SimpleNamespace(kind="kernel", kernel_shape=tuple(net.kernel_shape), layers=tuple(net.layers),
                                 logsign_k=(net.logsign_k if net._preprocess_name == "LogAndSign" else None),
                                 scale=float(net.scale), tanh_output=bool(net.tanh_output))


def kernel_cfg(kernel_shape, layers, logsign_k=None, scale=1.0, tanh_output=False):
    return types.SimpleNamespace(kind="kernel", kernel_shape=tuple(kernel_shape), layers=tuple(layers), logsign_k=logsign_k,
                                 scale=float(scale), tanh_output=bool(tanh_output))


def cw_cfg(layers, logsign_k=None, scale=1.0, tanh_output=False):
    """A coordinate-wise net: the kernel net of a 1 x 1 patch over a variable taken as [1, size]."""
    return types.SimpleNamespace(kind="cw", kernel_shape=(1, 1), layers=tuple(layers), logsign_k=logsign_k,
                                 scale=float(scale), tanh_output=bool(tanh_output))


def as_torch(params, dtype, requires_grad=False):
    return {m: {v: torch.tensor(np.asarray(a, np.float64), dtype=dtype, requires_grad=requires_grad) for v, a in d.items()}
            for m, d in params.items()}


def features(cfg, g_kn):
    """[K, N] gradients -> the [N, in] LSTM input."""
    x = g_kn.t()
    if cfg.logsign_k is None:
        return x
    k = float(cfg.logsign_k)
    log = torch.clamp(torch.log(x.abs() + EPS) / k, min=-1.0)
    sign = torch.clamp(x * float(np.exp(k)), -1.0, 1.0)
    return torch.stack([log, sign], 2).reshape(x.shape[0], -1)           # the pairs interleaved


def zero_state(cfg, N, dtype):
    return [(torch.zeros(N, H, dtype=dtype), torch.zeros(N, H, dtype=dtype)) for H in cfg.layers]


def step(cfg, p, g_kn, state, keep=None):
    """One step: (delta [K, N], new state [(h [N, H], c [N, H]) per layer]).  keep (a dict): the intermediates act_l, z_l,
    out, for the backward tests."""
    x = features(cfg, g_kn)
    new = []
    for l, (H, (h, c)) in enumerate(zip(cfg.layers, state)):
        pl = p["lstm_%d" % (l + 1)]
        act = torch.cat([x, h], 1)
        z = act @ pl["w_gates"] + pl["b_gates"]
        if keep is not None:
            keep.setdefault("act", []).append(act)
            keep.setdefault("z", []).append(z)
        i, j, f, o = z[:, :H], z[:, H:2 * H], z[:, 2 * H:3 * H], z[:, 3 * H:]
        cn = torch.sigmoid(f + 1.0) * c + torch.sigmoid(i) * torch.tanh(j)
        hn = torch.tanh(cn) * torch.sigmoid(o)
        new.append((hn, cn))
        x = hn
    out = x @ p["linear"]["w"] + p["linear"]["b"]
    if keep is not None:
        keep["out"], keep["h_last"] = out, x
    d = torch.tanh(out) if cfg.tanh_output else out
    return cfg.scale * d.t(), new


def unroll(cfg, params, gs, dtype):
    """T steps from the zero state on the gradient sequence gs [T][K, N]: (the deltas, the final state)."""
    p = as_torch(params, dtype)
    N = np.asarray(gs[0]).shape[1]
    st = zero_state(cfg, N, dtype)
    out = []
    for g in gs:
        d, st = step(cfg, p, torch.tensor(np.asarray(g, np.float64), dtype=dtype), st)
        out.append(d)
    return out, st


def state_to_buf(state):
    """[(h [N, H], c [N, H])] -> the unit-major buffer of l2o_klstm_state_floats (h [H][N] then c [H][N] per layer)."""
    return torch.cat([a.t().reshape(-1) for hc in state for a in hc])


def buf_to_state(buf, layers, N):
    out, off = [], 0
    for H in layers:
        out.append((buf[off:off + H * N].view(H, N).t(), buf[off + H * N:off + 2 * H * N].view(H, N).t()))
        off += 2 * H * N
    return out


def bwd_step(cfg, p, g_kn, state, dx_next, carry):
    """One BPTT step by autograd of the restated step, in the dtype of the arguments: dict(carry=[(dh, dc)], act, dz, h_last,
    dd) -- the contract of l2o_klstm_bwd_step.  carry: [(dL/dh_l(t), dL/dc_l(t))] from step t + 1."""
    st = [(h.detach().clone().requires_grad_(True), c.detach().clone().requires_grad_(True)) for h, c in state]
    keep = {}
    delta, new = step(cfg, p, g_kn, st, keep)
    for z in keep["z"]:
        z.retain_grad()
    keep["out"].retain_grad()
    obj = (delta * dx_next).sum()
    for (hn, cn), (dh, dc) in zip(new, carry):
        obj = obj + (hn * dh).sum() + (cn * dc).sum()
    obj.backward()
    return dict(carry=[(h.grad, c.grad) for h, c in st], act=[a.detach() for a in keep["act"]],
                dz=[z.grad for z in keep["z"]], h_last=keep["h_last"].detach(), dd=keep["out"].grad)


class KernelOracleEngine(OracleEngine):
    """OracleEngine with HipEngine.klstm_step / klstm_bwd_step's contract in float32 torch."""

    def klstm_net(self, net):
        return None

    def klstm_step(self, net, g, st_in, st_out, x, N):
        self.calls.append("klstm_step")
        self._dense(g, st_in, st_out, x)
        cfg = cfg_of(net)
        K = net.output_size
        assert g.numel() == x.numel() == K * N and st_in.numel() == st_out.numel() == 2 * N * sum(cfg.layers)
        p = as_torch(net.variables, torch.float32)
        delta, new = step(cfg, p, g.view(K, N), buf_to_state(st_in, cfg.layers, N))
        st_out.copy_(state_to_buf(new))
        x.view(K, N).add_(delta)

    def klstm_bwd_step(self, net, io, N):
        self.calls.append("klstm_bwd_step")
        cfg = cfg_of(net)
        K = net.output_size
        p = as_torch(net.variables, torch.float32)
        assert io["carry_in"].data_ptr() != io["carry_out"].data_ptr()
        res = bwd_step(cfg, p, io["g"].view(K, N), buf_to_state(io["st_prev"], cfg.layers, N), io["dx_next"].view(K, N),
                       buf_to_state(io["carry_in"], cfg.layers, N))
        io["carry_out"].copy_(state_to_buf(res["carry"]))
        for l in range(len(cfg.layers)):
            io["act"][l].copy_(res["act"][l])
            io["dz"][l].copy_(res["dz"][l])
        io["h_last"].copy_(res["h_last"])
        io["dd"].copy_(res["dd"])


def graph_unroll(nets, assign, fg, x0, T, dtype=torch.float64, want_grad=False, drop_dd=None):
    """The unroll of a graph with mixed nets, restated: variable v (array x0[v]) is stepped by net assign[v] of
    nets = {key: (cfg, params)}, a kernel net on the variable as [K, N], a coordinate-wise one on it as [1, size];
    fg(xs, t) -> (f, [gradients]) is the optimizee on evaluation t (arrays in the dtype of xs).  x_{t+1} = x_t + delta_t from
    the zero state, fx[t] = f(x_t), t = 0..T.  Returns (fx [T + 1], x_T arrays) and, with want_grad, the first-order
    meta-gradient {key: {module: {variable: array}}} of sum_t fx[t]: the optimizee gradients are constants.
    drop_dd = (net key, t): that net's dd operand of step t, dL/d(Linear output), is zeroed (the tests' proof that the bound
    sees a missing term)."""
    npdt = np.float64 if dtype == torch.float64 else np.float32
    tp = {k: as_torch(p, dtype, requires_grad=want_grad) for k, (_, p) in nets.items()}
    xs = [torch.tensor(np.asarray(a, np.float64), dtype=dtype) for a in x0]
    shapes = []
    for v, a in enumerate(x0):
        cfg = nets[assign[v]][0]
        K = cfg.kernel_shape[0] * cfg.kernel_shape[1]
        shapes.append((K, int(np.asarray(a).size) // K))
    states = [zero_state(nets[assign[v]][0], shapes[v][1], dtype) for v in range(len(x0))]
    fx, loss = [], 0
    for t in range(T + 1):
        f, gs = fg([x.detach().numpy().reshape(np.asarray(a).shape).astype(npdt) for x, a in zip(xs, x0)], t)
        gs = [torch.tensor(np.asarray(g, np.float64), dtype=dtype).reshape(sh) for g, sh in zip(gs, shapes)]
        fx.append(float(f))
        if want_grad:                                        # f(x_t) to first order in the weights: g_t . x_t
            loss = loss + sum((g * x.reshape(sh)).sum() for g, x, sh in zip(gs, xs, shapes))
        if t == T:
            break
        for v in range(len(xs)):
            key = assign[v]
            cfg = nets[key][0]
            p = tp[key]
            delta, states[v] = step(cfg, p, gs[v], states[v])
            if drop_dd == (key, t):
                delta = delta.detach()
            xs[v] = (xs[v].reshape(shapes[v]) + delta).reshape(xs[v].shape)
    xT = [x.detach().numpy().reshape(np.asarray(a).shape) for x, a in zip(xs, x0)]
    if not want_grad:
        return np.asarray(fx), xT
    loss.backward()
    grads = {k: {m: {v: (np.zeros(a.shape) if a.grad is None else a.grad.numpy().astype(np.float64)) for v, a in d.items()}
                 for m, d in p.items()} for k, p in tp.items()}
    return np.asarray(fx), xT, grads
