"""Shared helpers for the parity tests (oracle <-> HIP path)."""
import copy

import numpy as np

import oracle as O
from open_l2o_amd import _abi
from open_l2o_amd._engine import NetSpec, ProblemDesc

ORACLE_CFGS = {"dm": O.DM_IDENTITY, "dm_logsign": O.DM_LOGSIGN, "rnnprop": O.RNNPROP}


def spec_of(cfg):
    """oracle NetConfig -> engine NetSpec."""
    if cfg.kind == "rnnprop":
        return NetSpec(_abi.NET_RNNPROP, _abi.PRE_FC_ELU, tuple(cfg.layers), cfg.scale, cfg.tanh_output)
    if cfg.preprocess_name == "LogAndSign":
        return NetSpec(_abi.NET_CW, _abi.PRE_LOGSIGN, tuple(cfg.layers), cfg.scale, cfg.tanh_output,
                       logsign_k=cfg.preprocess_options["k"])
    return NetSpec(_abi.NET_CW, _abi.PRE_IDENTITY, tuple(cfg.layers), cfg.scale, cfg.tanh_output)


def make_params(cfg, seed, trained_like=False):
    """Sonnet-default weights; ``trained_like`` shrinks the output Linear (a freshly
    initialised net takes O(1) steps and the trajectory is violently chaotic; a trained
    optimizer takes small steps)."""
    rng = np.random.default_rng(seed)
    p = O.init_net_params(cfg, rng)
    # non-zero biases so that every bias path is exercised
    for k in p:
        for v in p[k]:
            if v.startswith("b"):
                p[k][v] = (rng.standard_normal(p[k][v].shape) * 0.1).astype(np.float32)
    if trained_like:
        p["linear"]["w"] = (p["linear"]["w"] * 0.1).astype(np.float32)
        p["linear"]["b"] = (p["linear"]["b"] * 0.1).astype(np.float32)
    return p


def random_state(cfg, n, seed, scale=0.5):
    rng = np.random.default_rng(seed)
    return tuple(((rng.standard_normal((n, H)) * scale).astype(np.float32),
                  (rng.standard_normal((n, H)) * scale).astype(np.float32)) for H in cfg.layers)


def make_problem(kind, B, D, seed, M=None, stddev=None):
    """Returns (oracle problem, x0, dict of arrays for the device desc)."""
    rng = np.random.default_rng(seed)
    if kind == "quadratic":
        p, x = O.Quadratic.sample(rng, B, D, stddev=0.01 if stddev is None else stddev)
        arrays = dict(kind=_abi.PROB_QUADRATIC, W=p.w, y=p.y, M=D)
    elif kind == "lasso":
        p, x = O.Lasso.sample(rng, B, D, stddev=0.01 if stddev is None else stddev, l=0.1, num_rows=M)
        arrays = dict(kind=_abi.PROB_LASSO, W=p.w, y=p.y[..., 0], M=p.w.shape[1], l1=p.l)
    elif kind == "rastrigin":
        p, x = O.Rastrigin.sample(rng, B, D, stddev=1 if stddev is None else stddev)
        arrays = dict(kind=_abi.PROB_RASTRIGIN, W=p.A, y=p.B[..., 0], C=p.C[..., 0], M=D, alpha=p.alpha)
    elif kind == "square_cos":
        p, x = O.SquareCos.sample(rng, B, D, stddev=0.01 if stddev is None else stddev)
        arrays = dict(kind=_abi.PROB_SQUARE_COS, W=p.w, y=p.y, C=p.wcos.sum(axis=1), M=D, alpha=10.0)
    else:
        raise ValueError(kind)
    return p, x, arrays


def device_problem(eng, arrays, B, D, B_global=None, x_scale=None):
    return ProblemDesc(kind=arrays["kind"], B_local=B, B_global=B if B_global is None else B_global, D=D,
                       M=arrays.get("M", 0), l1=arrays.get("l1", 0.0), alpha=arrays.get("alpha", 0.0),
                       W=eng.tensor(arrays["W"]) if "W" in arrays else None,
                       y=eng.tensor(arrays["y"]) if "y" in arrays else None,
                       C=eng.tensor(arrays["C"]) if "C" in arrays else None,
                       x_scale=None if x_scale is None else eng.tensor(x_scale),
                       w_shared=bool(arrays.get("w_shared", False)))


def as_float64(prob):
    """A copy of an oracle problem (Quadratic, Lasso, Rastrigin, SquareCos) with float64 arrays."""
    p = copy.copy(prob)
    for k, v in vars(prob).items():
        if isinstance(v, np.ndarray):
            setattr(p, k, v.astype(np.float64))
    return p


def oracle_meta_grad(cfg, params, prob, x0, state0, T, m0=None, v0=None, step0=1, beta1=0.95, beta2=0.95):
    """The meta-gradient of ONE unroll from any starting point, by the oracle's forward and its hand-derived BPTT
    (oracle.net_bwd_step); float64 when params / x0 / the problem are.  ``prob``: an oracle problem (prob.f / prob.grad,
    the same at every step), or ``fg(x, t) -> (f, g)``, an optimizee that changes per step (a minibatch per evaluation,
    t = 0..T; mnist_fg).  x0 is shaped as ``prob`` expects it -- for several variables stepped by one coordinate-wise net
    the flat concatenation of all of them (the BPTT is the same over the concatenation) --, state0 the net state before
    step 0, m0 / v0 RNNProp's carried moments (zeros: None), step0 the fed `step`.
    Returns (grads {module: {variable: array}} of L = sum_{t=0..T} f(x_t), end) with end = dict(x, state, m, v, loss):
    what the harness' `update` carries into the next unroll."""
    fg = (lambda x, t: (prob.f(x), prob.grad(x))) if hasattr(prob, "grad") else prob
    dt = x0.dtype.type
    rn = cfg.kind == "rnnprop"
    x, state = x0.copy(), state0
    m = None if not rn else (np.zeros_like(x0) if m0 is None else np.asarray(m0, x0.dtype).reshape(x0.shape).copy())
    v = None if not rn else (np.zeros_like(x0) if v0 is None else np.asarray(v0, x0.dtype).reshape(x0.shape).copy())
    hist = []
    loss = dt(0)
    for t in range(T):
        f, g = fg(x, t)
        loss = loss + f
        if rn:
            (mt, gt), m, v = O.rnnprop_inputs(g, m, v, step0 + t, beta1, beta2)
            inputs = (mt.reshape(-1), gt.reshape(-1))
        else:
            inputs = g.reshape(-1)
        hist.append((inputs, state, g))
        delta, state = O.net_apply(cfg, params, inputs, state)
        x = x + delta.reshape(x.shape)
    f, G = fg(x, T)
    loss = loss + f
    G = G.reshape(-1)
    N = x0.size
    carry = tuple(np.zeros((N, 20), x0.dtype) for _ in range(4))
    grads = {}

    def add(mod, var, val):
        grads.setdefault(mod, {})
        grads[mod][var] = val if var not in grads[mod] else grads[mod][var] + val

    for t in reversed(range(T)):
        inputs, st_prev, g = hist[t]
        carry, rows = O.net_bwd_step(cfg, params, inputs, st_prev, G, carry)
        add("lstm_1", "w_gates", rows["act1"].T @ rows["dz1"])
        add("lstm_1", "b_gates", rows["dz1"].sum(0))
        add("lstm_2", "w_gates", rows["act2"].T @ rows["dz2"])
        add("lstm_2", "b_gates", rows["dz2"].sum(0))
        add("linear", "w", rows["h2"].T @ rows["dd"][:, None])
        add("linear", "b", rows["dd"].sum(keepdims=True))
        if rn:
            add("input_projection", "w", rows["feats"].T @ rows["du"])
            add("input_projection", "b", rows["du"].sum(0))
        G = G + g.reshape(-1)
    return grads, dict(x=x, state=state, m=m, v=v, loss=loss)


def mnist_fg(mlp, shapes, idx, scales=None):
    """``fg(x, t)`` of oracle_meta_grad over an O.MnistMLP (fg / fg_deep; float64 when x is): x is the flat
    concatenation of the optimizee's variables, split by ``shapes`` in the graph's order; evaluation t (step t, and t = T
    for the gradient at x_T) uses minibatch row idx[t]; with per-coordinate scales (one array per variable, the train
    forks' x-scale feed) it returns f(x * s) and s * grad f(x * s)."""
    sizes = [int(np.prod(sh)) for sh in shapes]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
    s = None if scales is None else np.concatenate([np.asarray(a, np.float64).reshape(-1) for a in scales])

    def fg(x, t):
        sc = None if s is None else s.astype(x.dtype)
        xs = x if sc is None else x * sc
        vs = [xs[offs[i]:offs[i + 1]].reshape(sh) for i, sh in enumerate(shapes)]
        f, grads = mlp.fg(vs, np.asarray(idx[t]))
        g = np.concatenate([a.reshape(-1) for a in grads])
        return f, (g if sc is None else g * sc)
    return fg


def block_errors(got, want):
    """{(module, variable): max |got - want| / max |want|} over the weight-gradient blocks of ``want``
    ({module: {variable: array}}); ``got`` is keyed either the same way or by (module, variable)."""
    out = {}
    for mod in want:
        for var, w in want[mod].items():
            g = got[(mod, var)] if (mod, var) in got else got[mod][var]
            g = np.asarray(g, np.float64).reshape(w.shape)
            out[(mod, var)] = float(np.abs(g - w).max()) / max(float(np.abs(w).max()), 1e-30)
    return out


def rel_err(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-30)))


def max_abs(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


import contextlib


@contextlib.contextmanager
def lib_option(opt, value):
    """Set a libl2o_hip option (l2o_set_option) for the duration of a with-block."""
    from open_l2o_amd import _abi
    old = _abi.set_option(opt, value)
    try:
        yield
    finally:
        _abi.set_option(opt, old)
