"""Twin-L2O: the reference's model-free minimax optimizer (``Model_Free_L2O/L2O-Minimax/Twin-L2O.py``), its evaluation
(``mode: "test"``) unroll.

Two per-coordinate two-layer LSTM optimizers -- one steps the min variable ``u``, one the max variable ``v`` -- alternate
over an analytic saddle objective; every coordinate of every problem instance shares the two networks.  The reference calls
two ``nn.LSTMCell`` per iteration per instance from Python; here all iterations of all instances are ONE launch of
``l2o_twin_unroll`` (``libl2o_hip.so``, ``csrc/l2o_twin.h``).  Meta-training of the twin networks is not built.

Objectives (``params["loss"]``; ``u = theta_min``, ``v = theta_max``): 1 saddle ``a u^2 - b v^2``, 2 rotated saddle
``a u^2 - b v^2 + 2 u v``, 3 seesaw ``-b v sin(a pi u)`` (all with dim 1), 4 matrix game ``u^T A v`` (dim >= 1).

One run of ``optim_it`` iterations, k = 1 ... optim_it: odd k is a min step (network "min" on the row ``[df/du, df/dv]``),
even k a max step (network "max" on ``[df/dv, df/du]``), both gradients at the current point; a network's own
``(h1, c1, h2, c2)`` are multiplied by ``rescale`` before its step and replaced by it; ``delta = output(h2')`` is ADDED:
``sign(delta) * sche_lr[k - 1]`` while ``k < 0.2 optim_it``, ``delta * out_mul`` after that.

Where the reference cannot be followed literally:

* it allocates the initial states ``[batch, H]`` but feeds rows ``[batch * dim]``, and its ``curve_info`` has two columns:
  with ``dim`` > 1 neither works as written.  Here there is one state row per coordinate and ``2 dim`` curve columns.
* ``preproc=True`` builds a 2-column input that is then concatenated with ``second`` for an ``LSTMCell(2, H)``: it cannot
  run in the reference.  ``Optimizer(preproc=True)`` raises ``NotImplementedError``.
* ``optim_it < 5`` divides by zero in ``sche_lr``: ``ValueError``.
"""
from __future__ import annotations

import collections
import os

import numpy as np
import torch

from . import _engine

SADDLE, ROTATED_SADDLE, SEESAW, MATRIX_GAME = 1, 2, 3, 4
PARAM_NAMES = ("recurs.weight_ih", "recurs.weight_hh", "recurs.bias_ih", "recurs.bias_hh",
               "recurs2.weight_ih", "recurs2.weight_hh", "recurs2.bias_ih", "recurs2.bias_hh",
               "output.weight", "output.bias")


# ---------------------------------------------------------------------------------------------------------
# problems
# ---------------------------------------------------------------------------------------------------------
class Problem(object):
    """n_inst instances of one objective.  data: kinds 1-3 float32 [n_inst, 2] (a, b); kind 4 [n_inst, dim, dim]."""

    def __init__(self, kind, data, dim=1):
        kind, dim = int(kind), int(dim)
        if kind not in (SADDLE, ROTATED_SADDLE, SEESAW, MATRIX_GAME):
            raise ValueError("twin: loss %r is not one of 1 (saddle), 2 (rotated saddle), 3 (seesaw), 4 (matrix game)" % (kind,))
        if dim < 1:
            raise ValueError("twin: dim %d" % dim)
        if kind != MATRIX_GAME and dim != 1:
            raise ValueError("twin: the saddle, rotated-saddle and seesaw objectives have dim = 1 (got %d); only the matrix "
                             "game has dim >= 1" % dim)
        if isinstance(data, (str, os.PathLike)):
            data = np.loadtxt(data, ndmin=2)                 # the reference's text format: one instance per line
        data = np.asarray(data, dtype=np.float32)
        if kind == MATRIX_GAME:
            data = data.reshape(-1, dim, dim)                # as fit_optimizer / the test mode reshape the rows
        else:
            if data.ndim != 2 or data.shape[1] != 2:
                raise ValueError("twin: data of the scalar objectives is [n, 2] = a, b (got %r)" % (data.shape,))
        if data.shape[0] < 1:
            raise ValueError("twin: no instances")
        self.kind, self.dim, self.data = kind, dim, np.ascontiguousarray(data)

    @property
    def n_inst(self):
        return int(self.data.shape[0])

    def take(self, index):
        """The instances data[index] (any NumPy index that keeps the first axis)."""
        return Problem(self.kind, self.data[index], self.dim)


def problem(loss, data, dim=1):
    """The objective the reference's ``params["loss"]`` (1-4) names."""
    return Problem(loss, data, dim)


def saddle(data):
    return Problem(SADDLE, data)


def rotated_saddle(data):
    return Problem(ROTATED_SADDLE, data)


def seesaw(data):
    return Problem(SEESAW, data)


def matrix_game(data, dim):
    return Problem(MATRIX_GAME, data, dim)


# ---------------------------------------------------------------------------------------------------------
# networks
# ---------------------------------------------------------------------------------------------------------
class Optimizer(object):
    """The reference's ``Optimizer``: ``recurs = LSTMCell(2 if use_second else 1, H)``, ``recurs2 = LSTMCell(H, H)``,
    ``output = Linear(H, 1)``, the parameters under the reference's names (float32 arrays in ``self.params``).  The default
    initialisation is torch's, U(-1/sqrt(H), 1/sqrt(H)), from a generator seeded by `seed`."""

    def __init__(self, hidden_size=50, use_second=True, preproc=False, seed=None):
        if preproc:
            raise NotImplementedError("twin.Optimizer(preproc=True): the reference's preprocessing builds a 2-column input "
                                      "and then concatenates `second` to it for an LSTMCell(2, H); it cannot run there, so "
                                      "there is nothing to restate")
        self.hidden_size, self.use_second, self.preproc = int(hidden_size), bool(use_second), False
        if self.hidden_size < 1:
            raise ValueError("twin.Optimizer: hidden_size %d" % self.hidden_size)
        gen = torch.Generator()
        if seed is None:
            gen.seed()
        else:
            gen.manual_seed(int(seed))
        bound = 1.0 / np.sqrt(self.hidden_size)
        self.params = collections.OrderedDict(
            (name, ((torch.rand(shape, generator=gen, dtype=torch.float32) * 2.0 - 1.0) * bound).numpy())
            for name, shape in self.shapes().items())

    @property
    def n_in(self):
        return 2 if self.use_second else 1

    def shapes(self):
        H = self.hidden_size
        return collections.OrderedDict((
            ("recurs.weight_ih", (4 * H, self.n_in)), ("recurs.weight_hh", (4 * H, H)), ("recurs.bias_ih", (4 * H,)),
            ("recurs.bias_hh", (4 * H,)), ("recurs2.weight_ih", (4 * H, H)), ("recurs2.weight_hh", (4 * H, H)),
            ("recurs2.bias_ih", (4 * H,)), ("recurs2.bias_hh", (4 * H,)), ("output.weight", (1, H)), ("output.bias", (1,))))

    def state_dict(self):
        return collections.OrderedDict((k, torch.from_numpy(v.copy())) for k, v in self.params.items())

    def load_state_dict(self, sd):
        """A state dict under the reference's parameter names (what ``torch.load`` gives for its ``bestmin.pth``)."""
        shapes = self.shapes()
        if set(sd.keys()) != set(shapes):
            raise KeyError("twin.Optimizer.load_state_dict: keys %s, expected %s" % (sorted(sd.keys()), sorted(shapes)))
        new = collections.OrderedDict()
        for name, shape in shapes.items():
            v = sd[name]
            a = np.ascontiguousarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v, dtype=np.float32)
            if a.shape != tuple(shape):
                raise ValueError("twin.Optimizer.load_state_dict: %s is %r, expected %r" % (name, a.shape, tuple(shape)))
            new[name] = a.copy()
        self.params = new
        return self


# ---------------------------------------------------------------------------------------------------------
# the run
# ---------------------------------------------------------------------------------------------------------
def schedule(optim_it):
    """(n_sign, sign_lr): iterations k <= n_sign (the reference's ``iteration < 0.2 * optim_it``) move by
    ``sign(delta) * sign_lr[k - 1]``; sign_lr is the reference's ``sche_lr`` -- its NumPy expression in float64 -- cast to
    float32."""
    optim_it = int(optim_it)
    if optim_it < 5:
        raise ValueError("twin: optim_it = %d: the reference's step schedule divides by int(0.2 * optim_it) = 0; "
                         "optim_it >= 5" % optim_it)
    sche_lr = np.arange(1e-4, 1e-1, (1e-1 - 1e-4) / int(0.2 * optim_it))
    n_sign = sum(1 for k in range(1, optim_it + 1) if k < 0.2 * optim_it)
    assert n_sign <= len(sche_lr)
    return n_sign, sche_lr.astype(np.float32)


class Result(object):
    """What ``unroll`` returns: theta [n_inst, 2, dim], states (min, max: [4, H, n_inst dim] = h1, c1, h2, c2), curve
    [n_inst, n_iter + 1, 2 dim] (row 0 the start, row j the point after iteration iter0 + j - 1: u then v), f
    [n_inst, n_iter], delta [n_inst, n_iter, dim]; an array that was not recorded is None."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def draw_start(prob, opt_min, opt_max, seed=None):
    """theta0 and the two initial states drawn as the reference draws them: u, v uniform in (-0.5, 0.5)
    (``0.5 * (-1 + 2 * rand)``), the states N(0, 0.01^2) -- one state row per coordinate."""
    gen = torch.Generator()
    if seed is None:
        gen.seed()
    else:
        gen.manual_seed(int(seed))
    rows = prob.n_inst * prob.dim
    theta0 = (0.5 * (-1.0 + 2.0 * torch.rand((prob.n_inst, 2, prob.dim), generator=gen, dtype=torch.float32))).numpy()
    states = tuple((torch.randn((4, o.hidden_size, rows), generator=gen, dtype=torch.float32) * 0.01).numpy()
                   for o in (opt_min, opt_max))
    return theta0, states


def unroll(problem, opt_min, opt_max, optim_it, rescale=1e-4, out_mul=1.0, theta0=None, states=None, seed=None, iter0=1,
           n_iter=None, record=("curve", "f")):
    """Iterations iter0 ... iter0 + n_iter - 1 (default: up to optim_it) of a run of optim_it iterations on every instance
    of `problem`, in one launch.  optim_it fixes the step schedule alone: iterations past it go on by the delta rule.  theta0 [n_inst, 2, dim] and states (see Result) are drawn by ``draw_start`` from a
    generator seeded by `seed` when None; to continue a run pass the theta and states of the Result before."""
    optim_it, iter0 = int(optim_it), int(iter0)
    n_sign, sign_lr = schedule(optim_it)
    if n_iter is None:
        n_iter = max(optim_it - iter0 + 1, 0)
    n_iter = int(n_iter)
    if iter0 < 1 or n_iter < 0:
        raise ValueError("twin.unroll: iter0 = %d, n_iter = %d" % (iter0, n_iter))
    record = tuple(record)
    if any(r not in ("curve", "f", "delta") for r in record):
        raise ValueError("twin.unroll: record %r (any of 'curve', 'f', 'delta')" % (record,))
    if theta0 is None or states is None:
        t0, s0 = draw_start(problem, opt_min, opt_max, seed)
        theta0 = t0 if theta0 is None else theta0
        states = s0 if states is None else states
    n_inst, dim = problem.n_inst, problem.dim
    theta0 = np.ascontiguousarray(theta0, dtype=np.float32)
    if theta0.shape != (n_inst, 2, dim):
        raise ValueError("twin.unroll: theta0 is %r, expected %r" % (theta0.shape, (n_inst, 2, dim)))
    states = tuple(np.ascontiguousarray(s, dtype=np.float32) for s in states)
    for s, o in zip(states, (opt_min, opt_max)):
        if s.shape != (4, o.hidden_size, n_inst * dim):
            raise ValueError("twin.unroll: a state is %r, expected %r" % (s.shape, (4, o.hidden_size, n_inst * dim)))
    engine = _engine.default_engine()
    out = engine.twin_unroll(tuple((o.hidden_size, o.n_in, o.params) for o in (opt_min, opt_max)),
                             (problem.kind, dim, problem.data),
                             dict(iter0=iter0, n_iter=n_iter, n_sign=n_sign, rescale=float(rescale), out_mul=float(out_mul),
                                  sign_lr=sign_lr),
                             theta0, states, record)
    curve = None
    if "curve" in record:
        curve = np.concatenate([theta0.reshape(n_inst, 1, 2 * dim),
                                np.asarray(out["curve"]).reshape(n_iter, n_inst, 2 * dim).transpose(1, 0, 2)], axis=1)
    f = np.ascontiguousarray(np.asarray(out["f"]).reshape(n_iter, n_inst).T) if "f" in record else None
    delta = np.ascontiguousarray(np.asarray(out["delta"]).reshape(n_iter, n_inst, dim).transpose(1, 0, 2)) \
        if "delta" in record else None
    return Result(theta=np.asarray(out["theta"]).reshape(n_inst, 2, dim), states=tuple(np.asarray(s) for s in out["states"]),
                  curve=curve, f=f, delta=delta, iter0=iter0, n_iter=n_iter, optim_it=optim_it, dim=dim)


def curve_info(result):
    """The reference's test-mode ``curve_info`` of a whole run (iter0 = 1, n_iter = optim_it):
    [n_inst, optim_it // 2 + 1, 2 dim]; row 0 the start, row j >= 1 holds u after iteration 2 j - 1 and v after 2 j."""
    if result.curve is None or result.iter0 != 1 or result.n_iter != result.optim_it:
        raise ValueError("twin.curve_info: needs the recorded curve of a whole run (iter0 = 1, n_iter = optim_it)")
    dim, half = result.dim, result.optim_it // 2
    info = np.zeros((result.curve.shape[0], half + 1, 2 * dim), dtype=result.curve.dtype)
    info[:, 0] = result.curve[:, 0]
    info[:, 1:, :dim] = result.curve[:, 1:2 * half:2, :dim]
    info[:, 1:, dim:] = result.curve[:, 2:2 * half + 1:2, dim:]
    return info


def distances(problem, result):
    """The reference's (all_distance_ever_u, all_distance_ever_v), each [n_inst, n_iter], of the point after every
    iteration: sum |u| and sum |v|; for the seesaw the distance of |u| to the nearest k / a, k = 0, 1, ... -- what the
    reference's search loop ends with (it walks k upwards past the minimum), evaluated in float32 as there."""
    if result.curve is None:
        raise ValueError("twin.distances: needs the recorded curve")
    dim = problem.dim
    pts = np.asarray(result.curve[:, 1:], dtype=np.float32)
    du = np.abs(pts[:, :, :dim]).sum(axis=2, dtype=np.float32)
    dv = np.abs(pts[:, :, dim:]).sum(axis=2, dtype=np.float32)
    if problem.kind == SEESAW:
        a = problem.data[:, 0].astype(np.float32)[:, None]
        with np.errstate(invalid="ignore", over="ignore"):
            k0 = np.nan_to_num(np.floor(du.astype(np.float64) * a), nan=0.0, posinf=0.0, neginf=0.0)
            best = du.copy()                                  # k = 0
            for dk in (-1.0, 0.0, 1.0, 2.0):
                k = np.maximum(k0 + dk, 0.0).astype(np.float32)
                best = np.minimum(best, np.abs(du - k / a))
        du = best
    return du, dv
