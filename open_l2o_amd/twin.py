"""Twin-L2O: the reference's model-free minimax optimizer (``Model_Free_L2O/L2O-Minimax/Twin-L2O.py``): its evaluation
(``mode: "test"``) unroll and its meta-training (``mode: "train"``).

Two per-coordinate two-layer LSTM optimizers -- one steps the min variable ``u``, one the max variable ``v`` -- alternate
over an analytic saddle objective; every coordinate of every problem instance shares the two networks.  The reference calls
two ``nn.LSTMCell`` per iteration per instance from Python; here all iterations of all instances are ONE launch of
``l2o_twin_unroll`` (``libl2o_hip.so``, ``csrc/l2o_twin.h``).

Meta-training (``meta_gradient``, ``train_batch``, ``fit``: the reference's ``do_fit(should_train=True)`` and
``fit_optimizer``).  A training batch is cut into segments of ``2 unroll_unit`` iterations; a segment's forward, its BPTT and
the weight-gradient contraction are HIP (``csrc/l2o_twin_train.h``); ``torch.optim.Adam`` -- the reference's own optimizer --
steps both networks at every segment's end.  Inside a segment the LSTM inputs are detached, the stepped variable is detached
right after its loss is taken and the sign rule has derivative zero, so each network's gradient is a BPTT through its own
state chain alone; iteration k contributes ``(loss_k + loss_{k-1}) / batch_size`` with ``loss_k = +f`` after a min step and
``-f`` after a max step (``loss_{k-1} = 0`` at a segment's first iteration).

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


# ---------------------------------------------------------------------------------------------------------
# meta-training
# ---------------------------------------------------------------------------------------------------------
def _segment_forward(problem, opt_min, opt_max, optim_it, iter0, n_iter, theta0, states, rescale, out_mul, batch_size):
    """The recording forward of one segment: (Result of the forward, the engine's handle for _segment_backward)."""
    optim_it, iter0, n_iter = int(optim_it), int(iter0), int(n_iter)
    n_sign, sign_lr = schedule(optim_it)
    if iter0 < 1 or iter0 % 2 == 0 or n_iter < 2 or n_iter % 2:
        raise ValueError("twin.meta_gradient: a segment starts at an odd iteration and has an even number of them "
                         "(iter0 = %d, n_iter = %d)" % (iter0, n_iter))
    n_inst, dim = problem.n_inst, problem.dim
    theta0 = np.ascontiguousarray(theta0, dtype=np.float32)
    if theta0.shape != (n_inst, 2, dim):
        raise ValueError("twin.meta_gradient: theta0 is %r, expected %r" % (theta0.shape, (n_inst, 2, dim)))
    states = tuple(np.ascontiguousarray(s, dtype=np.float32) for s in states)
    for s, o in zip(states, (opt_min, opt_max)):
        if s.shape != (4, o.hidden_size, n_inst * dim):
            raise ValueError("twin.meta_gradient: a state is %r, expected %r" % (s.shape, (4, o.hidden_size, n_inst * dim)))
    batch_size = n_inst if batch_size is None else int(batch_size)
    out, handle = _engine.default_engine().twin_segment_forward(
        tuple((o.hidden_size, o.n_in, o.params) for o in (opt_min, opt_max)), (problem.kind, dim, problem.data),
        dict(iter0=iter0, n_iter=n_iter, n_sign=n_sign, rescale=float(rescale), out_mul=float(out_mul), sign_lr=sign_lr),
        theta0, states, 1.0 / batch_size)
    curve = np.concatenate([theta0.reshape(n_inst, 1, 2 * dim),
                            np.asarray(out["curve"]).reshape(n_iter, n_inst, 2 * dim).transpose(1, 0, 2)], axis=1)
    res = Result(theta=np.asarray(out["theta"]).reshape(n_inst, 2, dim), states=tuple(np.asarray(s) for s in out["states"]),
                 curve=curve, f=np.ascontiguousarray(np.asarray(out["f"]).reshape(n_iter, n_inst).T),
                 delta=np.ascontiguousarray(np.asarray(out["delta"]).reshape(n_iter, n_inst, dim).transpose(1, 0, 2)),
                 iter0=iter0, n_iter=n_iter, optim_it=optim_it, dim=dim, batch_size=batch_size)
    return res, handle


def _segment_backward(res, handle, inst_weight):
    """Fills res.grads and res.loss: the segment's total_loss, sum over k and instances of w_k s_k f m / batch_size in
    float64 from the recorded f (w_k = 2, 1 at the last iteration; s_k = +1 for a min step, -1 for a max step)."""
    if inst_weight is not None:
        inst_weight = np.ascontiguousarray(inst_weight, dtype=np.float32)
        if inst_weight.shape != (res.f.shape[0],):
            raise ValueError("twin.meta_gradient: inst_weight is %r, expected %r" % (inst_weight.shape, (res.f.shape[0],)))
    res.grads = _engine.default_engine().twin_segment_backward(handle, inst_weight)
    k = res.iter0 + np.arange(res.n_iter)
    ws = np.where(k % 2 == 1, 1.0, -1.0) * np.where(np.arange(res.n_iter) == res.n_iter - 1, 1.0, 2.0)
    m = np.ones(res.f.shape[0]) if inst_weight is None else inst_weight.astype(np.float64)
    res.loss = float((res.f.astype(np.float64) * ws[None, :] * m[:, None]).sum() / res.batch_size)
    return res


def meta_gradient(problem, opt_min, opt_max, optim_it, iter0, n_iter, theta0, states, rescale=1e-4, out_mul=1.0,
                  batch_size=None, inst_weight=None):
    """One segment of the meta-training: iterations iter0 (odd) ... iter0 + n_iter - 1 (n_iter even) of a run of optim_it
    iterations, and the gradient of the segment's loss with respect to both networks.  Returns the Result of ``unroll``
    (curve, f and delta recorded, bit for bit those of ``unroll``) with ``grads = (dict, dict)`` under PARAM_NAMES for the
    min and the max network and ``loss``, the segment's total_loss.  batch_size (default n_inst) is the reference's divisor;
    inst_weight [n_inst] (default all 1) the curriculum's weights."""
    res, handle = _segment_forward(problem, opt_min, opt_max, optim_it, iter0, n_iter, theta0, states, rescale, out_mul,
                                   batch_size)
    return _segment_backward(res, handle, inst_weight)


def sche_ratio(epoch_index):
    """The reference's curriculum schedule (Twin-L2O.py lines 84-88)."""
    if 0 <= epoch_index <= 80:
        return 0.2 + epoch_index / 100
    return 1


def get_index(curve_info, iteration_index, unroll_unit, batch_data, ratio):
    """The reference's ``metrics.get_index`` (utils/metrics.py lines 18-38): the instances that enter a segment's loss, the
    ``int(ratio * batch)`` with the smallest sum over the curve so far of ``(-b sin(a pi u))^2``.  As there: the curve so far
    is columns ``0 : flag * 2 * unroll_unit - 1`` with ``flag = iteration_index // 10`` (a literal 10; with flag 0 the slice
    ends at -1), the sums are Python floats, the sort is stable and descending, and ``[-k:]`` is the whole list when k = 0.
    (a and b enter as Python floats of their float32 values.)"""
    import math
    result = []
    k = int(ratio * len(curve_info))
    flag = iteration_index // 10
    curve_u = curve_info[:, 0:flag * 2 * unroll_unit - 1, 0]
    for i in range(len(curve_u)):
        a, b = float(batch_data[i, 0]), float(batch_data[i, 1])
        grad_v = [(-1) * b * math.sin(a * math.pi * float(u)) for u in curve_u[i]]
        result.append(sum([d ** 2 for d in grad_v]))
    return sorted(range(len(result)), key=lambda i: result[i], reverse=True)[-k:]


class Trainer(object):
    """The two networks' parameters as torch tensors and their two ``torch.optim.Adam`` (default betas and eps,
    ``lr = meta_lr``): the reference's meta-optimizers.  ``step`` assigns ``.grad`` from a segment's gradients, steps both
    and writes the new values back into the two ``Optimizer``s' float32 arrays."""

    def __init__(self, opt_min, opt_max, lr):
        self.opts = (opt_min, opt_max)
        self.tensors = tuple(collections.OrderedDict((k, torch.nn.Parameter(torch.from_numpy(o.params[k].copy())))
                                                     for k in PARAM_NAMES) for o in self.opts)
        self.adams = tuple(torch.optim.Adam(list(t.values()), lr=lr) for t in self.tensors)

    def step(self, grads):
        for o, t, adam, g in zip(self.opts, self.tensors, self.adams, grads):
            for k in PARAM_NAMES:
                t[k].grad = torch.from_numpy(np.ascontiguousarray(g[k], dtype=np.float32).reshape(tuple(t[k].shape)).copy())
            adam.step()
            for k in PARAM_NAMES:
                o.params[k] = t[k].detach().numpy().copy()

    def step_counts(self):
        """Adam's step count of the min and of the max network (0 before the first step)."""
        return tuple(int(next(iter(a.state.values()))["step"]) if a.state else 0 for a in self.adams)


def train_batch(problem, trainer, optim_it, unroll_unit, rescale=1e-4, out_mul=1.0, theta0=None, states=None, seed=None,
                curriculum=False, epoch_index=0, log=None):
    """The reference's ``do_fit(should_train=True)`` on one batch -- every instance of `problem` -- with the networks and
    Adams of `trainer`: optim_it iterations cut into segments of 2 unroll_unit; at each segment's end both Adams step on the
    segment's gradient (iterations past the last whole segment run without a step).  curriculum (the config's ``CL``;
    seesaw only): between a segment's forward and its backward ``get_index`` picks the instances that enter the loss from
    the train-mode curve so far (which, as in the reference, does not yet hold the segment's last iteration); with none
    picked there is no backward and no step.  A segment wholly inside the sign phase has zero gradients and still steps.
    Returns (all_distance_ever_v, all_distance_ever_u, curve_info): the distances [batch, optim_it] and the train-mode
    curve_info [batch, optim_it, 2 dim] (row k - 1: the point after iteration k).  log: a list that gets one dict per
    segment (iter0, inst_weight, loss, stepped)."""
    optim_it, unroll_unit = int(optim_it), int(unroll_unit)
    if curriculum and problem.kind != SEESAW:
        raise ValueError("twin.train_batch: the curriculum (CL) ranks instances by the seesaw's gradient, (-b sin(a pi u))^2: "
                         "it is defined for loss 3 only (got loss %d)" % problem.kind)
    if unroll_unit < 1:
        raise ValueError("twin.train_batch: unroll_unit %d" % unroll_unit)
    schedule(optim_it)
    opt_min, opt_max = trainer.opts
    if theta0 is None or states is None:
        t0, s0 = draw_start(problem, opt_min, opt_max, seed)
        theta0 = t0 if theta0 is None else theta0
        states = s0 if states is None else states
    n_inst, dim, L = problem.n_inst, problem.dim, 2 * unroll_unit
    info = np.zeros((n_inst, optim_it, 2 * dim))
    theta, iter0 = np.ascontiguousarray(theta0, dtype=np.float32), 1
    while iter0 + L - 1 <= optim_it:
        res, handle = _segment_forward(problem, opt_min, opt_max, optim_it, iter0, L, theta, states, rescale, out_mul, n_inst)
        info[:, iter0 - 1:iter0 + L - 2] = res.curve[:, 1:L]
        weight, stepped = None, True
        if curriculum:
            index = get_index(info, iter0 + L - 1, unroll_unit, problem.data, sche_ratio(epoch_index))
            weight = np.zeros(n_inst, np.float32)
            for b in index:
                weight[b] += 1.0
            stepped = len(index) > 0
        info[:, iter0 + L - 2] = res.curve[:, L]
        if stepped:
            _segment_backward(res, handle, weight)
            trainer.step(res.grads)
        if log is not None:
            log.append(dict(iter0=iter0, inst_weight=weight, loss=res.loss if stepped else None, stepped=stepped))
        theta, states, iter0 = res.theta, res.states, iter0 + L
    if iter0 <= optim_it:
        res = unroll(problem, opt_min, opt_max, optim_it, rescale=rescale, out_mul=out_mul, theta0=theta, states=states,
                     iter0=iter0, record=("curve",))
        info[:, iter0 - 1:] = res.curve[:, 1:]
    whole = Result(curve=np.concatenate([np.zeros((n_inst, 1, 2 * dim), np.float32), info.astype(np.float32)], axis=1))
    du, dv = distances(problem, whole)
    return dv, du, info


def batch_seed(seed, epoch, batch):
    """The seed of ``draw_start`` for batch `batch` of epoch `epoch` of a ``fit`` with config seed `seed`:
    ``(seed * 1000003 + epoch) * 1000003 + batch + 1``, reduced mod 2^63.  (The reference draws every batch's start from the
    global torch generator as it goes; here each batch's draw stands alone.)"""
    return ((int(seed) * 1000003 + int(epoch)) * 1000003 + int(batch) + 1) % (1 << 63)


EVAL_SEED = 70


def evaluate(params, eval_prob, opt_min, opt_max):
    """fit_optimizer's evaluation loss: every eval instance in ONE ``unroll`` launch of eval_optim_iter iterations, the mean
    over instances of sum(dist_v^2 + dist_u^2) after the burn-in half."""
    theta0, states = draw_start(eval_prob, opt_min, opt_max, seed=EVAL_SEED)
    res = unroll(eval_prob, opt_min, opt_max, params["eval_optim_iter"], rescale=params["rescale"], out_mul=1.0, theta0=theta0,
                 states=states, record=("curve",))
    du, dv = distances(eval_prob, res)
    burn = int(0.5 * params["eval_optim_iter"])
    du, dv = np.asarray(du, np.float64)[:, burn:], np.asarray(dv, np.float64)[:, burn:]
    return float(np.mean(np.sum(np.square(dv) + np.square(du), axis=1)))


def fit(params, root, out, epochs=None, eval_interval=5, verbose=False):
    """The reference's ``fit_optimizer`` for a ``*_train.json`` config (dict `params`; paths relative to `root`; results under
    `out`).  Per epoch: the training rows are shuffled by ``RandomState(10)`` -- the stream of the reference's
    ``np.random.seed(10)`` / ``np.random.shuffle`` -- (the matrix game's on their reshaped [n, dim, dim] form);
    ``n_train // batch_size`` batches of ``train_batch``, each from a start drawn by ``draw_start(seed=batch_seed(seed, epoch,
    batch))``; ``epoch{e}min.pth`` / ``epoch{e}max.pth`` (``torch.save`` of the reference-named state dict); with
    ``save_curve`` every instance's train-mode curve under ``curve_info/epoch{e}/`` by the reference's names; every
    eval_interval epochs ``evaluate`` and, on improvement, ``bestmin.pth`` / ``bestmax.pth``.  The networks are seeded `seed`
    and `seed + 1`.  ``save_train`` (the reference's seaborn plots) is read and ignored.  Data files shorter than n_train / n_eval are used as
    far as they go, with a warning.  Returns (best_loss, opt_min,
    opt_max, history: one dict per epoch)."""
    dim, loss = int(params.get("dim", 1)), int(params["loss"])
    curriculum = bool(params.get("CL", 0))
    if curriculum and loss != SEESAW:
        raise ValueError("twin.fit: \"CL\": 1 ranks instances by the seesaw's gradient: loss 3 only (got loss %d)" % loss)
    n_train, n_eval, batch = int(params["n_train"]), int(params["n_eval"]), int(params["batch_size"])
    epochs = int(params["train_epochs"] if epochs is None else epochs)

    def find(rel):
        for q in (os.path.join(root, rel), os.path.join(root, os.path.basename(rel))):
            if os.path.exists(q):
                return q
        raise FileNotFoundError("twin.fit: %s not found under %s" % (rel, root))

    train = np.loadtxt(find(params["train_data_path"]), ndmin=2).astype(np.float32)[:n_train]
    evald = np.loadtxt(find(params["eval_data_path"]), ndmin=2).astype(np.float32)[:n_eval]
    if train.shape[0] < n_train or evald.shape[0] < n_eval or n_train < batch:
        # (the reference slices [0:n_train] without a check and then fails on the first batch; a short file -- the truncated
        # fixtures of tests/golden/twin -- trains on what it holds, in one batch at the most, and says so)
        import warnings
        warnings.warn("twin.fit: n_train = %d, n_eval = %d, batch_size = %d but the data holds %d and %d instances: using "
                      "what is there" % (n_train, n_eval, batch, train.shape[0], evald.shape[0]))
        n_train, n_eval = min(n_train, train.shape[0]), min(n_eval, evald.shape[0])
        batch = min(batch, n_train)
    if batch < 1 or n_eval < 1:
        raise ValueError("twin.fit: batch_size = %d, n_eval = %d" % (batch, n_eval))
    if loss == MATRIX_GAME:
        train, evald = train.reshape(n_train, dim, dim), evald.reshape(n_eval, dim, dim)
    eval_prob = Problem(loss, evald, dim)
    seed = int(params.get("seed", 0))
    opts = tuple(Optimizer(hidden_size=params["hidden_size"], use_second=bool(params["use_second"]), seed=seed + i)
                 for i in range(2))
    trainer = Trainer(opts[0], opts[1], lr=params["meta_lr"])
    rng = np.random.RandomState(10)
    os.makedirs(out, exist_ok=True)
    best, history = 100000000000000000, []
    for epoch in range(epochs):
        rng.shuffle(train)
        for it in range(n_train // batch):
            rows = train[it * batch:(it + 1) * batch]
            prob = Problem(loss, rows, dim)
            theta0, states = draw_start(prob, opts[0], opts[1], seed=batch_seed(seed, epoch, it))
            dv, du, info = train_batch(prob, trainer, params["train_optim_iter"], params["unroll_unit"],
                                       rescale=params["rescale"], out_mul=1.0, theta0=theta0, states=states,
                                       curriculum=curriculum, epoch_index=epoch)
            if params.get("save_curve"):
                cdir = os.path.join(out, "curve_info", "epoch%d" % epoch)
                os.makedirs(cdir, exist_ok=True)
                for i in range(batch):
                    first, last = float(rows[i].reshape(-1)[0]), float(rows[i].reshape(-1)[-1])
                    np.savetxt(os.path.join(cdir, "iteration%d_batch_index_%d_u_%s_v_%s.txt"
                                            % (it, i, round(first, 3), round(last, 3))), info[i])
        for o, which in zip(opts, ("min", "max")):
            torch.save(o.state_dict(), os.path.join(out, "epoch%d%s.pth" % (epoch, which)))
        entry = dict(epoch=epoch, steps=trainer.step_counts(), eval_loss=None)
        if epoch % int(eval_interval) == 0:
            entry["eval_loss"] = evaluate(params, eval_prob, opts[0], opts[1])
            if entry["eval_loss"] < best:
                best = entry["eval_loss"]
                for o, which in zip(opts, ("min", "max")):
                    torch.save(o.state_dict(), os.path.join(out, "best%s.pth" % which))
        history.append(entry)
        if verbose:
            print(entry)
    return best, opts[0], opts[1], history
