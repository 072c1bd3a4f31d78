"""The reference's confocal_microscopy_3d optimizee (DM/problems.py:701-956) in torch on the CPU, float64 or float32: loss and
gradients by autograd, written from the problem's formulas; not a test module: the tests import it.

Per batch row, P points with raw parameters t (not clipped) mapped affinely -- I0 = 0.5 + 1.5 t, centre = 0.5 + (R - 1.5) t
per axis, sigma = 2 + 2 t -- and one point's image at voxel (ix, iy, iz) is I0 Ex[ix] Ey[iy] Ez[iz] / 8 with
E[k] = erf((k + 0.5 - c) / (sqrt2 sigma)) - erf((k - 0.5 - c) / (sqrt2 sigma)); x and y share sigma_xy.
pred = sum of the images + bg; target = l2_normalize(t) = t rsqrt(max(sum t^2, 1e-12)) with t the same sum over the
simulation parameters + bg_sim, or a supplied volume; loss = mean_b sum_v (pred - target)^2.  The volume is built here in the
order [batch, iy, ix, iz] (TF's default meshgrid 'xy' order, flat index (iy Rx + ix) Rz + iz), which is the order a supplied
volume is read in.

    ref = Confocal(roi=(Rx, Ry, Rz), num_points=P, img=None | [batch, V])
    f, grads = ref.fg(theta, sim)          # theta / sim / grads: 6P + 1 arrays [batch] in the graph's order: per point
                                           # I, x, y, z, sigmaxy, sigmaz; then bg.  sim is None with an img.
    fg = ref.flat_fg(batch, sim)           # fg(x, t) of helpers.oracle_meta_grad over the flat concatenation
"""
import math

import numpy as np
import torch

PARTS = ("I", "x", "y", "z", "sigmaxy", "sigmaz")


def trainable_names(num_points):
    return ["%s_var_%d" % (p, i) for i in range(num_points) for p in PARTS] + ["bg_var"]


def sim_names(num_points):
    """The reference's spelling: y_sim%d has no underscore."""
    return [("y_sim%d" if p == "y" else p + "_sim_%d") % i for i in range(num_points) for p in PARTS] + ["bg_sim"]


def declared_names(num_points, inference=False):
    """Declaration order: the trainable point arrays, the simulation arrays, bg_var, bg_sim."""
    tr = trainable_names(num_points)
    if inference:
        return tr
    sm = sim_names(num_points)
    return tr[:-1] + sm[:-1] + ["bg_var", "bg_sim"]


class Confocal(object):
    def __init__(self, roi, num_points, img=None):
        self.roi = tuple(int(r) for r in roi)
        self.P = int(num_points)
        self.img = None if img is None else np.asarray(img, np.float64).reshape(len(img), -1)

    def _axis(self, c, sg, R, dt):
        """[batch, R]: E[k] for the centre c and width sg (each [batch])."""
        k = torch.arange(R, dtype=dt)[None, :]
        den = math.sqrt(2.0) * sg[:, None]
        return torch.erf((k + 0.5 - c[:, None]) / den) - torch.erf((k - 0.5 - c[:, None]) / den)

    def volume(self, vs, dt):
        """[batch, Ry, Rx, Rz]: the image sum of the 6P + 1 arrays vs plus the background."""
        rx, ry, rz = self.roi
        out = vs[6 * self.P][:, None, None, None]
        for p in range(self.P):
            t_i, t_x, t_y, t_z, t_sxy, t_sz = vs[6 * p:6 * p + 6]
            sxy, sz = 2.0 + 2.0 * t_sxy, 2.0 + 2.0 * t_sz
            ex = self._axis(0.5 + (rx - 1.5) * t_x, sxy, rx, dt)
            ey = self._axis(0.5 + (ry - 1.5) * t_y, sxy, ry, dt)
            ez = self._axis(0.5 + (rz - 1.5) * t_z, sz, rz, dt)
            i0 = 0.5 + 1.5 * t_i
            out = out + (i0 / 8.0)[:, None, None, None] * ey[:, :, None, None] * ex[:, None, :, None] * ez[:, None, None, :]
        return out

    def fg(self, theta, sim=None, want_grad=True):
        """(loss, [gradient per trainable array]) in the dtype of ``theta``."""
        npdt = np.float64 if np.asarray(theta[0]).dtype == np.float64 else np.float32
        dt = torch.float64 if npdt == np.float64 else torch.float32
        vs = [torch.tensor(np.asarray(a, npdt).reshape(-1), dtype=dt).requires_grad_(want_grad) for a in theta]
        assert len(vs) == 6 * self.P + 1
        batch = vs[0].shape[0]
        pred = self.volume(vs, dt).reshape(batch, -1)
        if self.img is not None:
            t = torch.tensor(self.img.astype(npdt), dtype=dt)
        else:
            ss = [torch.tensor(np.asarray(a, npdt).reshape(-1), dtype=dt) for a in sim]
            t = self.volume(ss, dt).reshape(batch, -1)
        target = t * torch.rsqrt(torch.clamp((t * t).sum(1, keepdim=True), min=1e-12))
        loss = ((pred - target) ** 2).sum(1).mean()
        if not want_grad:
            return npdt(loss.detach().numpy()), None
        grads = torch.autograd.grad(loss, vs)
        return npdt(loss.detach().numpy()), [g.detach().numpy().astype(npdt) for g in grads]

    def flat_fg(self, batch, sim=None, scales=None):
        """``fg(x, t)`` over the flat concatenation of the 6P + 1 arrays (helpers.oracle_meta_grad); with scales (one array
        per variable) f(x * s) and s * grad f(x * s)."""
        nv = 6 * self.P + 1
        s = None if scales is None else np.concatenate([np.asarray(a, np.float64).reshape(-1) for a in scales])

        def fg(x, t):
            sc = None if s is None else s.astype(x.dtype)
            xs = x if sc is None else x * sc
            sm = None if sim is None else [np.asarray(a).astype(x.dtype) for a in sim]
            f, grads = self.fg([xs[i * batch:(i + 1) * batch] for i in range(nv)], sm)
            g = np.concatenate([a.reshape(-1) for a in grads])
            return f, (g if sc is None else g * sc)
        return fg


def sample(batch, num_points, seed, lo=0.0, hi=1.0):
    """(theta, sim): 6P + 1 float32 arrays [batch] each, raw values uniform in [lo, hi]."""
    rng = np.random.default_rng(seed)
    nv = 6 * num_points + 1
    draw = lambda: [(lo + (hi - lo) * rng.random(batch)).astype(np.float32) for _ in range(nv)]   # noqa: E731
    return draw(), draw()
