"""Time the confocal optimizee (problems.confocal_microscopy_3d, util.get_config("confocal_microscopy_3d")) on the GPU, in
one process, with HIP events after a warm-up:

  * us per l2o_confocal_fg -- loss and all 6P + 1 gradients of one evaluation in simulation mode -- and forward only;
  * the per-kernel split comes from the device, in a run of its own: ``--loop N`` runs N bare evaluations and nothing else,
    for ``rocprofv3 --kernel-trace --stats -- python scripts/confocal_step_bench.py --loop 2000``;
  * us per optimizer step -- one unroll of meta_loss (the plain (20, 20) coordinate-wise net over the 31 variables) on the
    step-granular path, divided by its length -- and the launches per step;
  * as the yardstick that is not the code under test: the same loss and gradients through float32 torch autograd on the
    same GPU (torch.erf on the separable tables, one einsum per point), timed the same way.

    python scripts/confocal_step_bench.py [--batch 32] [--points 5] [--roi 28] [--iters 500] [--unroll 20] [--unrolls 10]

Prints one JSON line."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from open_l2o_amd import _engine, meta, util  # noqa: E402
from open_l2o_amd.session import Session  # noqa: E402


def _timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1) / iters


def _inputs(batch, points, seed=0):
    rng = np.random.default_rng(seed)
    nv = 6 * points + 1
    return ([rng.random(batch).astype(np.float32) for _ in range(nv)],
            [rng.random(batch).astype(np.float32) for _ in range(nv)])


def make_fg(eng, batch, points, roi, want_grad=True):
    theta, sim = _inputs(batch, points)
    d = _engine.ConfocalDesc(batch, points, roi)
    th, sm = [eng.tensor(a) for a in theta], [eng.tensor(a) for a in sim]
    grads = [eng.zeros(batch) for _ in theta] if want_grad else None
    loss = eng.zeros(1)
    return (lambda: eng.confocal_fg(d, th, sm, loss, grads)), loss, (theta, sim)


def time_torch(theta, sim, points, roi, iters, warmup=20):
    """The same loss and gradients through float32 torch autograd on the GPU."""
    dev = torch.device("cuda")
    vs = [torch.tensor(a, device=dev).requires_grad_(True) for a in theta]
    ss = [torch.tensor(a, device=dev) for a in sim]
    ks = [torch.arange(r, device=dev, dtype=torch.float32)[None, :] for r in roi]
    out = {}

    def axis(c, sg, k):
        den = math.sqrt(2.0) * sg[:, None]
        return torch.erf((k + 0.5 - c[:, None]) / den) - torch.erf((k - 0.5 - c[:, None]) / den)

    def volume(v):
        vol = v[6 * points][:, None, None, None]
        for p in range(points):
            t_i, t_x, t_y, t_z, t_sxy, t_sz = v[6 * p:6 * p + 6]
            sxy, sz = 2.0 + 2.0 * t_sxy, 2.0 + 2.0 * t_sz
            ex = axis(0.5 + (roi[0] - 1.5) * t_x, sxy, ks[0])
            ey = axis(0.5 + (roi[1] - 1.5) * t_y, sxy, ks[1])
            ez = axis(0.5 + (roi[2] - 1.5) * t_z, sz, ks[2])
            vol = vol + torch.einsum("b,by,bx,bz->byxz", (0.5 + 1.5 * t_i) / 8.0, ey, ex, ez)
        return vol.reshape(vol.shape[0], -1)

    def fg():
        t = volume(ss)
        target = t * torch.rsqrt(torch.clamp((t * t).sum(1, keepdim=True), min=1e-12))
        loss = ((volume(vs) - target) ** 2).sum(1).mean()
        out["loss"], out["grads"] = loss, torch.autograd.grad(loss, vs)

    us = _timed(fg, iters, warmup)
    return us, float(out["loss"].detach())


def time_step(eng, batch, points, roi, T, unrolls, warmup=2):
    problem, net_config, na = util.get_config("confocal_microscopy_3d", problem_options={
        "batch_size": batch, "num_points": points, "ROI": list(roi)})
    optimizer = meta.MetaOptimizer(**net_config)
    ml = optimizer.meta_loss(problem, T, net_assignments=na)
    graph = optimizer.graph
    counts = {"confocal_fg": 0}
    orig_fg = eng.confocal_fg

    def fg(*a, **k):
        counts["confocal_fg"] += 1
        return orig_fg(*a, **k)
    eng.confocal_fg = fg
    times = []
    with Session() as sess:
        sess.run(ml.reset)
        for k in range(warmup + unrolls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            graph.launch({}, commit=True, events=(e0, e1))
            e1.synchronize()
            if k >= warmup:
                times.append(1e3 * e0.elapsed_time(e1) / T)
    del eng.confocal_fg
    nvar = len(graph.x)
    lstm_launches = -(-nvar // eng.MAX_STEP_SEGS)            # l2o_cwlstm_step_multi takes MAX_STEP_SEGS variables per launch
    assert counts["confocal_fg"] == (warmup + unrolls) * (T + 1)
    return float(np.median(times)), graph.last_path, nvar, lstm_launches


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=32)
    p.add_argument("--points", type=int, default=5)
    p.add_argument("--roi", type=int, default=28)
    p.add_argument("--iters", type=int, default=500)
    p.add_argument("--unroll", type=int, default=20)
    p.add_argument("--unrolls", type=int, default=10)
    p.add_argument("--loop", type=int, default=0, help="only run this many bare evaluations (for a kernel trace)")
    a = p.parse_args()
    roi = (a.roi, a.roi, a.roi)
    eng = _engine.HipEngine()
    _engine.set_default_engine(eng)
    meta.set_random_seed(0)
    fg, loss, (theta, sim) = make_fg(eng, a.batch, a.points, roi)
    if a.loop:
        for _ in range(a.loop):
            fg()
        torch.cuda.synchronize()
        print(json.dumps({"workload": "confocal_microscopy_3d", "loop": a.loop, "loss": float(eng.to_numpy(loss)[0])}))
        return
    fg_us = _timed(fg, a.iters, 20)
    f, loss_f, _ = make_fg(eng, a.batch, a.points, roi, want_grad=False)
    f_us = _timed(f, a.iters, 20)
    torch_us, torch_loss = time_torch(theta, sim, a.points, roi, a.iters)
    step_us, path, nvar, lstm_launches = time_step(eng, a.batch, a.points, roi, a.unroll, a.unrolls)
    print(json.dumps({"workload": "confocal_microscopy_3d", "batch": a.batch, "points": a.points, "roi": list(roi),
                      "variables": nvar, "fg_us": round(fg_us, 2), "forward_only_us": round(f_us, 2),
                      "torch_autograd_fg_us": round(torch_us, 2), "loss": float(eng.to_numpy(loss)[0]),
                      "torch_loss": torch_loss, "step_us": round(step_us, 2), "unroll": a.unroll, "path": path,
                      "launches_per_step": {"l2o_confocal_fg": 2, "l2o_cwlstm_step_multi": lstm_launches},
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
