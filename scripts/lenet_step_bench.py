"""Time the LeNet optimizee (problems.LeNet, util.get_config("lenet")) on the GPU, in one process, with HIP events after a
warm-up:

  * us per l2o_lenet_fg -- loss and all gradients of one minibatch (batch norm on, the reference's default);
  * us per optimizer step -- one unroll of meta_loss (the default LogAndSign coordinate-wise net over all 62 232
    coordinates) on the step-granular path, divided by its length: per step the fg, the LSTM step and the minibatch draw;
  * as the yardstick that is not the code under test: the same loss and gradients through float32 torch autograd on the
    same GPU (conv2d / max_pool2d / matmul of the installed torch, batch norm from var_mean), timed the same way.

    python scripts/lenet_step_bench.py [--batch 128] [--iters 200] [--unroll 20] [--unrolls 10]

Prints one JSON line.  Synthetic CIFAR-10-shaped data (problems.synthetic_cifar10); the arithmetic does not depend on it."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from open_l2o_amd import _engine, meta, problems, util  # noqa: E402
from open_l2o_amd.session import Session  # noqa: E402

SHAPES = [(5, 5, 3, 6), (6,), (6,), (5, 5, 6, 16), (16,), (16,), (400, 120), (120,), (120,), (120, 84), (84,), (84,),
          (84, 10), (10,)]


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


def time_fg(eng, data, batch, iters, warmup=20):
    images = np.ascontiguousarray(data["images"], np.float32).reshape(len(data["labels"]), -1)
    d = _engine.LenetDesc(batch, True, eng.tensor(images), eng.int_tensor(data["labels"]))
    rng = np.random.default_rng(0)
    rows = rng.integers(0, len(images), batch)
    idx = eng.int_tensor(rows)
    w = [rng.normal(0, 0.01, sh).astype(np.float32) for sh in SHAPES]
    for k in (2, 5, 8, 11):
        w[k][:] = 0.0
    ws = [eng.tensor(a) for a in w]
    grads = [eng.zeros(*sh) for sh in SHAPES]
    loss = eng.zeros(1)
    fg_us = _timed(lambda: eng.lenet_fg(d, idx, ws, loss, grads), iters, warmup)
    return fg_us, float(eng.to_numpy(loss)[0]), (images[rows], np.asarray(data["labels"])[rows], w)


def time_torch(x, y, w, iters, warmup=20):
    """The same net through float32 torch autograd on the GPU."""
    dev = torch.device("cuda")
    x = torch.tensor(x, device=dev).reshape(-1, 32, 32, 3).permute(0, 3, 1, 2).contiguous()
    y = torch.tensor(y, device=dev, dtype=torch.int64)
    vs = [torch.tensor(a, device=dev).requires_grad_(True) for a in w]
    out = {}

    def bn(h, dims, beta):                  # batch statistics, biased variance, an offset and no scale
        var, mean = torch.var_mean(h, dims, unbiased=False, keepdim=True)
        return (h - mean) * torch.rsqrt(var + 1e-3) + beta

    def fg():
        h = x
        for k in (0, 3):
            h = F.conv2d(h, vs[k].permute(3, 2, 0, 1)) + vs[k + 1].view(1, -1, 1, 1)
            h = F.max_pool2d(torch.sigmoid(bn(h, (0, 2, 3), vs[k + 2].view(1, -1, 1, 1))), 2, 2)
        h = h.permute(0, 2, 3, 1).reshape(h.shape[0], -1)
        for k in (6, 9):
            h = torch.sigmoid(bn(h @ vs[k] + vs[k + 1], (0,), vs[k + 2]))
        loss = F.cross_entropy(h @ vs[12] + vs[13], y)
        out["loss"], out["grads"] = loss, torch.autograd.grad(loss, vs)

    us = _timed(fg, iters, warmup)
    return us, float(out["loss"])


def time_step(data, batch, T, unrolls, warmup=2):
    problem, net_config, na = util.get_config("lenet", problem_options={"data": data, "batch_size": batch})
    optimizer = meta.MetaOptimizer(**net_config)
    ml = optimizer.meta_loss(problem, T, net_assignments=na)
    graph = optimizer.graph
    n_coord = sum(int(np.prod(v.shape)) for v in graph.x)
    times = []
    with Session() as sess:
        sess.run(ml.reset)
        for k in range(warmup + unrolls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            graph.launch({}, commit=True, events=(e0, e1))
            e1.synchronize()
            if k >= warmup:
                times.append(1e3 * e0.elapsed_time(e1) / T)
    return float(np.median(times)), graph.last_path, n_coord


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=128)
    p.add_argument("--iters", type=int, default=200)
    p.add_argument("--unroll", type=int, default=20)
    p.add_argument("--unrolls", type=int, default=10)
    a = p.parse_args()
    eng = _engine.HipEngine()
    _engine.set_default_engine(eng)
    meta.set_random_seed(0)
    data = problems.synthetic_cifar10(4096, seed=0)
    fg_us, loss, (x, y, w) = time_fg(eng, data, a.batch, a.iters)
    torch_us, torch_loss = time_torch(x, y, w, a.iters)
    step_us, path, n_coord = time_step(data, a.batch, a.unroll, a.unrolls)
    print(json.dumps({"workload": "lenet", "batch": a.batch, "coordinates": n_coord, "fg_us": round(fg_us, 2),
                      "torch_autograd_fg_us": round(torch_us, 2), "loss": loss, "torch_loss": torch_loss,
                      "step_us": round(step_us, 2), "unroll": a.unroll, "path": path,
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
