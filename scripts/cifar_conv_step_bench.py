"""Time the CIFAR-10 conv-net optimizee (problems.cifar10, util.get_config("cifar_conv")) on the GPU, in one process, with HIP events after a warm-up:

  * us per l2o_cifar_conv_fg -- loss and all gradients of one minibatch (batch norm on, the reference's default);
  * us per optimizer step -- one unroll of meta_loss (the default LogAndSign coordinate-wise net over all 13 706
    coordinates) on the step-granular path, divided by its length: per step the fg, the LSTM step and the minibatch draw.

    python scripts/cifar_conv_step_bench.py [--batch 128] [--iters 200] [--unroll 20] [--unrolls 10]

Prints one JSON line.  Synthetic CIFAR-10-shaped data (problems.synthetic_cifar10); the arithmetic does not depend on it."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from open_l2o_amd import _engine, meta, problems, util  # noqa: E402
from open_l2o_amd.session import Session  # noqa: E402


def time_fg(eng, data, batch, iters, warmup=20):
    images = np.ascontiguousarray(data["images"], np.float32).reshape(len(data["labels"]), -1)
    d = _engine.CifarConvDesc(batch, True, eng.tensor(images), eng.int_tensor(data["labels"]))
    rng = np.random.default_rng(0)
    idx = eng.int_tensor(rng.integers(0, len(images), batch))
    shapes = [(3, 3, 3, 16), (16,), (16,), (16,), (5, 5, 16, 32), (32,), (32,), (32,), (32, 10), (10,)]
    ws = [eng.tensor(rng.normal(0, 0.01, sh)) for sh in shapes]
    for k in (2, 6):
        ws[k].fill_(1.0)
    grads = [eng.zeros(*sh) for sh in shapes]
    loss = eng.zeros(1)
    for _ in range(warmup):
        eng.cifar_conv_fg(d, idx, ws, loss, grads)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        eng.cifar_conv_fg(d, idx, ws, loss, grads)
    e1.record()
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1) / iters


def time_step(data, batch, T, unrolls, warmup=2):
    problem, net_config, na = util.get_config("cifar_conv", problem_options={"data": data, "batch_size": batch})
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
    fg_us = time_fg(eng, data, a.batch, a.iters)
    step_us, path, n_coord = time_step(data, a.batch, a.unroll, a.unrolls)
    print(json.dumps({"workload": "cifar_conv", "batch": a.batch, "coordinates": n_coord, "fg_us": round(fg_us, 2),
                      "step_us": round(step_us, 2), "unroll": a.unroll, "path": path,
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
