"""Milliseconds per meta-training step on N MNIST replicas (Replicas.train_step; BASELINE config 5's optimizee: RNNProp on
the 784-20-10 MLP, minibatch 64 -- or --batch_size 128, the reference's mnist config -- T = 20) in the one-instance-per-XCD
form (l2o_mlp_unroll_multi_record, up to eight replicas per launch) and in the whole-chip form (each replica's own
recording unroll, one after the other).  Median over --steps timed steps after --warmup; every step resets nothing (the
replicas carry their state, as the training drivers' segments do) and syncs on its losses.  One JSON line per form.

--eval_len T instead times the evaluation of the replicas (Replicas.run: one unroll of T steps per replica from a fresh
reset, the evaluate drivers' --replicas flow): median milliseconds per run of all N replicas and coordinate-steps per
second (N x 15 910 coordinates x T / time).

    python scripts/replica_train_bench.py [--replicas 8] [--batch_size 64] [--steps 30] [--warmup 5] [--forms xcd,chip]
    python scripts/replica_train_bench.py --batch_size 128 --eval_len 200 [--steps 10] [--warmup 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from open_l2o_amd import meta, meta_rnnprop_train, problems, util  # noqa: E402
from open_l2o_amd.replicas import Replicas  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--replicas", type=int, default=8)
    p.add_argument("--steps", type=int, default=30)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--unroll_length", type=int, default=20)
    p.add_argument("--forms", default="xcd,chip")
    p.add_argument("--batch_size", type=int, default=64)
    p.add_argument("--eval_len", type=int, default=0, help="time Replicas.run of this many steps instead of train_step")
    f = p.parse_args()
    T = f.eval_len or f.unroll_length
    data = problems.synthetic_mnist(2048, seed=0, label_noise=0.1)
    for form in f.forms.split(","):
        meta.set_random_seed(1)
        problem, net_config, assignments = util.get_config("mnist", net_name="RNNprop",
                                                           problem_options={"batch_size": f.batch_size, "data": data})
        opt = meta_rnnprop_train.MetaOptimizer(0, 0.95, 0.95, **net_config)
        reps = Replicas(opt, [problem] * f.replicas, T, assignments)
        if f.eval_len:
            evaluate(f, reps, form, T)
            continue
        reps.reset()
        times = []
        for i in range(f.warmup + f.steps):
            t0 = time.perf_counter()
            out = reps.train_step({reps.step: 1 + (i % 5) * T}, 1e-3, form=form)
            dt = time.perf_counter() - t0
            if i % 5 == 4:
                reps.reset()                             # (an epoch of 100 steps: five segments, as the drivers run it)
            if i >= f.warmup:
                times.append(dt)
        ms = 1e3 * float(np.median(times))
        line = {"metric": "replica_train_step_ms", "form": reps.last_form, "replicas": f.replicas, "T": T}
        if f.batch_size != 64:                          # (the batch-64 line stays what it was)
            line["batch_size"] = f.batch_size
        print(json.dumps(dict(line, **{"median_ms": round(ms, 4), "ms_per_replica": round(ms / f.replicas, 4),
                          "min_ms": round(1e3 * min(times), 4), "steps": len(times),
                          "loss": float(out["loss"])})), flush=True)


def evaluate(f, reps, form, T):
    """Replicas.run(form) of all replicas, reset before every run (not timed), synced on the losses."""
    times = []
    for i in range(f.warmup + f.steps):
        reps.reset()
        t0 = time.perf_counter()
        fx = reps.run({reps.step: 1}, form=form)
        dt = time.perf_counter() - t0
        if i >= f.warmup:
            times.append(dt)
    ms = 1e3 * float(np.median(times))
    ncoord = sum(int(np.prod(v.shape)) for v in reps.graphs[0].x)
    print(json.dumps({"metric": "replica_eval_ms", "form": reps.last_form, "replicas": f.replicas, "batch_size": f.batch_size,
                      "T": T, "median_ms": round(ms, 4), "min_ms": round(1e3 * min(times), 4),
                      "coord_steps_per_s": round(f.replicas * ncoord * T / (ms * 1e-3), 1), "runs": len(times),
                      "mean_final_loss": float(np.mean(fx))}), flush=True)


if __name__ == "__main__":
    main()
