"""Milliseconds per meta-training step on N MNIST replicas (Replicas.train_step; BASELINE config 5's optimizee: RNNProp on
the 784-20-10 MLP, minibatch 64, T = 20) in the one-instance-per-XCD form (l2o_mlp_unroll_multi_record, up to eight
replicas per launch) and in the whole-chip form (each replica's own l2o_mlp_unroll_record launch, one after the other).
Median over --steps timed steps after --warmup; every step resets nothing (the replicas carry their state, as the
training drivers' segments do) and syncs on its losses.  One JSON line per form.

    python scripts/replica_train_bench.py [--replicas 8] [--steps 30] [--warmup 5] [--forms xcd,chip]
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
    f = p.parse_args()
    T = f.unroll_length
    data = problems.synthetic_mnist(2048, seed=0, label_noise=0.1)
    for form in f.forms.split(","):
        meta.set_random_seed(1)
        problem, net_config, assignments = util.get_config("mnist", net_name="RNNprop",
                                                           problem_options={"batch_size": 64, "data": data})
        opt = meta_rnnprop_train.MetaOptimizer(0, 0.95, 0.95, **net_config)
        reps = Replicas(opt, [problem] * f.replicas, T, assignments)
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
        print(json.dumps({"metric": "replica_train_step_ms", "form": reps.last_form, "replicas": f.replicas, "T": T,
                          "median_ms": round(ms, 4), "ms_per_replica": round(ms / f.replicas, 4),
                          "min_ms": round(1e3 * min(times), 4), "steps": len(times),
                          "loss": float(out["loss"])}), flush=True)


if __name__ == "__main__":
    main()
