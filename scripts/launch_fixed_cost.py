#!/usr/bin/env python
"""Fixed cost of one fused unroll launch, from a sweep over the unroll length T.

    python bench.py --unroll T --steps 20 --warmup 5 > run_T.json        (T = 25, 50, 100, 200 ...; one file per run)
    python scripts/launch_fixed_cost.py parent=runs/parent_*.json new=runs/new_*.json

Every file holds the JSON result line of one bench.py run (other lines are ignored).  Per label, ms_per_unroll is fitted
against T by least squares: the SLOPE is the time of one step of the step loop, the INTERCEPT the time a launch costs
whatever its length -- launch latency, workgroup ramp, prologue, epilogue, the combine kernel and its dependent launch.
With --full runs the in-kernel counters are fitted the same way (cycles of wave 0 of workgroup 0: kernel entry to last
store, and the step loop alone), which splits the intercept into the part inside that wave and the rest."""
import glob
import json
import re
import sys

import numpy as np


def result_line(path):
    for line in open(path):
        line = line.strip()
        if line.startswith("{") and '"ms_per_unroll"' in line:
            return json.loads(line)
    raise SystemExit("%s: no bench.py result line" % path)


def unroll_length(res):
    m = re.search(r"\bT\s*=\s*(\d+)", res["config"]["workload"])
    if not m:
        raise SystemExit("no T in %r" % res["config"]["workload"])
    return int(m.group(1))


def fit(ts, ys):
    """least squares y = a + b T -> (a, b, largest residual)"""
    A = np.stack([np.ones(len(ts)), np.asarray(ts, np.float64)], 1)
    (a, b), *_ = np.linalg.lstsq(A, np.asarray(ys, np.float64), rcond=None)
    return a, b, float(np.max(np.abs(A @ np.array([a, b]) - ys)))


def main(argv):
    if not argv:
        raise SystemExit(__doc__)
    for item in argv:
        label, _, pattern = item.partition("=")
        paths = sorted(glob.glob(pattern))
        if len(paths) < 2:
            raise SystemExit("%s: %d files match %r (need two values of T at least)" % (label, len(paths), pattern))
        runs = [result_line(p) for p in paths]
        ts = [unroll_length(r) for r in runs]
        us = [r["ms_per_unroll"] * 1e3 for r in runs]
        for t in sorted(set(ts)):
            v = [u for tt, u in zip(ts, us) if tt == t]
            print("%-8s T=%-4d us per unroll: %s" % (label, t, "  ".join("%.2f" % x for x in v)))
        a, b, res = fit(ts, us)
        print("%-8s wall: intercept %.2f us per launch, slope %.4f us per step (largest residual %.2f us, %d runs)"
              % (label, a, b, res, len(runs)))
        roofs = [r.get("roofline") or {} for r in runs]
        if all("cycles_per_step_in_kernel" in rf for rf in roofs):
            hz = float(np.mean([rf["clock_hz"] for rf in roofs]))
            tot = [rf["cycles_per_step_in_kernel"] * (t + 0.3) for rf, t in zip(roofs, ts)]
            loop = [rf["cycles_per_step_loop"] * (t + 0.3) for rf, t in zip(roofs, ts)]
            at, bt, _ = fit(ts, tot)
            al, bl, _ = fit(ts, loop)
            print("%-8s in-kernel (wave 0 of workgroup 0, cycles): entry -> last store %.0f + %.1f T; step loop %.0f + %.1f T;"
                  " prologue + epilogue %.0f cycles = %.2f us at %.4f GHz"
                  % (label, at, bt, al, bl, float(np.mean(np.array(tot) - np.array(loop))),
                     float(np.mean(np.array(tot) - np.array(loop))) / hz * 1e6, hz / 1e9))
            print("%-8s slope check: wall slope x clock = %.1f cycles per step, step loop %.1f" % (label, b * 1e-6 * hz, bl))


if __name__ == "__main__":
    main(sys.argv[1:])
