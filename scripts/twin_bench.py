#!/usr/bin/env python
"""Time of l2o_twin_unroll (the Twin-L2O evaluation unroll, one launch for every iteration of every instance) on the GPU,
beside the float32 torch restatement of the same run, batched over all rows, on the same GPU in the same process (the
yardstick that is not the code under test).

    python scripts/twin_bench.py [--processes 3] [--reps 3] [--out profiles/twin_bench.txt]

Shapes: the reference's seesaw test (500 instances, optim_it 2000, H = 50) and its matrix game (500 instances x dim 5,
optim_it 2000, H = 80), default-initialised networks.  Per shape and process: HIP events around each of `reps` whole runs
after one warm-up run (inputs restored before every run); the table gives every timing, ms per run and us per iteration.
Every child process runs under its own time limit and the first failure ends the script.  Needs a GPU: no fallback."""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, loss, instances, dim, hidden)
SHAPES = [("seesaw 500 x 1, H = 50", 3, 500, 1, 50), ("matrix game 500 x 5, H = 80", 4, 500, 5, 80)]
OPTIM_IT = 2000
RESCALE = 1e-4


def torch_run(torch, kind, data, cells, lr, n_sign, theta, states, n_iter):
    """The run of tests/twin_reference.py restated on device tensors: every row in one batch, two LSTMCell calls and a
    Linear per iteration."""
    n, _, dim = theta.shape
    u, v = theta[:, 0].clone(), theta[:, 1].clone()
    st = [[t.clone() for t in s] for s in states]
    with torch.no_grad():
        for k in range(1, n_iter + 1):
            which = (k + 1) % 2
            if kind == 4:
                gu = torch.matmul(data, v.unsqueeze(-1)).squeeze(-1)
                gv = torch.matmul(data.transpose(1, 2), u.unsqueeze(-1)).squeeze(-1)
            else:
                a, b = data[:, 0:1], data[:, 1:2]
                gu = (-1) * b * v * torch.cos(a * math.pi * u) * a * math.pi
                gv = (-1) * b * torch.sin(a * math.pi * u)
            g, s = (gu, gv) if which == 0 else (gv, gu)
            rec1, rec2, out = cells[which]
            h1, c1, h2, c2 = (RESCALE * t for t in st[which])
            h1, c1 = rec1(torch.cat((g.reshape(-1, 1), s.reshape(-1, 1)), 1), (h1, c1))
            h2, c2 = rec2(h1, (h2, c2))
            st[which] = [h1, c1, h2, c2]
            delta = out(h2).reshape(n, dim)
            step = torch.sign(delta) * lr[k - 1] if k <= n_sign else delta
            if which == 0:
                u = u + step
            else:
                v = v + step
    return u, v


def child(reps):
    import numpy as np
    import torch
    import __graft_entry__  # noqa: F401
    from open_l2o_amd import _abi, _engine, twin

    if not torch.cuda.is_available():
        raise SystemExit("twin_bench: no GPU")
    eng = _engine.HipEngine()
    n_sign, lr = twin.schedule(OPTIM_IT)

    def timed(fn, restore):
        out = []
        for i in range(reps + 1):                             # (the first run is the warm-up)
            restore()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            out.append(a.elapsed_time(b))
        return out[1:]

    res = {}
    for name, kind, n, dim, H in SHAPES:
        rng = np.random.default_rng(1)
        if kind == 4:
            data = (rng.uniform(0.5, 1.0, (n, dim, dim)) * (rng.uniform(size=(n, dim, dim)) < 0.5)).astype(np.float32)
        else:
            data = rng.uniform(0.9, 1.0, (n, 2)).astype(np.float32)
        prob = twin.problem(kind, data, dim)
        mn, mx = twin.Optimizer(H, seed=2), twin.Optimizer(H, seed=3)
        theta0, states0 = twin.draw_start(prob, mn, mx, seed=4)
        dev = _engine.TwinDevice(eng, tuple((o.hidden_size, o.n_in, o.params) for o in (mn, mx)), (kind, n, dim, prob.data),
                                 dict(iter0=1, n_iter=OPTIM_IT, n_sign=n_sign, rescale=RESCALE, out_mul=1.0, sign_lr=lr))
        keep = [eng.tensor(theta0)] + [eng.tensor(s) for s in states0]
        bufs = [t.clone() for t in keep]
        curve = eng.empty(OPTIM_IT, n, 2 * dim)

        def restore():
            for b, k in zip(bufs, keep):
                b.copy_(k)

        def launch(curve=None):
            rc = dev.unroll(*bufs, curve, None, None, eng._stream())
            if rc != _abi.L2O_OK:
                raise SystemExit("twin_bench: l2o_twin_unroll returned %d" % rc)

        r = {"l2o_twin_unroll": timed(launch, restore), "l2o_twin_unroll + curve": timed(lambda: launch(curve), restore)}
        cells = []
        for o in (mn, mx):
            rec1, rec2 = torch.nn.LSTMCell(2, H), torch.nn.LSTMCell(H, H)
            out = torch.nn.Linear(H, 1)
            with torch.no_grad():
                for mod, pre in ((rec1, "recurs."), (rec2, "recurs2."), (out, "output.")):
                    for pn, p in mod.named_parameters():
                        p.copy_(torch.from_numpy(o.params[pre + pn]).reshape(p.shape))
            cells.append(tuple(m.to(eng.device) for m in (rec1, rec2, out)))
        data_d, lr_l = eng.tensor(prob.data), [float(x) for x in lr]
        sts = [[s[j].t().contiguous() for j in range(4)] for s in keep[1:]]
        end = {}

        def torch_whole():
            end["uv"] = torch_run(torch, kind, data_d, cells, lr_l, n_sign, keep[0], sts, OPTIM_IT)

        r["torch float32, batched"] = timed(torch_whole, lambda: None)
        restore()
        launch()
        torch.cuda.synchronize()
        uv = torch.stack(end["uv"], 1)
        ok = torch.isfinite(uv) & torch.isfinite(bufs[0])
        r["finite rows"] = float(ok.flatten(1).all(dim=1).float().mean())
        r["max |theta - torch| over finite rows"] = float((uv - bufs[0]).abs()[ok].max()) if bool(ok.any()) else float("nan")
        res[name] = r
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.reps)
    runs = []
    for _ in range(a.processes):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps)], cwd=ROOT,
                           capture_output=True, text=True, timeout=240)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit("twin_bench: a child failed (exit status %d)" % r.returncode)
        runs.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    lines = ["l2o_twin_unroll, optim_it %d, rescale %g: ms per run (HIP events; %d runs after one warm-up run, every timing), "
             "one bracket per process; then the mean in us per iteration" % (OPTIM_IT, RESCALE, a.reps)]
    for shape in runs[0]:
        for what, v in runs[0][shape].items():
            if isinstance(v, list):
                every = [x for r in runs for x in r[shape][what]]
                lines.append("%-28s %-26s %s   mean %.2f us / iteration" % (
                    shape, what, "  ".join("[" + " ".join("%.2f" % x for x in r[shape][what]) + "]" for r in runs),
                    1e3 * sum(every) / len(every) / OPTIM_IT))
            else:
                lines.append("%-28s %-26s %s" % (shape, what, "  ".join("%.3g" % r[shape][what] for r in runs)))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
