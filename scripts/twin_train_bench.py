#!/usr/bin/env python
"""Time of one Twin-L2O training batch (twin.train_batch: per segment the recording forward, the BPTT and the weight-gradient
contraction in HIP, torch.optim.Adam on the host) beside the float32 autograd restatement of the same batch -- the graph of
tests/twin_train_reference.py on device tensors, batched over all rows, torch.optim.Adam on the device -- on the same GPU in
the same process (the yardstick that is not the code under test).

    python scripts/twin_train_bench.py [--processes 3] [--reps 3] [--out profiles/twin_train_bench.txt]

Shapes: seesaw x 128, H = 50 and matrix game 128 x dim 5, H = 80; a batch is 100 iterations with unroll_unit 5, i.e. ten
meta-steps, no curriculum.  Per shape and process: HIP events around each of `reps` whole batches after one warm-up batch;
the HOST part of a batch is inside the bracket (for train_batch: descriptors, uploads, downloads and Adam per segment).
Every batch starts from the same theta and states and continues from the weights the batch before left.  The table gives
every timing.  Every child process runs under its own time limit and the first failure ends the script.  Needs a GPU."""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, loss, instances, dim, hidden)
SHAPES = [("seesaw 128 x 1, H = 50", 3, 128, 1, 50), ("matrix game 128 x 5, H = 80", 4, 128, 5, 80)]
OPTIM_IT, UNROLL_UNIT, RESCALE, META_LR = 100, 5, 1e-4, 1e-4


def torch_batch(torch, kind, data, cells, adams, lr, n_sign, theta, states):
    """do_fit(should_train=True) restated on device tensors: every row in one batch, autograd over each segment."""
    n, _, dim = theta.shape
    u, v = theta[:, 0].clone(), theta[:, 1].clone()
    st = [[t.clone() for t in s] for s in states]
    reward, prev = 0.0, 0.0
    for k in range(1, OPTIM_IT + 1):
        which = (k + 1) % 2
        ud, vd = u.detach(), v.detach()
        if kind == 4:
            gu = torch.matmul(data, vd.unsqueeze(-1)).squeeze(-1)
            gv = torch.matmul(data.transpose(1, 2), ud.unsqueeze(-1)).squeeze(-1)
        else:
            a, b = data[:, 0:1], data[:, 1:2]
            gu = (-1) * b * vd * torch.cos(a * math.pi * ud) * a * math.pi
            gv = (-1) * b * torch.sin(a * math.pi * ud)
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
        if kind == 4:
            f = (u * torch.matmul(data, v.unsqueeze(-1)).squeeze(-1)).sum(dim=1)
        else:
            f = ((-1) * data[:, 1:2] * v * torch.sin(math.pi * u * data[:, 0:1])).sum(dim=1)
        loss = f if which == 0 else (-1) * f
        reward = reward + (loss + prev) / n
        prev = loss.clone()
        if which == 0:
            u = u.detach()
        else:
            v = v.detach()
        if k % (2 * UNROLL_UNIT) == 0:
            for a_ in adams:
                a_.zero_grad()
            reward.sum().backward()
            for a_ in adams:
                a_.step()
            st = [[t.detach() for t in s] for s in st]
            reward, prev = 0.0, 0.0
    return u, v


def child(reps):
    import numpy as np
    import torch
    import __graft_entry__  # noqa: F401
    from open_l2o_amd import _abi, _engine, twin

    if not torch.cuda.is_available():
        raise SystemExit("twin_train_bench: no GPU")
    eng = _engine.HipEngine()
    _engine.set_default_engine(eng)
    n_sign, lr = twin.schedule(OPTIM_IT)

    def timed(fn):
        out = []
        for i in range(reps + 1):                             # (the first batch is the warm-up)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            out.append(a.elapsed_time(b))
        return out[1:]

    res = {"build id": _abi.build_id()}
    for name, kind, n, dim, H in SHAPES:
        rng = np.random.default_rng(1)
        if kind == 4:
            data = (rng.uniform(0.5, 1.0, (n, dim, dim)) * (rng.uniform(size=(n, dim, dim)) < 0.5)).astype(np.float32)
        else:
            data = rng.uniform(0.9, 1.0, (n, 2)).astype(np.float32)
        prob = twin.problem(kind, data, dim)
        mn, mx = twin.Optimizer(H, seed=2), twin.Optimizer(H, seed=3)
        theta0, states0 = twin.draw_start(prob, mn, mx, seed=4)
        cells = []
        for o in (mn, mx):                                    # (before train_batch moves the weights)
            rec1, rec2 = torch.nn.LSTMCell(2, H), torch.nn.LSTMCell(H, H)
            out = torch.nn.Linear(H, 1)
            with torch.no_grad():
                for mod, pre in ((rec1, "recurs."), (rec2, "recurs2."), (out, "output.")):
                    for pn, p in mod.named_parameters():
                        p.copy_(torch.from_numpy(o.params[pre + pn]).reshape(p.shape))
            cells.append(tuple(m.to(eng.device) for m in (rec1, rec2, out)))
        adams = [torch.optim.Adam([p for m in c for p in m.parameters()], lr=META_LR) for c in cells]
        trainer = twin.Trainer(mn, mx, lr=META_LR)
        r = {"twin.train_batch (HIP)": timed(lambda: twin.train_batch(prob, trainer, OPTIM_IT, UNROLL_UNIT, rescale=RESCALE,
                                                                      theta0=theta0, states=states0))}
        data_d, lr_l = eng.tensor(prob.data), [float(x) for x in lr]
        theta_d = eng.tensor(theta0)
        sts = [[eng.tensor(s[j]).t().contiguous() for j in range(4)] for s in states0]
        r["torch float32 autograd, batched"] = timed(lambda: torch_batch(torch, kind, data_d, cells, adams, lr_l, n_sign,
                                                                         theta_d, sts))
        # both sides took reps + 1 batches of ten Adam steps from the same start: the weights they ended with
        w_t = cells[0][1].weight_ih.detach().cpu().numpy()
        r["max |w - torch's| after %d steps" % (10 * (reps + 1))] = float(np.abs(mn.params["recurs2.weight_ih"] - w_t).max())
        r["adam steps"] = float(trainer.step_counts()[0])
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
            raise SystemExit("twin_train_bench: a child failed (exit status %d)" % r.returncode)
        runs.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    lines = ["one Twin-L2O training batch, %d iterations, unroll_unit %d (ten meta-steps), rescale %g: ms per batch, host part "
             "included (HIP events; %d batches after one warm-up batch, every timing), one bracket per process; then the mean"
             % (OPTIM_IT, UNROLL_UNIT, RESCALE, a.reps), "build id " + "  ".join(r.pop("build id") for r in runs)]
    for shape in runs[0]:
        means = {}
        for what, v in runs[0][shape].items():
            if isinstance(v, list):
                every = [x for r in runs for x in r[shape][what]]
                means[what] = sum(every) / len(every)
                lines.append("%-28s %-34s %s   mean %.2f ms" % (
                    shape, what, "  ".join("[" + " ".join("%.2f" % x for x in r[shape][what]) + "]" for r in runs), means[what]))
            else:
                lines.append("%-28s %-34s %s" % (shape, what, "  ".join("%.3g" % r[shape][what] for r in runs)))
        lines.append("%-28s %-34s %.2f" % (shape, "torch / HIP", means["torch float32 autograd, batched"] / means["twin.train_batch (HIP)"]))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
