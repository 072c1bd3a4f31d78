#!/usr/bin/env python
"""Time of one l2o_klstm_step (networks.KernelDeepLSTM's forward step) and of one l2o_klstm_bwd_step on the GPU, beside the
float32 torch restatement of the same step on the same GPU in the same run (the yardstick that is not the code under test).

    python scripts/klstm_step_bench.py [--processes 3] [--iters 200] [--out profiles/<file>.txt]

Per shape: HIP events around `iters` back-to-back launches after a warm-up, in `processes` fresh child processes (this parent
never opens the GPU); the table gives every process's mean per launch in microseconds.  Needs a GPU: no fallback."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# mnist_conv's second filter and vgg16's widest, both under the default net of the tests: (20, 20), LogAndSign(k = 5)
SHAPES = [(5, 5, 16, 32), (3, 3, 512, 512)]
LAYERS = (20, 20)


def torch_step(feats_of, p, g, st, K, N, scale):
    """The step of tests/kernel_lstm_reference.py, restated on device tensors."""
    import torch
    x = feats_of(g.view(K, N).t())
    new = []
    for l, (h, c) in enumerate(st):
        H = h.shape[1]
        z = torch.cat([x, h], 1) @ p["lstm_%d" % (l + 1)]["w_gates"] + p["lstm_%d" % (l + 1)]["b_gates"]
        cn = torch.sigmoid(z[:, 2 * H:3 * H] + 1.0) * c + torch.sigmoid(z[:, :H]) * torch.tanh(z[:, H:2 * H])
        new.append((torch.tanh(cn) * torch.sigmoid(z[:, 3 * H:]), cn))
        x = new[-1][0]
    return scale * (x @ p["linear"]["w"] + p["linear"]["b"]).t(), new


def child(iters):
    import numpy as np
    import torch
    import __graft_entry__  # noqa: F401
    from open_l2o_amd import _engine, networks

    if not torch.cuda.is_available():
        raise SystemExit("klstm_step_bench: no GPU")
    eng = _engine.HipEngine()
    eps, k = float(np.finfo(np.float32).eps), 5.0

    def feats_of(x):
        log = torch.clamp(torch.log(x.abs() + eps) / k, min=-1.0)
        return torch.stack([log, torch.clamp(x * float(np.exp(k)), -1.0, 1.0)], 2).reshape(x.shape[0], -1)

    def timed(fn):
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / iters

    out = {}
    for shape in SHAPES:
        K, N = shape[0] * shape[1], shape[2] * shape[3]
        networks.set_random_seed(1)
        net = networks.KernelDeepLSTM(shape[:2], LAYERS, preprocess_name="LogAndSign", preprocess_options={"k": 5}, scale=0.01)
        rng = np.random.default_rng(2)
        g = eng.tensor(rng.normal(size=K * N))
        x = eng.zeros(K * N)
        ns = 2 * N * sum(LAYERS)
        st = eng.tensor(rng.normal(0, 0.5, ns))
        st2 = eng.empty(ns)
        res = {"klstm_step": timed(lambda: eng.klstm_step(net, g, st, st2, x, N))}
        Hs = list(LAYERS)
        ins = [net.in_dim] + Hs[:-1]
        io = dict(g=g, dx_next=eng.tensor(rng.normal(size=K * N)), st_prev=st, carry_in=eng.zeros(ns), carry_out=eng.empty(ns),
                  act=[eng.empty(N, a + h) for a, h in zip(ins, Hs)], dz=[eng.empty(N, 4 * h) for h in Hs],
                  tc=eng.empty(N * sum(Hs)), h_last=eng.empty(N, Hs[-1]), dd=eng.empty(N, K))
        res["klstm_bwd_step"] = timed(lambda: eng.klstm_bwd_step(net, io, N))
        p = {m: {v: eng.tensor(a) for v, a in d.items()} for m, d in net.variables.items()}
        sts, off = [], 0
        for H in Hs:
            sts.append((st[off:off + H * N].view(H, N).t().contiguous(), st[off + H * N:off + 2 * H * N].view(H, N).t().contiguous()))
            off += 2 * H * N
        res["torch_float32_step"] = timed(lambda: torch_step(feats_of, p, g, sts, K, N, 0.01))
        # the bytes a step has to move (g, x in and out, state in and out) over the kernel's time
        res["klstm_step_GBps"] = 4.0 * (3 * K * N + 2 * ns) / res["klstm_step"] / 1e3
        out["x".join(str(d) for d in shape)] = res
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.iters)
    runs = []
    for _ in range(a.processes):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--iters", str(a.iters)], cwd=ROOT,
                           capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit("klstm_step_bench: a child failed (exit status %d)" % r.returncode)
        runs.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    lines = ["l2o_klstm_step / l2o_klstm_bwd_step, layers %r, LogAndSign(k=5); microseconds per launch (HIP events, %d launches "
             "after a warm-up of 20), one column per process" % (LAYERS, a.iters)]
    for shape in runs[0]:
        for what in runs[0][shape]:
            lines.append("%-14s %-20s %s" % (shape, what, "  ".join("%10.2f" % r[shape][what] for r in runs)))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
