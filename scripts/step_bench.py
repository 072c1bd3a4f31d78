"""Time one step-path optimizee on the GPU, in one process, with HIP events after a warm-up:

  * fg_us: us per evaluation through the engine -- loss and all gradients (the image nets: of one minibatch, batch norm on,
    the reference's default; confocal: simulation mode, and forward only as forward_only_us);
  * step_us: us per optimizer step -- one unroll of meta_loss over util.get_config(<problem>) (its default coordinate-wise
    net over all coordinates) on the step-granular path, divided by its length: per step the fg, the LSTM step and, for the
    image nets, the minibatch draw;
  * lenet and confocal, as the yardstick that is not the code under test: the same loss and gradients through float32 torch
    autograd on the same GPU, timed the same way (lenet: conv2d / max_pool2d / matmul of the installed torch, batch norm
    from var_mean; confocal: torch.erf on the separable tables, one einsum per point);
  * confocal: the per-kernel split comes from the device, in a run of its own: ``--loop N`` runs N bare evaluations and
    nothing else, for ``rocprofv3 --kernel-trace --stats -- python scripts/step_bench.py --problem confocal --loop 2000``;
  * confocal with ``--fused 1 --replicas N``: nothing but N fused unrolls as ONE launch (replicas.Replicas, form "rows":
    rows_step_us_per_instance) against the same N replicas as N single fused launches (the yardstick:
    single_step_us_per_instance) -- us per optimizer step per instance, the median of 10 event-timed rounds each;
  * vgg16: three runs in one process of fg_us (l2o_vgg16_fg), the float32 torch-autograd yardstick (conv2d / max_pool2d of
    the installed torch: MIOpen and rocBLAS, which may pick Winograd) and step_us (fg, 28 l2o_cwlstm_step launches and the
    minibatch draw), at the reference's widths unless ``--channels`` narrows them; ``--loop N`` runs N bare evaluations and
    one short unroll and nothing else, for a kernel trace;
  * nas: three runs in one process of fg_us (l2o_nas_fg), the float32 torch-autograd yardstick (conv2d,
    avg_pool2d(count_include_pad=False) and batch norm by hand from var_mean) and step_us (fg, 18 l2o_cwlstm_step launches
    and the minibatch draw); ``--loop N`` runs N bare evaluations and one short unroll and nothing else, for a kernel trace;
  * mnist with ``--hvp 1``: us per l2o_mlp_hvp (784-20-10, the Hessian-vector product of second_derivatives=True) against
    l2o_mlp_deep_fg of the same shape and against the same H u through float32 torch double backward on the same GPU, three
    event-timed runs each; and one meta_minimize train step at --unroll steps with and without second_derivatives, and with
    the flag but the Hessian-vector products left out (what of the extra time is the T products, what the un-fused
    recording and BPTT).

    python scripts/step_bench.py --problem {mnist_conv,cifar_conv,lenet} [--batch 128] [--iters 200] [--unroll 20] [--unrolls 10]
    python scripts/step_bench.py --problem confocal [--batch 32] [--points 5] [--roi 28] [--iters 500] [--unroll 20] [--fused 1]
                                 [--unrolls 10] [--loop N] [--replicas N]
    python scripts/step_bench.py --problem vgg16 [--batch 128] [--channels 64,128,256,512,512] [--iters 20] [--unroll 5]
                                 [--unrolls 3] [--loop N]
    python scripts/step_bench.py --problem nas [--batch 128] [--iters 200] [--unroll 20] [--unrolls 10] [--loop N]
    python scripts/step_bench.py --problem mnist --hvp 1 [--batch 128] [--iters 200] [--unroll 20] [--unrolls 10]

Prints one JSON line.  The image nets run on synthetic data (problems.synthetic_mnist / synthetic_cifar10); the arithmetic
does not depend on it."""
import argparse
import functools
import json
import math
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from open_l2o_amd import _engine, meta, problems, util  # noqa: E402
from open_l2o_amd.session import Session  # noqa: E402

_CONV_SHAPES = [(16,), (16,), (16,), (5, 5, 16, 32), (32,), (32,), (32,)]
# per image net: its data, descriptor and engine method, the variable shapes with batch norm, and which of them start at
# a constant (gamma at 1; LeNet's batch norm has only an offset, at 0)
IMAGE_NETS = {
    "mnist_conv": types.SimpleNamespace(
        data=problems.synthetic_mnist, desc=_engine.MnistConvDesc, fg="mnist_conv_fg", const=((2, 6), 1.0),
        shapes=[(3, 3, 1, 16)] + _CONV_SHAPES + [(512, 10), (10,)]),
    "cifar_conv": types.SimpleNamespace(
        data=problems.synthetic_cifar10, desc=_engine.CifarConvDesc, fg="cifar_conv_fg", const=((2, 6), 1.0),
        shapes=[(3, 3, 3, 16)] + _CONV_SHAPES + [(32, 10), (10,)]),
    "lenet": types.SimpleNamespace(
        data=problems.synthetic_cifar10, desc=_engine.LenetDesc, fg="lenet_fg", const=((2, 5, 8, 11), 0.0),
        shapes=[(5, 5, 3, 6), (6,), (6,), (5, 5, 6, 16), (16,), (16,), (400, 120), (120,), (120,), (120, 84), (84,), (84,),
                (84, 10), (10,)]),
}


def _timed(fn, iters, warmup=20):
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


def time_step(config, options, T, unrolls, warmup=2):
    problem, net_config, na = util.get_config(config, problem_options=options)
    optimizer = meta.MetaOptimizer(**net_config)
    ml = optimizer.meta_loss(problem, T, net_assignments=na)
    graph = optimizer.graph
    times = []
    with Session() as sess:
        sess.run(ml.reset)
        for k in range(warmup + unrolls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            graph.launch({}, commit=True, events=(e0, e1))
            e1.synchronize()
            if k >= warmup:
                times.append(1e3 * e0.elapsed_time(e1) / T)
    return float(np.median(times)), graph


# -- the image nets ----------------------------------------------------------------------------------------------------
def image_net_fg(eng, net, data, batch):
    """One evaluation as a callable, its loss buffer, and the minibatch and weights on the host (for the yardstick)."""
    images = np.ascontiguousarray(data["images"], np.float32).reshape(len(data["labels"]), -1)
    d = net.desc(batch, True, eng.tensor(images), eng.int_tensor(data["labels"]))
    rng = np.random.default_rng(0)
    rows = rng.integers(0, len(images), batch)
    idx = eng.int_tensor(rows)
    w = [rng.normal(0, 0.01, sh).astype(np.float32) for sh in net.shapes]
    for k in net.const[0]:
        w[k][:] = net.const[1]
    ws = [eng.tensor(a) for a in w]
    grads = [eng.zeros(*sh) for sh in net.shapes]
    loss = eng.zeros(1)
    fg = functools.partial(getattr(eng, net.fg), d, idx, ws, loss, grads)
    return fg, loss, (images[rows], np.asarray(data["labels"])[rows], w)


def lenet_torch(x, y, w, iters):
    """LeNet through float32 torch autograd on the GPU."""
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

    us = _timed(fg, iters)
    return us, float(out["loss"])


def image_net_main(eng, a):
    net = IMAGE_NETS[a.problem]
    data = net.data(4096, seed=0)
    fg, loss, (x, y, w) = image_net_fg(eng, net, data, a.batch)
    fg_us = _timed(fg, a.iters)
    yardstick = {}
    if a.problem == "lenet":
        torch_us, torch_loss = lenet_torch(x, y, w, a.iters)
        yardstick = {"torch_autograd_fg_us": round(torch_us, 2), "loss": float(eng.to_numpy(loss)[0]), "torch_loss": torch_loss}
    step_us, graph = time_step(a.problem, {"data": data, "batch_size": a.batch}, a.unroll, a.unrolls)
    return {"workload": a.problem, "batch": a.batch, "coordinates": sum(int(np.prod(v.shape)) for v in graph.x),
            "fg_us": round(fg_us, 2), **yardstick, "step_us": round(step_us, 2), "unroll": a.unroll, "path": graph.last_path,
            "device": torch.cuda.get_device_name(0)}


# -- vgg16 -------------------------------------------------------------------------------------------------------------
def vgg16_shapes(channels):
    shapes, c_in = [], 3
    for n, c in zip((2, 2, 3, 3, 3), channels):
        for _ in range(n):
            shapes += [(3, 3, c_in, c), (c,)]
            c_in = c
    return shapes + [(c_in, 10), (10,)]


def vgg16_torch(x, y, w, iters):
    """VGG-16 through float32 torch autograd on the GPU."""
    dev = torch.device("cuda")
    x = torch.tensor(x, device=dev).reshape(-1, 32, 32, 3).permute(0, 3, 1, 2).contiguous()
    y = torch.tensor(y, device=dev, dtype=torch.int64)
    vs = [torch.tensor(a, device=dev).requires_grad_(True) for a in w]
    out = {}

    def fg():
        h, k = x, 0
        for n in (2, 2, 3, 3, 3):
            for _ in range(n):
                h = F.relu(F.conv2d(h, vs[k].permute(3, 2, 0, 1), vs[k + 1], padding=1))
                k += 2
            h = F.max_pool2d(h, 2)
        z = h.reshape(h.shape[0], -1) @ vs[26] + vs[27]
        loss = F.cross_entropy(F.softmax(z, dim=1), y)
        out["loss"], out["grads"] = loss, torch.autograd.grad(loss, vs)

    us = _timed(fg, iters, warmup=5)
    return us, float(out["loss"])


def vgg16_main(eng, a):
    channels = tuple(int(c) for c in a.channels.split(","))
    shapes = vgg16_shapes(channels)
    data = problems.synthetic_cifar10(4096, seed=0)
    images = np.ascontiguousarray(data["images"], np.float32).reshape(len(data["labels"]), -1)
    d = _engine.Vgg16Desc(a.batch, channels, eng.tensor(images), eng.int_tensor(data["labels"]))
    rng = np.random.default_rng(0)
    rows = rng.integers(0, len(images), a.batch)
    idx = eng.int_tensor(rows)
    # O(1) activations (at the reference's initialisation the float32 logits are exactly the bias): He-scaled weights
    w = [rng.normal(0, math.sqrt(2.0 / (9 * sh[2])) if len(sh) == 4 else (1.0 / math.sqrt(sh[0]) if len(sh) == 2 else 0.1),
                    sh).astype(np.float32) for sh in shapes]
    ws, grads, loss = [eng.tensor(t) for t in w], [eng.zeros(*sh) for sh in shapes], eng.zeros(1)
    fg = functools.partial(eng.vgg16_fg, d, idx, ws, loss, grads)
    options = {"data": data, "batch_size": a.batch, "channels": channels}
    if a.loop:
        fg_us = _timed(fg, a.loop, warmup=2)
        step_us, _ = time_step("vgg16", options, 2, 1, warmup=1)
        return {"workload": "vgg16", "loop": a.loop, "fg_us": round(fg_us, 2), "step_us": round(step_us, 2)}
    runs = []
    for _ in range(3):
        fg_us = _timed(fg, a.iters, warmup=3)
        torch_us, torch_loss = vgg16_torch(images[rows], np.asarray(data["labels"])[rows], w, a.iters)
        step_us, graph = time_step("vgg16", options, a.unroll, a.unrolls, warmup=1)
        runs.append({"fg_us": round(fg_us, 2), "torch_autograd_fg_us": round(torch_us, 2), "step_us": round(step_us, 2)})
    return {"workload": "vgg16", "batch": a.batch, "channels": list(channels),
            "coordinates": sum(int(np.prod(v.shape)) for v in graph.x), "runs": runs,
            "loss": float(eng.to_numpy(loss)[0]), "torch_loss": torch_loss, "unroll": a.unroll, "path": graph.last_path,
            "device": torch.cuda.get_device_name(0)}


# -- nas ---------------------------------------------------------------------------------------------------------------
NAS_SHAPES = [sh for i in range(4) for sh in ((3, 3, 3 if i == 0 else 16, 16), (16,), (16,), (16,))] + [(16, 10), (10,)]


def nas_torch(x, y, w, iters):
    """The NAS cell with batch norm through float32 torch autograd on the GPU."""
    dev = torch.device("cuda")
    x = torch.tensor(x, device=dev).reshape(-1, 32, 32, 3).permute(0, 3, 1, 2).contiguous()
    y = torch.tensor(y, device=dev, dtype=torch.int64)
    vs = [torch.tensor(a, device=dev).requires_grad_(True) for a in w]
    out = {}

    def layer(h, k):                        # batch statistics, biased variance, eps 1e-3
        z = F.conv2d(h, vs[k].permute(3, 2, 0, 1), vs[k + 1], padding=1)
        var, mean = torch.var_mean(z, (0, 2, 3), unbiased=False, keepdim=True)
        return F.relu((z - mean) * torch.rsqrt(var + 1e-3) * vs[k + 2].view(1, -1, 1, 1) + vs[k + 3].view(1, -1, 1, 1))

    def fg():
        node0 = layer(x, 0)
        n02, node1 = layer(node0, 4), layer(node0, 8)
        n13 = layer(node1, 12)
        node3 = F.avg_pool2d(node1, 3, stride=1, padding=1, count_include_pad=False) + n02 + n13 + node0
        loss = F.cross_entropy(F.relu(node3.mean(dim=(2, 3)) @ vs[16] + vs[17]), y)
        out["loss"], out["grads"] = loss, torch.autograd.grad(loss, vs)

    us = _timed(fg, iters)
    return us, float(out["loss"])


def nas_main(eng, a):
    data = problems.synthetic_cifar10(4096, seed=0)
    images = np.ascontiguousarray(data["images"], np.float32).reshape(len(data["labels"]), -1)
    d = _engine.NasDesc(a.batch, True, eng.tensor(images), eng.int_tensor(data["labels"]))
    rng = np.random.default_rng(0)
    rows = rng.integers(0, len(images), a.batch)
    idx = eng.int_tensor(rows)
    # O(1) activations and logits on both sides of their ReLU: He-scaled conv weights, gamma 1, fc weights of std 1
    w = [rng.normal(0, math.sqrt(2.0 / (9 * sh[2])) if len(sh) == 4 else (1.0 if len(sh) == 2 else 0.1), sh).astype(np.float32)
         for sh in NAS_SHAPES]
    for k in (2, 6, 10, 14):
        w[k][:] = 1.0
    ws, grads, loss = [eng.tensor(t) for t in w], [eng.zeros(*sh) for sh in NAS_SHAPES], eng.zeros(1)
    fg = functools.partial(eng.nas_fg, d, idx, ws, loss, grads)
    options = {"data": data, "batch_size": a.batch}
    if a.loop:
        fg_us = _timed(fg, a.loop, warmup=5)
        step_us, _ = time_step("nas", options, 2, 1, warmup=1)
        return {"workload": "nas", "loop": a.loop, "fg_us": round(fg_us, 2), "step_us": round(step_us, 2)}
    runs = []
    for _ in range(3):
        fg_us = _timed(fg, a.iters)
        torch_us, torch_loss = nas_torch(images[rows], np.asarray(data["labels"])[rows], w, a.iters)
        step_us, graph = time_step("nas", options, a.unroll, a.unrolls)
        runs.append({"fg_us": round(fg_us, 2), "torch_autograd_fg_us": round(torch_us, 2), "step_us": round(step_us, 2)})
    return {"workload": "nas", "batch": a.batch, "coordinates": sum(int(np.prod(v.shape)) for v in graph.x), "runs": runs,
            "loss": float(eng.to_numpy(loss)[0]), "torch_loss": torch_loss, "unroll": a.unroll, "path": graph.last_path,
            "device": torch.cuda.get_device_name(0)}


# -- confocal ----------------------------------------------------------------------------------------------------------
def confocal_fg(eng, batch, points, roi, want_grad=True):
    rng = np.random.default_rng(0)
    nv = 6 * points + 1
    theta = [rng.random(batch).astype(np.float32) for _ in range(nv)]
    sim = [rng.random(batch).astype(np.float32) for _ in range(nv)]
    d = _engine.ConfocalDesc(batch, points, roi)
    th, sm = [eng.tensor(a) for a in theta], [eng.tensor(a) for a in sim]
    grads = [eng.zeros(batch) for _ in theta] if want_grad else None
    loss = eng.zeros(1)
    return (lambda: eng.confocal_fg(d, th, sm, loss, grads)), loss, (theta, sim)


def confocal_torch(theta, sim, points, roi, iters):
    """The confocal loss and gradients through float32 torch autograd on the GPU."""
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

    us = _timed(fg, iters)
    return us, float(out["loss"].detach())


def confocal_replicas(a):
    """N fused unrolls as one rows launch, and the same N replicas as N single fused launches: us per optimizer step per
    instance, medians of `rounds` event-timed rounds after a warm-up, the two forms alternating in one process."""
    from open_l2o_amd.replicas import Replicas
    roi, N, T, rounds = [a.roi] * 3, a.replicas, a.unroll, 10
    problem, net_config, na = util.get_config("confocal_microscopy_3d", problem_options={
        "batch_size": a.batch, "num_points": a.points, "ROI": roi, "fused": True})
    reps = Replicas(meta.MetaOptimizer(**net_config), [problem] * N, T, na)
    reps.reset()
    if not reps.rows_supported():
        raise SystemExit("step_bench: form 'rows' does not apply")

    def rows():
        reps.launch({})

    def singles():
        for g in reps.graphs:
            g.launch({}, commit=True)
    times = {"rows": [], "single": []}
    for k in range(2 + rounds):
        for name, fn in (("rows", rows), ("single", singles)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if k >= 2:
                times[name].append(1e3 * e0.elapsed_time(e1) / (T * N))
        if k == 0:
            forms = (reps.last_form, reps.graphs[0].last_path)
    assert forms == ("rows", "confocal_unroll"), forms
    return {"workload": "confocal_microscopy_3d", "batch": a.batch, "points": a.points, "roi": roi, "replicas": N,
            "unroll": T, "rounds": rounds, "rows_step_us_per_instance": round(float(np.median(times["rows"])), 2),
            "single_step_us_per_instance": round(float(np.median(times["single"])), 2),
            "rows_min_max": [round(min(times["rows"]), 2), round(max(times["rows"]), 2)],
            "single_min_max": [round(min(times["single"]), 2), round(max(times["single"]), 2)],
            "workgroups_per_rows_launch": N * a.batch, "device": torch.cuda.get_device_name(0)}


def confocal_main(eng, a):
    if a.replicas:
        if not a.fused:
            raise SystemExit("step_bench: --replicas needs --fused 1")
        return confocal_replicas(a)
    roi = (a.roi, a.roi, a.roi)
    fg, loss, (theta, sim) = confocal_fg(eng, a.batch, a.points, roi)
    if a.loop:
        for _ in range(a.loop):
            fg()
        torch.cuda.synchronize()
        return {"workload": "confocal_microscopy_3d", "loop": a.loop, "loss": float(eng.to_numpy(loss)[0])}
    fg_us = _timed(fg, a.iters)
    f_us = _timed(confocal_fg(eng, a.batch, a.points, roi, want_grad=False)[0], a.iters)
    torch_us, torch_loss = confocal_torch(theta, sim, a.points, roi, a.iters)
    calls = [0]
    orig_fg = eng.confocal_fg

    def counted(*args, **kw):
        calls[0] += 1
        return orig_fg(*args, **kw)
    eng.confocal_fg = counted
    step_us, graph = time_step("confocal_microscopy_3d", {"batch_size": a.batch, "num_points": a.points, "ROI": list(roi)},
                               a.unroll, a.unrolls)
    del eng.confocal_fg
    assert calls[0] == (2 + a.unrolls) * (a.unroll + 1)
    fused = {}
    if a.fused:                                              # the same unroll as ONE launch, timed in the same process
        fused_us, fgraph = time_step("confocal_microscopy_3d", {"batch_size": a.batch, "num_points": a.points, "ROI": list(roi),
                                                                "fused": True}, a.unroll, a.unrolls)
        fused = {"fused_step_us": round(fused_us, 2), "fused_path": fgraph.last_path}
    nvar = len(graph.x)
    lstm_launches = -(-nvar // eng.MAX_STEP_SEGS)            # l2o_cwlstm_step_multi takes MAX_STEP_SEGS variables per launch
    return {"workload": "confocal_microscopy_3d", "batch": a.batch, "points": a.points, "roi": list(roi),
            "variables": nvar, "fg_us": round(fg_us, 2), "forward_only_us": round(f_us, 2),
            "torch_autograd_fg_us": round(torch_us, 2), "loss": float(eng.to_numpy(loss)[0]),
            "torch_loss": torch_loss, "step_us": round(step_us, 2), "unroll": a.unroll, "path": graph.last_path, **fused,
            "launches_per_step": {"l2o_confocal_fg": 2, "l2o_cwlstm_step_multi": lstm_launches},
            "device": torch.cuda.get_device_name(0)}


# -- the MLP optimizee's Hessian-vector product ------------------------------------------------------------------------------
def mnist_hvp_torch(x, y, w, u, iters):
    """H u of the 784-20-10 sigmoid MLP's mean cross-entropy through float32 torch double backward on the GPU."""
    dev = torch.device("cuda")
    x, y = torch.tensor(x, device=dev), torch.tensor(y, device=dev, dtype=torch.int64)
    vs = [torch.tensor(a, device=dev).requires_grad_(True) for a in w]
    us = [torch.tensor(a, device=dev) for a in u]
    out = {}

    def hvp():
        loss = F.cross_entropy(torch.sigmoid(x @ vs[0] + vs[1]) @ vs[2] + vs[3], y)
        g = torch.autograd.grad(loss, vs, create_graph=True)
        out["hu"] = torch.autograd.grad(sum((a * b).sum() for a, b in zip(g, us)), vs)
    times = [_timed(hvp, iters) for _ in range(3)]
    return times, [t.detach().cpu().numpy() for t in out["hu"]]


def time_train_step(data, batch, T, second, steps, warmup=3, no_hvp=False):
    """us per sess.run([fx, update, step]) of meta_minimize on problems.mnist (the default net), a device synchronise at
    both ends; no_hvp: with the flag, but engine.mlp_hvp replaced by a fill (the recording and the BPTT without the products)."""
    import time
    problem, net_config, na = util.get_config("mnist", problem_options={"data": data, "batch_size": batch})
    optimizer = meta.MetaOptimizer(**net_config)
    ms = optimizer.meta_minimize(problem, T, net_assignments=na, learning_rate=1e-4, second_derivatives=second)
    eng = optimizer.graph.engine
    if no_hvp:
        eng.mlp_hvp = lambda d, idx, ws, us, outs: [o.zero_() for o in outs]
    times = []
    try:
        with Session() as sess:
            sess.run(ms.reset)
            for k in range(warmup + steps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                sess.run([ms.fx, ms.update, ms.step])
                torch.cuda.synchronize()
                if k >= warmup:
                    times.append(1e6 * (time.perf_counter() - t0))
    finally:
        if no_hvp:
            del eng.mlp_hvp
    return times, optimizer.graph.last_path


def mnist_hvp_main(eng, a):
    hidden, n_out = (20,), 10
    data = problems.synthetic_mnist(4096, seed=0, label_noise=0.1)
    images = np.ascontiguousarray(data["images"], np.float32).reshape(len(data["labels"]), -1)
    d = _engine.MlpDeepDesc(n_in=images.shape[1], hidden=hidden, n_out=n_out, batch=a.batch, activation=0,
                            images=eng.tensor(images), labels=eng.int_tensor(data["labels"]))
    rng = np.random.default_rng(0)
    rows = rng.integers(0, len(images), a.batch)
    shapes = [(images.shape[1], hidden[0]), (hidden[0],), (hidden[0], n_out), (n_out,)]
    w = [rng.normal(0, 0.3, sh).astype(np.float32) for sh in shapes]
    u = [rng.normal(0, 1.0, sh).astype(np.float32) for sh in shapes]
    idx, ws, us = eng.int_tensor(rows), [eng.tensor(x) for x in w], [eng.tensor(x) for x in u]
    outs, grads, loss = [eng.zeros(*sh) for sh in shapes], [eng.zeros(*sh) for sh in shapes], eng.zeros(1)
    hvp = functools.partial(eng.mlp_hvp, d, idx, ws, us, outs)
    fg = functools.partial(eng.mlp_deep_fg, d, idx, ws, loss, grads)
    hvp_us, fg_us = [], []
    for _ in range(3):                                       # the two alternate
        hvp_us.append(_timed(hvp, a.iters))
        fg_us.append(_timed(fg, a.iters))
    torch_us, torch_hu = mnist_hvp_torch(images[rows], np.asarray(data["labels"])[rows], w, u, a.iters)
    err = max(float(np.abs(eng.to_numpy(o) - t).max() / np.abs(t).max()) for o, t in zip(outs, torch_hu))
    steps = {}
    for name, kw in (("first_order", dict(second=False)), ("second", dict(second=True)),
                     ("second_without_hvp", dict(second=True, no_hvp=True))):
        times, path = time_train_step(data, a.batch, a.unroll, steps=a.unrolls, **kw)
        steps[name] = {"train_step_us": round(float(np.median(times)), 1),
                       "min_max": [round(min(times), 1), round(max(times), 1)], "path": path}
    extra = steps["second"]["train_step_us"] - steps["first_order"]["train_step_us"]
    in_hvp = steps["second"]["train_step_us"] - steps["second_without_hvp"]["train_step_us"]
    r = lambda xs: [round(x, 2) for x in xs]
    return {"workload": "mnist_hvp", "shape": [images.shape[1], hidden[0], n_out], "batch": a.batch, "iters": a.iters,
            "mlp_hvp_us": r(hvp_us), "mlp_deep_fg_us": r(fg_us), "torch_double_backward_us": r(torch_us),
            "hvp_over_fg": round(float(np.median(hvp_us) / np.median(fg_us)), 2), "max_rel_diff_vs_torch_f32": err,
            "unroll": a.unroll, "train_steps": steps, "extra_us": round(extra, 1), "extra_in_hvp_calls_us": round(in_hvp, 1),
            "hvp_share_of_extra": round(in_hvp / extra, 3) if extra > 0 else None, "device": torch.cuda.get_device_name(0)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--problem", required=True, choices=list(IMAGE_NETS) + ["vgg16", "nas", "confocal", "mnist"])
    p.add_argument("--hvp", type=int, choices=(0, 1), default=0,
                   help="mnist: time l2o_mlp_hvp against l2o_mlp_deep_fg and torch double backward, and the train step")
    p.add_argument("--batch", type=int, help="default: 128; confocal: 32")
    p.add_argument("--iters", type=int, help="default: 200; confocal: 500")
    p.add_argument("--unroll", type=int, help="default: 20; vgg16: 5")
    p.add_argument("--unrolls", type=int, help="default: 10; vgg16: 3")
    p.add_argument("--channels", default="64,128,256,512,512", help="vgg16: the widths of the five blocks")
    p.add_argument("--points", type=int, default=5, help="confocal")
    p.add_argument("--roi", type=int, default=28, help="confocal")
    p.add_argument("--fused", type=int, choices=(0, 1), default=0,
                   help="confocal: 1 also times the fused unroll (fused_step_us) beside the step path (step_us)")
    p.add_argument("--loop", type=int, default=0, help="confocal, vgg16, nas: only run this many bare evaluations (for a kernel trace)")
    p.add_argument("--replicas", type=int, default=0,
                   help="confocal, with --fused 1: time N fused unrolls as one launch against N single launches, nothing else")
    a = p.parse_args()
    confocal = a.problem == "confocal"
    a.batch = a.batch or (32 if confocal else 128)
    a.iters = a.iters or (500 if confocal else 20 if a.problem == "vgg16" else 200)
    a.unroll = a.unroll or (5 if a.problem == "vgg16" else 20)
    a.unrolls = a.unrolls or (3 if a.problem == "vgg16" else 10)
    if a.problem == "mnist" and not a.hvp:
        raise SystemExit("step_bench: --problem mnist measures the Hessian-vector product: give --hvp 1")
    eng = _engine.HipEngine()
    _engine.set_default_engine(eng)
    meta.set_random_seed(0)
    run = confocal_main if confocal else {"mnist": mnist_hvp_main, "vgg16": vgg16_main, "nas": nas_main}.get(a.problem, image_net_main)
    print(json.dumps(run(eng, a)))


if __name__ == "__main__":
    main()
