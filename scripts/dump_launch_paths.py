"""What UnrollGraph.launch computes on each of its paths, as one .npz -- to hold two trees against each other bit for bit:

    python scripts/dump_launch_paths.py --engine {oracle,hip} --out FILE.npz
    python scripts/dump_launch_paths.py --compare A.npz B.npz          (np.array_equal on every array; exit status 1 if not)

The cells are those of tests/test_launch_paths_cpu.py, on an engine that computes: plain (committed and not), recording,
gradients() (a recording launch of zero steps), restart=x0, L2O_DISABLE_FUSED, second derivatives, a fed RNNProp step, a fed
x-scale (the same array twice, then a new one), problems.mnist (plain, recording, and recording under
L2O_NO_MLP_UNROLL_RECORD / L2O_MLP_UNROLL_RECORD_GENERIC) and problems.confocal_microscopy_3d (fused and not).  Per launch:
fx[0..T] and every x_T, a recording launch's g_final, and per recording cell the network weights after one train_step; per
cell the path every launch took.  Seeded inputs.  --engine oracle (tests/oracle_engine.py: no GPU) runs problems.mnist at
6-20-10 on 32 images; --engine hip at the reference shape (784-20-10, minibatch 64, 256 synthetic images), which the FAST form
of l2o_mlp_unroll needs."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from open_l2o_amd import _engine, meta, meta_rnnprop_eval, problems, util  # noqa: E402

T, LR = 3, 1e-3


def build(name, options, rnnprop=False, T=T, second_derivatives=False, seed=11):
    meta.set_random_seed(seed)
    problem, net_config, na = util.get_config(name, net_name="RNNprop" if rnnprop else None, problem_options=options)
    opt = meta_rnnprop_eval.MetaOptimizer(0.95, 0.95, **net_config) if rnnprop else meta.MetaOptimizer(**net_config)
    opt.meta_loss(problem, T, net_assignments=na, second_derivatives=second_derivatives)
    opt.graph.reset()
    return opt, opt.graph


def mnist_options(hip):
    n_img, batch = (256, 64) if hip else (32, 4)
    if hip:
        data = problems.synthetic_mnist(n_img, seed=5)
    else:
        r = np.random.default_rng(5)
        data = {"images": r.random((n_img, 6)).astype(np.float32), "labels": r.integers(0, 10, size=n_img)}
    idx = np.random.default_rng(6).integers(0, n_img, size=(T + 1, batch))
    return {"batch_size": batch, "data": data, "sampler": lambda n, b, N: idx[:n]}


class Dump(object):
    def __init__(self, eng):
        self.eng, self.out = eng, {}

    def launch(self, cell, k, g, feed=None, commit=True, record=False, **kw):
        rec = {} if record else None
        fx, xs = g.launch(feed, commit, record=rec, **kw)
        g.wait_fx()
        pre = "%s/%d/" % (cell, k)
        self.out[pre + "fx"] = self.eng.to_numpy(fx)
        for j, x in enumerate(xs):
            self.out[pre + "x%d" % j] = self.eng.to_numpy(x)
        for j, gf in enumerate(rec["g_final"] if record else ()):
            self.out[pre + "g_final%d" % j] = self.eng.to_numpy(gf)
        self.out.setdefault(cell + "/paths", []).append(g.last_path)

    def cell(self, cell, opt, g, feeds=({}, {}), train=None, **kw):
        """One launch per feed, then (train: a feed) one train_step and the weights it leaves."""
        for k, feed in enumerate(feeds):
            self.launch(cell, k, g, feed, **kw)
        if train is not None:
            g.train_step(train, True, LR)
            self.out[cell + "/paths"].append(g.last_path)
            for key, mods in opt.save().items():
                for mod, variables in mods.items():
                    for var, a in variables.items():
                        self.out["%s/w/%s/%s/%s" % (cell, key, mod, var)] = np.asarray(a, np.float32)


def with_env(name, fn):
    os.environ[name] = "1"
    try:
        fn()
    finally:
        del os.environ[name]


def run(engine, path):
    hip = engine == "hip"
    if hip:
        eng = _engine.HipEngine()
    else:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from test_confocal_cpu import ConfocalOracleEngine
        eng = ConfocalOracleEngine()
    _engine.set_default_engine(eng)
    d = Dump(eng)
    quad = {"batch_size": 2, "num_dims": 16}
    d.cell("quadratic/plain", *build("quadratic", quad), feeds=({}, {}, {}))     # (hip: the third replays a prepared call)
    d.cell("quadratic/uncommitted", *build("quadratic", quad), commit=False)
    d.cell("quadratic/recording", *build("quadratic", quad), record=True, train={})
    opt, g = build("quadratic", quad)
    for k in range(2):
        for j, gf in enumerate(g.gradients()):
            d.out["quadratic/gradients/%d/g_final%d" % (k, j)] = eng.to_numpy(gf)
    opt, g = build("quadratic", quad)
    d.cell("quadratic/restart", opt, g, restart=[v.value.clone() for v in g.x])
    with_env("L2O_DISABLE_FUSED", lambda: d.cell("quadratic/steps", *build("quadratic", quad)))
    d.cell("quadratic/second_derivatives", *build("quadratic", quad, second_derivatives=True), record=True, train={})
    opt, g = build("lasso", quad, rnnprop=True)
    d.cell("lasso_rnnprop/plain", opt, g, feeds=({g.step: 1}, {g.step: 4}))
    d.cell("lasso_rnnprop/recording", opt, g, feeds=({g.step: 7},), record=True, train={g.step: 10})
    opt, g = build("quadratic", quad)
    a = np.random.default_rng(7).uniform(0.5, 2.0, size=(2, 16)).astype(np.float32)
    d.cell("quadratic/x_scale", opt, g, feeds=({g.scale[0]: a}, {g.scale[0]: a}, {g.scale[0]: (a * 1.5).astype(np.float32)}))
    mn = mnist_options(hip)
    d.cell("mnist/plain", *build("mnist", mn))
    opt, g = build("mnist", mn)
    d.cell("mnist/recording", opt, g, record=True, train={})
    with_env("L2O_NO_MLP_UNROLL_RECORD", lambda: d.cell("mnist/recording_steps", opt, g, record=True, train={}))
    with_env("L2O_MLP_UNROLL_RECORD_GENERIC", lambda: d.cell("mnist/recording_generic", opt, g, record=True, train={}))
    cf = {"batch_size": 2, "num_points": 1, "ROI": [4, 5, 3]}
    d.cell("confocal/fused", *build("confocal_microscopy_3d", dict(cf, fused=True)))
    d.cell("confocal/fused_recording", *build("confocal_microscopy_3d", dict(cf, fused=True)), record=True, train={})
    d.cell("confocal/steps", *build("confocal_microscopy_3d", cf))
    for key, val in d.out.items():
        if key.endswith("/paths"):
            print("%-32s %s" % (key[:-6], " ".join(val)))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez(path, **{k: np.asarray(v) for k, v in d.out.items()})
    print("%d arrays -> %s" % (len(d.out), path))


def compare(a, b):
    A, B = np.load(a), np.load(b)
    bad = sorted(set(A.files) ^ set(B.files)) + [k for k in A.files if k in B.files and not np.array_equal(A[k], B[k])]
    worst = max([float(np.max(np.abs(A[k].astype(np.float64) - B[k]))) for k in bad
                 if k in A.files and k in B.files and A[k].dtype.kind == "f" and A[k].shape == B[k].shape] or [0.0])
    print("%s vs %s  %d arrays  equal: %s  max |diff| %g%s" % (a, b, len(A.files), "no" if bad else "yes", worst,
                                                              "  differing: " + " ".join(bad) if bad else ""))
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--engine", choices=("oracle", "hip"), default="oracle")
    ap.add_argument("--out", default="launch_paths.npz")
    ap.add_argument("--compare", nargs=2, metavar="NPZ")
    args = ap.parse_args()
    sys.exit(compare(*args.compare) if args.compare else run(args.engine, args.out))
