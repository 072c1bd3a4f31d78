#!/usr/bin/env python
"""The reference's Twin-L2O ``mode: "test"`` (Model_Free_L2O/L2O-Minimax/Twin-L2O.py) for its own config files.

    python scripts/evaluate_twin.py --config seesaw_test.json [--root DIR] [--out DIR] [--random-weights]

Reads the keys of the reference's ``config/*_test.json``: loss, dim, hidden_size, use_second, rescale, test_optim_iter,
n_test, test_epochs, test_data_path, load_name, load_model, save_name, save_curve, seed, mode.  Paths are taken relative to
--root (the reference runs from its own directory): the data at ``<root>/<test_data_path>`` (or, failing that, the file of
that name directly in <root>), the trained networks at ``<root>/result/<load_name>/<load_model>{min,max}.pth``.  The reference
ships no trained weights: with --random-weights, when those files are absent, the two networks are default-initialised from
the config's seed.  All ``n_test x test_epochs`` runs (instance j, restart i -> row j * test_epochs + i) go out in ONE launch.
Writes, under --out (default ``<root>/result/<save_name>``): every run's curve_info as the reference names it, and
``twin_eval.json`` with the mean distances after the burn-in half and the evaluation loss of fit_optimizer
(mean over runs of sum(dist_v^2 + dist_u^2) after the burn-in).  ``mode: "train"`` is refused here: meta-training is
``scripts/train_twin.py``, whose ``best{min,max}.pth`` / ``epoch{e}{min,max}.pth`` this script loads through load_name / load_model.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

KEYS = ("seed", "use_second", "test_optim_iter", "test_epochs", "n_test", "hidden_size", "loss", "unroll_unit", "save_curve",
        "rescale", "CL", "mode", "test_data_path", "save_name", "load_name", "load_model", "dim")
DRAW_SEED = 70                     # the reference's torch.manual_seed(70) in front of its test loop


def load_config(path):
    """The config as a dict with the reference's defaults (dim 1) and its refusals."""
    with open(path) as f:
        params = json.load(f)
    params["dim"] = params.get("dim", 1)
    if params.get("mode") == "train":
        raise NotImplementedError("evaluate_twin: mode \"train\": meta-training of the twin networks is "
                                  "scripts/train_twin.py; this script runs the evaluation unroll (mode \"test\") alone")
    if params.get("mode") != "test":
        raise ValueError("evaluate_twin: mode %r" % (params.get("mode"),))
    return params


def _find(root, rel):
    for p in (os.path.join(root, rel), os.path.join(root, os.path.basename(rel))):
        if os.path.exists(p):
            return p
    raise FileNotFoundError("evaluate_twin: %s not found under %s" % (rel, root))


def setup(params, root, random_weights=False):
    """(problem of n_test * test_epochs rows, opt_min, opt_max, theta0, states) of the config."""
    import torch
    from open_l2o_amd import twin
    data = np.loadtxt(_find(root, params["test_data_path"]), ndmin=2).astype(np.float32)[:params["n_test"]]
    if data.shape[0] < params["n_test"]:
        raise ValueError("evaluate_twin: n_test = %d but the data holds %d instances" % (params["n_test"], data.shape[0]))
    prob = twin.problem(params["loss"], data, params["dim"])
    prob = prob.take(np.repeat(np.arange(params["n_test"]), params["test_epochs"]))
    opts = []
    for i, which in enumerate(("min", "max")):
        opt = twin.Optimizer(hidden_size=params["hidden_size"], use_second=bool(params["use_second"]),
                             seed=int(params.get("seed", 0)) + i)
        path = os.path.join(root, "result", params["load_name"], params["load_model"] + which + ".pth")
        if os.path.exists(path):
            opt.load_state_dict(torch.load(path, map_location="cpu"))
        elif not random_weights:
            raise FileNotFoundError("evaluate_twin: %s is missing (the reference ships no trained weights); "
                                    "--random-weights runs seeded default-initialised networks" % path)
        opts.append(opt)
    theta0, states = twin.draw_start(prob, opts[0], opts[1], seed=DRAW_SEED)
    return prob, opts[0], opts[1], theta0, states


def summarize(params, du, dv):
    """The figures of twin_eval.json from the distances [runs, optim_it]."""
    burn = int(0.5 * params["test_optim_iter"])
    du, dv = np.asarray(du, np.float64)[:, burn:], np.asarray(dv, np.float64)[:, burn:]
    return {"runs": int(du.shape[0]), "optim_it": int(params["test_optim_iter"]), "burn_in": burn,
            "mean_distance_u": float(du.mean()), "mean_distance_v": float(dv.mean()),
            "eval_loss": float(np.mean(np.sum(np.square(dv) + np.square(du), axis=1)))}


def evaluate(params, root, out=None, random_weights=False):
    from open_l2o_amd import twin
    prob, opt_min, opt_max, theta0, states = setup(params, root, random_weights)
    res = twin.unroll(prob, opt_min, opt_max, params["test_optim_iter"], rescale=params["rescale"], out_mul=1.0,
                      theta0=theta0, states=states, record=("curve",))
    du, dv = twin.distances(prob, res)
    summary = summarize(params, du, dv)
    if out is not None:
        os.makedirs(out, exist_ok=True)
        if params.get("save_curve"):
            info = twin.curve_info(res)
            cdir = os.path.join(out, "curve_info", "test_example", params["load_model"])
            os.makedirs(cdir, exist_ok=True)
            for r in range(prob.n_inst):
                j, i = divmod(r, params["test_epochs"])
                first, last = float(prob.data[r].reshape(-1)[0]), float(prob.data[r].reshape(-1)[-1])
                np.savetxt(os.path.join(cdir, "sample_index_%d_epoch_%d_u_%s_v_%s.txt" % (j, i, round(first, 3), round(last, 3))),
                           info[r])
        with open(os.path.join(out, "twin_eval.json"), "w") as f:
            json.dump(summary, f, indent=1)
    return summary


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", required=True)
    ap.add_argument("--root", default=".")
    ap.add_argument("--out", default=None)
    ap.add_argument("--random-weights", action="store_true")
    args = ap.parse_args(argv)
    params = load_config(args.config)
    out = args.out or os.path.join(args.root, "result", params["save_name"])
    print(json.dumps(evaluate(params, args.root, out, args.random_weights)))


if __name__ == "__main__":
    main()
