#!/usr/bin/env python
"""The reference's Twin-L2O ``mode: "train"`` (Model_Free_L2O/L2O-Minimax/Twin-L2O.py: fit_optimizer) for its own config files.

    python scripts/train_twin.py --config seesaw_CL_train.json --root DIR [--out DIR] [--epochs N] [--eval-interval N]

Reads the keys of the reference's ``config/*_train.json``: seed, use_second, meta_lr, batch_size, n_train, train_epochs,
train_optim_iter, eval_optim_iter, n_eval, hidden_size, loss, dim, unroll_unit, rescale, CL, save_curve, train_data_path,
eval_data_path, save_name, mode; save_train (the reference's seaborn plots) and load_name are read and ignored.  Paths are
taken relative to --root: the data at ``<root>/<train_data_path>`` (or, failing that, the file of that name directly in
<root>).  Writes under --out (default ``<root>/result/<save_name>``, where ``scripts/evaluate_twin.py`` looks with
``load_name = <save_name>`` and ``load_model = "best"`` or ``"epoch<e>"``): ``epoch{e}{min,max}.pth`` every epoch,
``best{min,max}.pth`` when the evaluation loss improves (every --eval-interval epochs, default 5), the train-mode curves
with ``save_curve``, and ``twin_train.json``, one record per epoch.  Every segment's forward, BPTT and weight gradient is a
HIP launch (``open_l2o_amd.twin.fit``); Adam is ``torch.optim.Adam``, as in the reference.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

KEYS = ("seed", "use_second", "meta_lr", "batch_size", "n_train", "train_epochs", "train_optim_iter", "eval_optim_iter", "n_eval",
        "save_train", "hidden_size", "loss", "save_curve", "unroll_unit", "rescale", "CL", "mode", "train_data_path",
        "eval_data_path", "save_name", "load_name", "dim")


def load_config(path):
    """The config as a dict with the reference's default (dim 1) and its refusals."""
    with open(path) as f:
        params = json.load(f)
    params["dim"] = params.get("dim", 1)
    if params.get("mode") != "train":
        raise ValueError("train_twin: mode %r (scripts/evaluate_twin.py runs mode \"test\")" % (params.get("mode"),))
    if params.get("CL") and params["loss"] != 3:
        raise ValueError("train_twin: \"CL\": 1 ranks instances by the seesaw's gradient: loss 3 only (got loss %r)" % (params["loss"],))
    return params


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", required=True)
    ap.add_argument("--root", default=".")
    ap.add_argument("--out", default=None)
    ap.add_argument("--epochs", type=int, default=None)
    ap.add_argument("--eval-interval", type=int, default=5)
    args = ap.parse_args(argv)
    params = load_config(args.config)
    from open_l2o_amd import twin
    out = args.out or os.path.join(args.root, "result", params["save_name"])
    best, _, _, history = twin.fit(params, args.root, out, epochs=args.epochs, eval_interval=args.eval_interval)
    with open(os.path.join(out, "twin_train.json"), "w") as f:
        json.dump({"best_loss": best, "epochs": history}, f, indent=1)
    print(json.dumps({"best_loss": best, "epochs": len(history), "adam_steps": history[-1]["steps"] if history else None}))


if __name__ == "__main__":
    main()
