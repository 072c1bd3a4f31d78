#!/usr/bin/env python
"""Record the byte goldens of the two-CU unroll's test suites: per cell the SHA-256 of the raw bytes of what the suite
compares (its module's docstring says which buffers), computed with the library this process loads (L2O_HIP_LIB, or the
in-tree build).  Run it ONCE on the commit whose bytes are the reference -- the commit before a change to the kernel that
claims bit-identity -- on an MI355X; the tests then hold every later build to these hashes.

  python scripts/record_pair_bytes.py SUITE [SUITE...] | all [--out-dir tests/golden] [--check]

--check: compare against the files instead of writing them (exit status 1 on a difference).

A suite is a test module with GOLDEN (unroll_harness.Golden: the file), golden_cells(eng) -> {cell id: {quantity: sha256}}
(it asserts the kernel and the template arguments every cell ran) and, optionally, GOLDEN_META (top-level keys beside
"cells")."""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

SUITES = {"split": "test_pair_split_forms", "step": "test_pair_step_paths", "combine": "test_pair_prologue_staging",
          "bias": "test_pair_bias_registers", "l2b": "test_pair_l2b_placement", "l2a": "test_pair_l2a_placement"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("suites", nargs="+", choices=sorted(SUITES) + ["all"])
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    from open_l2o_amd import _abi
    from open_l2o_amd._engine import HipEngine
    eng = HipEngine()
    print("library: %s (build id %s)" % (_abi.LIB_PATH, _abi.build_id()))
    different = 0
    for suite in sorted(SUITES) if "all" in args.suites else args.suites:
        mod = importlib.import_module(SUITES[suite])
        cells = mod.golden_cells(eng)
        out = dict(getattr(mod, "GOLDEN_META", {}), cells=cells)
        path = os.path.join(args.out_dir, os.path.basename(mod.GOLDEN.path))
        width = max(len(name) for name in cells)
        for name in sorted(cells):
            print("%-*s %s" % (width, name, " ".join("%s %s" % (k, cells[name][k][:12]) for k in sorted(cells[name]))))
        if args.check:
            with open(path) as f:
                ref = json.load(f)
            bad = [(n, k) for n in cells for k in cells[n] if ref["cells"].get(n, {}).get(k) != cells[n][k]]
            bad += [(n, None) for n in ref["cells"] if n not in cells] + [k for k in out if k != "cells" and ref.get(k) != out[k]]
            print("%s: DIFFERENT: %r" % (suite, bad) if bad else "%s: all %d cells equal %s" % (suite, len(cells), path))
            different += bool(bad)
        else:
            with open(path, "w") as f:
                json.dump(out, f, indent=1, sort_keys=True)
                f.write("\n")
            print("%s: wrote %s" % (suite, path))
    return 1 if different else 0


if __name__ == "__main__":
    sys.exit(main())
