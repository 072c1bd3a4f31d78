#!/usr/bin/env python
"""Record tests/golden/pair_combine_bytes.json: the SHA-256 of the raw bytes of fx[0..T] and fx_part of every cell of
COMBINE_CELLS in tests/test_pair_prologue_staging.py -- what k_combine_halves writes -- computed with the library this
process loads (L2O_HIP_LIB, or the in-tree build).  Run it ONCE on the commit whose bytes are the reference -- the commit
before a change to that kernel that claims bit-identity -- on an MI355X; the test then holds every later build to them.

  python scripts/record_pair_combine_bytes.py [--out tests/golden/pair_combine_bytes.json] [--check]

--check: compare against the file instead of writing it (exit status 1 on a difference)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "pair_combine_bytes.json"))
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    import test_pair_prologue_staging as cells
    from open_l2o_amd import _abi
    from open_l2o_amd._engine import HipEngine
    eng = HipEngine()
    out = {"cells": {}}
    for name in sorted(cells.COMBINE_CELLS):
        sha = cells.run_combine_cell(eng, name)
        out["cells"][name] = sha
        print("%-24s %s" % (name, " ".join("%s %s" % (k, sha[k][:12]) for k in sorted(sha))))
    print("library: %s (build id %s)" % (_abi.LIB_PATH, _abi.build_id()))
    if args.check:
        with open(args.out) as f:
            ref = json.load(f)
        bad = [(n, k) for n in out["cells"] for k in out["cells"][n] if ref["cells"].get(n, {}).get(k) != out["cells"][n][k]]
        print("DIFFERENT: %r" % bad if bad else "all %d cells equal %s" % (len(out["cells"]), args.out))
        return 1 if bad else 0
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
