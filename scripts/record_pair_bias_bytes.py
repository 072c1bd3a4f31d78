#!/usr/bin/env python
"""Record tests/golden/pair_bias_bytes.json: the SHA-256 of the raw bytes of fx, x_T and the final state (and m, v for
RNNProp) of every cell of tests/test_pair_bias_registers.py -- the FAST kernel of the two-CU unroll at T = 3 from the zero
state and continuing, the T = 2 cell and the T = 64 cell -- computed with the library this process loads (L2O_HIP_LIB, or
the in-tree build).  Run it ONCE on the commit whose bytes are the reference -- the commit before a change to that kernel
that claims bit-identity -- on an MI355X; the test then holds every later build to them.

  python scripts/record_pair_bias_bytes.py [--out tests/golden/pair_bias_bytes.json] [--check]

--check: compare against the file instead of writing it (exit status 1 on a difference)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


class _Patch:
    """monkeypatch.setattr for a script: set now, undo() puts everything back."""

    def __init__(self):
        self._saved = []

    def setattr(self, obj, name, value):
        self._saved.append((obj, name, getattr(obj, name)))
        setattr(obj, name, value)

    def undo(self):
        for obj, name, value in reversed(self._saved):
            setattr(obj, name, value)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "pair_bias_bytes.json"))
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    import test_pair_bias_registers as cells
    from open_l2o_amd import _abi
    from open_l2o_amd._engine import HipEngine
    for net in cells.NETS:
        cells.assert_biases_tell_quads_apart(net)
    eng = HipEngine()
    patch = _Patch()
    try:
        out = {"cells": cells.golden_cells(eng, patch)}
    finally:
        patch.undo()
    for name in sorted(out["cells"]):
        c = out["cells"][name]
        print("%-44s %s" % (name, " ".join("%s %s" % (k, c[k][:12]) for k in sorted(c))))
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
