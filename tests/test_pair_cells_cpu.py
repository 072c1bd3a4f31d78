"""The INPUTS of every cell behind the four byte goldens of the two-CU unroll (tests/golden/pair_split_bytes.json,
pair_step_paths_bytes.json, pair_combine_bytes.json, pair_bias_bytes.json), checked without a GPU: each module prepares its
launches on the CPU-side OracleEngine, and what a launch would hand to l2o_unroll* -- every array, T, step0, the zero-state
flag, the history it asks for, who reduces fx, the options in force, the host weights -- must equal
tests/golden/pair_cell_inputs.json, recorded from the test modules as they stood when the byte goldens were last matched
on an MI355X.  A failing byte test then reads at once as "the inputs moved" (this module fails too) or "the kernel moved".
A cell that a later change ADDS to a byte golden gets its entry (``describe`` of its launch) in the same commit; an entry
that exists is never re-recorded."""
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

import test_pair_bias_registers
import test_pair_prologue_staging
import test_pair_split_forms
import test_pair_step_paths
import unroll_harness as H
from open_l2o_amd import _abi
from oracle_engine import OracleEngine

SUITES = (test_pair_split_forms, test_pair_step_paths, test_pair_prologue_staging, test_pair_bias_registers)
OPTION_NAME = {o: n for n, o in _abi.OPTION_NAMES.items()}

with open(os.path.join(H.GOLDEN_DIR, "pair_cell_inputs.json")) as _f:
    INPUTS = json.load(_f)


def _plain(a):
    """A field of a descriptor as JSON holds it: tensors by their SHA-256."""
    if isinstance(a, torch.Tensor):
        return H.sha(a)
    if isinstance(a, tuple):
        return [_plain(b) for b in a]
    return a.item() if isinstance(a, np.generic) else a


def _fields(desc):
    return {f.name: _plain(getattr(desc, f.name)) for f in dataclasses.fields(desc)}


def describe(launch):
    with _abi.option_scope(launch.options):
        options = {OPTION_NAME.get(o, str(o)): _abi.get_option(o) for o, default in _abi.OPT_DEFAULTS.items()
                   if _abi.get_option(o) != default}
    weights = np.concatenate([np.asarray(launch.params[mod][var], np.float32).reshape(-1)
                              for mod in sorted(launch.params) for var in sorted(launch.params[mod])])
    out = {k: _plain(getattr(launch, k)) for k in ("T", "step0", "zero_state", "fused_fx", "x", "st", "m", "v", "x0")}
    out.update(options=options, weights=H.sha(weights), record=sorted(launch.hist_keys()), net=_fields(launch.spec),
               problem=_fields(launch.pd))
    return out


@pytest.mark.parametrize("suite", SUITES, ids=lambda s: os.path.basename(s.GOLDEN.path))
def test_golden_cells_hand_the_recorded_inputs_to_unroll(suite):
    want = INPUTS[os.path.basename(suite.GOLDEN.path)]
    launches = suite.golden_launches(OracleEngine())
    suite.GOLDEN.check_covers(launches)
    assert sorted(launches) == sorted(want)
    for cell in sorted(launches):
        got = describe(launches[cell])
        assert sorted(got) == sorted(want[cell]), cell
        for k in sorted(got):
            assert got[k] == want[cell][k], "%s: %s moved since the byte goldens were recorded" % (cell, k)
