"""The FAST kernel of the two-CU unroll (csrc/l2o_unroll_pair.h) builds the bf16x3 operands of its packed gate GEMM in the step
loop with the scalar-residual form of bx::split5 (plain v_sub_f32 on the four components instead of v_pk_add_f32 on pairs:
beside MFMAs a packed fp32 instruction costs more than its issue slot); the gather kernel keeps the packed form.  The same
fp32 subtractions in the same order: the change must not move a bit of any output, and it must not reach the kernels that
keep the packed form.

Checked here: every cell below reproduces, byte for byte, what the commit BEFORE the scalar-residual form computed
(tests/golden/pair_split_bytes.json: the SHA-256 of the raw bytes of fx[0..T], of x_T and of the packed final LSTM state,
recorded with that commit's library on an MI355X by scripts/record_pair_split_bytes.py), and runs the kernel instantiation
it is meant to run (l2o_last_unroll_variant).

Every cell: T = 4, B = 8 (one group of 16 workgroups), a random non-zero initial LSTM state, fixed seeds.
"""
import hashlib
import json
import os

import numpy as np
import pytest

from helpers import ORACLE_CFGS, device_problem, make_params, make_problem, random_state, spec_of
from open_l2o_amd import _abi

pytestmark = pytest.mark.gpu

T, B, STEP0 = 4, 8, 1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pair_split_bytes.json")

# id -> (net, kind, D, M, recording launch, exact gates, problem seed, expected template arguments)
# (the seeds are part of tests/golden/pair_split_bytes.json: a cell keeps its seed for good)
CELLS = {
    # CH 2, FAST prologue
    "quadratic_d32": ("dm", "quadratic", 32, None, False, False, 201, dict(CH=2, HIST=0, EXACT=0, FAST=1)),
    # CH 8, FAST: the flagship instantiation
    "quadratic_d128": ("dm", "quadratic", 128, None, False, False, 202, dict(CH=8, HIST=0, EXACT=0, FAST=1)),
    # CH 4, ragged: the kernel with the predicated gather (packed residuals, as before)
    "rastrigin_d40_logsign": ("dm_logsign", "rastrigin", 40, None, False, False, 203, dict(CH=4, HIST=0, EXACT=0, FAST=0)),
    # the 6-product core: must be untouched, the hash guards against collateral change
    "lasso_24x64_rnnprop": ("rnnprop", "lasso", 64, 24, False, False, 204, dict(CH=4, HIST=0, EXACT=0, FAST=0)),
    # the D = 128 cell on the recording kernel
    "quadratic_d128_recording": ("dm", "quadratic", 128, None, True, False, 202, dict(CH=8, HIST=1, EXACT=0, FAST=1)),
    # the D = 128 cell on the fp32-MFMA (exact gates) kernel: no split at all
    "quadratic_d128_exact": ("dm", "quadratic", 128, None, False, True, 202, dict(CH=8, HIST=0, EXACT=1, FAST=1)),
}


def _sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()


def run_cell(eng, name):
    """One launch of the cell -> ({"fx", "x", "st": sha256 of the raw bytes}, kernel name, template arguments)."""
    import torch
    net, kind, D, M, record, exact, seed, _ = CELLS[name]
    cfg = ORACLE_CFGS[net]
    spec = spec_of(cfg)
    wpack = eng.pack_weights(spec, make_params(cfg, seed=5, trained_like=True))
    prob, x0, arrays = make_problem(kind, B, D, seed=seed, M=M)
    rng = np.random.default_rng(seed + 50000)
    state0 = random_state(cfg, B * D, seed + 60000, scale=0.5)
    pd = device_problem(eng, arrays, B, D)
    x = eng.tensor(x0.reshape(B, D))
    st = eng.state_pack(*[eng.tensor(a) for hc in state0 for a in hc], B, D)
    m = v = None
    if cfg.kind == "rnnprop":
        gs = float(np.abs(prob.grad(x0)).max())
        m = eng.tensor((rng.standard_normal((B, D)) * 0.3 * gs).astype(np.float32))
        v = eng.tensor((rng.uniform(0.1, 1.0, (B, D)) * gs * gs).astype(np.float32))
    fx_part, fx = eng.zeros((T + 1) * B), eng.zeros(T + 1)
    hist = None
    if record:
        N = B * D
        hist = {"st": eng.zeros(T, st.numel()), "g": eng.zeros(T, N), "g_final": eng.zeros(N)}
    with _abi.option_scope({_abi.OPT_EXACT_GATES: 1} if exact else {}):
        eng.unroll(spec, wpack, pd, x, st, m, v, T, STEP0, fx_part, hist=hist)
        form, variant = eng.last_unroll_form()[0], eng.last_unroll_variant()
    eng.reduce_fx(fx_part, T + 1, B, B, fx)
    torch.cuda.synchronize()
    eng.check_unroll_status()                                     # (raises on a partner timeout)
    return {"fx": _sha(fx), "x": _sha(x), "st": _sha(st)}, form, variant


@pytest.fixture(scope="module")
def eng():
    from open_l2o_amd._engine import HipEngine
    return HipEngine()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_covers_every_cell(golden):
    assert sorted(golden["cells"]) == sorted(CELLS)
    assert (golden["T"], golden["B"]) == (T, B)


@pytest.mark.parametrize("name", sorted(CELLS))
def test_bytes_equal_the_parent_commit(eng, golden, name):
    got, form, variant = run_cell(eng, name)
    assert form == "k_unroll_pair"
    assert variant == dict(CELLS[name][7], KR=0, NV=0)
    want = golden["cells"][name]
    print("%s: %s" % (name, " ".join("%s %s" % (k, got[k][:12]) for k in sorted(got))))
    for k in ("fx", "x", "st"):
        assert got[k] == want[k], "%s: %s differs from the parent commit's bytes" % (name, k)


def test_cells_are_not_degenerate(golden):
    """The guard is only worth something where the gate arithmetic reaches the hashed bytes: the exact-gates run of the
    D = 128 inputs must differ in bits from the bf16x3 run of the same inputs."""
    c = golden["cells"]
    for k in ("fx", "x", "st"):
        assert c["quadratic_d128"][k] != c["quadratic_d128_exact"][k], k
