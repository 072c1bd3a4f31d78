"""CPU-side checks of the one-instance-per-XCD MLP unroll at the reference's minibatch of 128 (ABI v15): the workspace
size query accepts batch 64 and 128 and nothing else, and its layout is the documented one -- a header (struct MlpWs +
64 bytes of team counters) and per instance the 256-aligned sum of the partial-sum inboxes P [32][32][B * 20 / 32], the
sums S [2][B * 20] and the small parameters Sm [2][230], all 8-byte granules."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MLPWS_BYTES = 4 * 4 + 2 * 8 + 8 * 4 + 16 * 8      # status, seq, fault, pad0; ticks, ticks_total; pad[8]; phases[16]


@pytest.fixture(scope="module")
def lib():
    from open_l2o_amd import _abi
    if not os.path.exists(_abi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _abi.lib()


def _mlp(batch, n_in=784):
    from open_l2o_amd import _abi
    return _abi.Mlp(n_in=n_in, n_hidden=20, n_out=10, batch=batch, activation=0, n_data=1000)


def _expected(batch, n_inst):
    p = 32 * 32 * (batch * 20 // 32) * 8
    s = 2 * (batch * 20) * 8
    sm = 2 * 230 * 8
    return MLPWS_BYTES + 64 + n_inst * ((p + s + sm + 255) & ~255)


def _ws(lib, batch, n_inst, n_in=784):
    m = _mlp(batch, n_in)
    return int(lib.l2o_mlp_unroll_multi_workspace_bytes(C.byref(m), n_inst))


def test_abi_version_is_15(lib):
    from open_l2o_amd import _abi
    assert _abi.L2O_ABI_VERSION == 15 and lib.l2o_abi_version() == 15


@pytest.mark.parametrize("n_inst", [1, 8])
def test_batch128_workspace_bytes(lib, n_inst):
    got = _ws(lib, 128, n_inst)
    assert got > 0
    assert got == _expected(128, n_inst)
    assert _expected(128, n_inst) == 256 + n_inst * ((32 * 32 * 80 * 8 + 2 * 2560 * 8 + 2 * 230 * 8 + 255) & ~255)


@pytest.mark.parametrize("n_inst", [1, 8])
def test_batch64_workspace_bytes_unchanged(lib, n_inst):
    assert _ws(lib, 64, n_inst) == _expected(64, n_inst)


@pytest.mark.parametrize("batch", [32, 96, 256])
def test_other_batches_are_not_served(lib, batch):
    assert _ws(lib, batch, 1) == 0 and _ws(lib, batch, 8) == 0


def test_batch128_instance_and_shape_limits(lib):
    assert _ws(lib, 128, 0) == 0 and _ws(lib, 128, 9) == 0
    m = _abi_mlp_wrong_hidden()
    assert int(lib.l2o_mlp_unroll_multi_workspace_bytes(C.byref(m), 1)) == 0


def _abi_mlp_wrong_hidden():
    from open_l2o_amd import _abi
    return _abi.Mlp(n_in=784, n_hidden=32, n_out=10, batch=128, activation=0, n_data=1000)
