"""What HipEngine's struct-building methods hand to the library, without a GPU: the BPTT calls (pack_weights_device, bwd_step,
bwd_multi, bwd_unroll, bwd_step_generic, klstm_bwd_step), the analytic unroll with a history and with fx, the small passes
that keep a scratch buffer (problem_hvp, atb, wgrad, wgrad_compact, colsum) and the seven step-path <stem>_fg methods -- on
the recording engine of test_fused_host_paths_cpu.py.  Per method: the symbol sequence, the bytes of every struct against
one built here from _abi, every pointer and array element (NULLs included), the scalars; that a cached buffer is reused for
a smaller request and replaced for a larger one; and the refusals of the fg methods with their texts."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from helpers import ORACLE_CFGS, spec_of
from open_l2o_amd import _abi, _engine
from open_l2o_amd._engine import NetSpec, ProblemDesc
from test_fused_host_paths_cpu import RecordingLib, StubEngine, addr, confocal_desc, confocal_struct, f32, net_cfg, val

WEIGHT_FIELDS = ("w_gates1", "b_gates1", "w_gates2", "b_gates2", "w_lin", "b_lin", "w_fc", "b_fc", "wpack")
CASES = [("dm", False), ("rnnprop", True)]


def i32(*shape):
    return torch.zeros(*shape, dtype=torch.int32)


def args_of(eng, k=-1):
    return [val(a) for a in eng.lib.calls[k][1]]


def struct_of(cls, **fields):
    """The bytes of a `cls` with the given fields: a tensor gives its address, a list fills an array field element by
    element, None stays NULL."""
    s, value = cls(), lambda v: v.data_ptr() if isinstance(v, torch.Tensor) else v
    for k, v in fields.items():
        if isinstance(v, (list, tuple)):
            for i, e in enumerate(v):
                getattr(s, k)[i] = value(e)
        elif v is not None:
            setattr(s, k, value(v))
    return bytes(s)


def net_weights(rnnprop):
    """A weights dict as meta.py keeps it: the input projection only for RNNProp, the packed copy always."""
    w = {k: f32(2) for k in WEIGHT_FIELDS[:6]}
    w.update(w_fc=f32(2) if rnnprop else None, wpack=f32(7))
    if rnnprop:
        w["b_fc"] = f32(2)
    return w


# ---- 1. the BPTT calls -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,rnnprop", CASES)
def test_pack_weights_device(name, rnnprop):
    eng, spec, w, out = StubEngine(), spec_of(ORACLE_CFGS[name]), net_weights(rnnprop), f32(9)
    eng.pack_weights_device(spec, w, out)
    assert eng.lib.symbols() == ["l2o_wpack_device"]
    args = args_of(eng)
    assert bytes(args[0]) == net_cfg(spec)
    want = struct_of(_abi.NetWeights, **dict(w, wpack=None))         # (wpack is the OUTPUT: never read from the dict)
    assert bytes(args[1]) == want and args[1].wpack is None and args[1].w_gates1 == w["w_gates1"].data_ptr()
    assert args[1].w_fc == addr(w.get("w_fc")) and args[1].b_fc == addr(w.get("b_fc"))
    assert args[2:] == [out.data_ptr(), None]
    # the same buffer, the same configuration again: its padding is clean, the pack kernel runs without the memset
    eng.pack_weights_device(spec, w, out)
    again = args_of(eng)
    assert again[0].options == _abi.options_word() | (8 | 1) << (4 * _abi.OPT_WPACK_NO_CLEAR)
    assert bytes(again[1]) == want and again[2:] == [out.data_ptr(), None]
    eng.pack_weights_device(spec, w, f32(9))
    assert args_of(eng)[0].options == _abi.options_word()


BWD_IO_PTRS = ("g", "m", "v", "st_prev", "dx_next", "carry_in", "carry_out", "act1", "dz1", "act2", "dz2", "h2", "dd",
               "feats", "du")


@pytest.mark.parametrize("with_dg", [False, True])
@pytest.mark.parametrize("name,rnnprop", CASES)
def test_bwd_step(name, rnnprop, with_dg):
    eng, spec, w = StubEngine(), spec_of(ORACLE_CFGS[name]), net_weights(rnnprop)
    io = {k: f32(3) for k in BWD_IO_PTRS}
    if not rnnprop:
        io.update(m=None, v=None)
        del io["feats"], io["du"]
    if with_dg:
        io.update(dg=f32(3), a_stride=48, b_stride=200)
    eng.bwd_step(spec, w, io, 0.25, 0.5, 4, 6)
    assert eng.lib.symbols() == ["l2o_cwlstm_bwd_step"]
    args = args_of(eng)
    assert bytes(args[0]) == net_cfg(spec) and bytes(args[1]) == struct_of(_abi.NetWeights, **w)
    assert args[1].wpack == w["wpack"].data_ptr()
    assert bytes(args[2]) == struct_of(_abi.BwdIO, **io)
    b = args[2]
    for k in BWD_IO_PTRS:
        assert getattr(b, k) == addr(io.get(k)), k
    assert (b.a_stride, b.b_stride, b.dg) == ((48, 200, io["dg"].data_ptr()) if with_dg else (0, 0, None))
    assert args[3:] == [0.25, 0.5, 4, 6, None]


@pytest.mark.parametrize("name,rnnprop", CASES)
def test_bwd_multi(name, rnnprop):
    eng, spec, w = StubEngine(), spec_of(ORACLE_CFGS[name]), net_weights(rnnprop)
    segs = [dict(g=f32(3), m=f32(3) if rnnprop else None, v=f32(3) if rnnprop else None, st_prev=f32(8), dx_next=f32(3),
                 B=1, D=3),
            dict(g=f32(5), st_prev=f32(8), dx_next=None, B=5, D=1)]
    ci, co, A, Bm = f32(4, 32, 20), f32(4, 32, 20), f32(32, 3), f32(32, 5)
    eng.bwd_multi(spec, w, segs, ci, co, A, Bm, 0.1, 0.2)
    assert eng.lib.symbols() == ["l2o_cwlstm_bwd_multi"]
    args = args_of(eng)
    assert bytes(args[0]) == net_cfg(spec) and bytes(args[1]) == struct_of(_abi.NetWeights, **w)
    assert len(args[2]) == 2 and bytes(args[2]) == b"".join(struct_of(_abi.BwdSeg, **s) for s in segs)
    for got, s in zip(args[2], segs):
        assert [getattr(got, k) for k in ("g", "m", "v", "st_prev", "dx_next")] == \
            [addr(s.get(k)) for k in ("g", "m", "v", "st_prev", "dx_next")]
        assert (got.B, got.D) == (s["B"], s["D"])
    assert args[3:] == [2, ci.data_ptr(), co.data_ptr(), A.data_ptr(), Bm.data_ptr(), 0.1, 0.2, None]
    eng.bwd_multi(spec, w, segs, None, co, A, Bm, 0.1, 0.2)          # (the first BPTT step: no incoming carry)
    assert args_of(eng)[4:6] == [None, co.data_ptr()]
    # the carries and the row matrices are checked: contiguous fp32
    for bad in (f32(4, 32, 40)[:, :, ::2], torch.zeros(4, 32, 20, dtype=torch.float64)):
        with pytest.raises(AssertionError, match="contiguous fp32"):
            eng.bwd_multi(spec, w, segs, bad, co, A, Bm, 0.1, 0.2)
        with pytest.raises(AssertionError, match="contiguous fp32"):
            eng.bwd_multi(spec, w, segs, ci, bad, A, Bm, 0.1, 0.2)


@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("name,rnnprop", CASES)
def test_bwd_unroll(name, rnnprop, compact):
    eng, spec, w, T = StubEngine(), spec_of(ORACLE_CFGS[name]), net_weights(rnnprop), 2
    panels = [dict(B=1, D=3, gs=[f32(3) for _ in range(T)], sts=[f32(8) for _ in range(T)],
                   ms=[f32(3) for _ in range(T)] if rnnprop else None, vs=[f32(3) for _ in range(T)] if rnnprop else None,
                   dxs=[f32(3) for _ in range(T)], g_final=f32(3)),
              dict(B=2, D=1, gs=[f32(2) for _ in range(T)], sts=[f32(8) for _ in range(T)])]
    A, Bm, ci, co = f32(T + 1, 48, 3), f32(T, 48, 5), f32(4, 48, 20), f32(4, 48, 20)
    eng.bwd_unroll(spec, w, panels, T, 3, A, Bm, carry_in=ci, carry_out=co, compact=compact)
    assert eng.lib.symbols() == ["l2o_cwlstm_bwd_unroll_compact" if compact else "l2o_cwlstm_bwd_unroll"]
    args = args_of(eng)
    assert bytes(args[0]) == net_cfg(spec) and bytes(args[1]) == struct_of(_abi.NetWeights, **w)
    assert len(args[2]) == 2 and bytes(args[2]) == (struct_of(_abi.BwdUnrollSeg, B=1, D=3, g_final=panels[0]["g_final"]) +
                                                    struct_of(_abi.BwdUnrollSeg, B=2, D=1))
    assert args[2][0].g_final == panels[0]["g_final"].data_ptr() and args[2][1].g_final is None
    table = eng._bwd_table
    assert args[3:] == [2, table.data_ptr(), T, 3, ci.data_ptr(), co.data_ptr(), A.data_ptr(), Bm.data_ptr(), None]
    want = [[addr(p["gs"][t]), addr(p["ms"][t]) if p.get("ms") else 0, addr(p["vs"][t]) if p.get("vs") else 0,
             addr(p["sts"][t]), addr(p["dxs"][t]) if p.get("dxs") else 0] for t in range(T) for p in panels]
    assert table.dtype == torch.int64 and table.tolist() == want
    # a table the caller built, no carries
    mine = eng.bwd_table(panels, T)
    eng.bwd_unroll(spec, w, panels, T, 1, A, Bm, table=mine, compact=compact)
    assert args_of(eng)[4:] == [mine.data_ptr(), T, 1, None, None, A.data_ptr(), Bm.data_ptr(), None] and eng._bwd_table is mine


def test_gen_net_and_bwd_step_generic():
    eng = StubEngine()
    spec = NetSpec(_abi.NET_RNNPROP, _abi.PRE_FC_ELU, (6, 5), 0.5, True)
    rng = np.random.default_rng(0)
    params = {"lstm_1": {"w_gates": rng.random((9, 24)), "b_gates": rng.random(24)},
              "lstm_2": {"w_gates": rng.random((11, 20)), "b_gates": rng.random(20)},
              "linear": {"w": rng.random((5, 1)), "b": rng.random(1)},
              "input_projection": {"w": rng.random((2, 3)), "b": rng.random(3)}}
    gen = eng.gen_net(spec, params, direct=True)
    assert isinstance(gen, _engine.HipEngine.GenNet) and gen.layers == (6, 5) and len(gen.tensors) == 8
    t = gen.tensors
    assert all(a.dtype == torch.float32 for a in t)
    assert np.array_equal(t[2].numpy(), params["lstm_2"]["w_gates"].astype(np.float32))
    assert bytes(gen.c) == struct_of(_abi.GenNet, n_layers=2, hidden=[6, 5], in_dim=3, direct_inputs=1, w_gates=[t[0], t[2]],
                                     b_gates=[t[1], t[3]], w_lin=t[4], b_lin=t[5], w_fc=t[6], b_fc=t[7])
    c = gen.c
    assert (c.n_layers, list(c.hidden), c.in_dim, c.direct_inputs) == (2, [6, 5, 0], 3, 1)
    assert list(c.w_gates) == [t[0].data_ptr(), t[2].data_ptr(), None] and list(c.b_gates) == [t[1].data_ptr(), t[3].data_ptr(), None]
    assert (c.w_lin, c.b_lin, c.w_fc, c.b_fc) == tuple(a.data_ptr() for a in t[4:])
    plain = eng.gen_net(NetSpec(_abi.NET_CW, _abi.PRE_LOGSIGN, (6, 5)), params)
    assert (plain.c.in_dim, plain.c.direct_inputs, plain.c.w_fc, plain.c.b_fc, len(plain.tensors)) == (2, 0, None, None, 6)
    assert eng.gen_net(NetSpec(_abi.NET_CW, _abi.PRE_IDENTITY, (6, 5)), params).c.in_dim == 1
    assert eng.lib.calls == []

    io = {k: f32(4) for k in ("g", "m", "v", "st_prev", "dx_next", "carry_out", "tc", "h_last", "dd", "feats", "du")}
    io.update(carry_in=None, act=[f32(4), f32(4)], dz=[f32(4), f32(4)])
    eng.bwd_step_generic(spec, gen, io, 0.3, 0.6, 4)
    assert eng.lib.symbols() == ["l2o_cwlstm_bwd_step_generic"]
    args = args_of(eng)
    assert bytes(args[0]) == bytes(spec.to_c()) and args[0].hidden == -1 and args[1] is gen.c
    assert bytes(args[2]) == struct_of(_abi.GenBwdIO, **io)
    b = args[2]
    for k in ("g", "m", "v", "st_prev", "dx_next", "carry_in", "carry_out", "tc", "h_last", "dd", "feats", "du", "dg"):
        assert getattr(b, k) == addr(io.get(k)), k
    assert list(b.act) == [io["act"][0].data_ptr(), io["act"][1].data_ptr(), None]
    assert list(b.dz) == [io["dz"][0].data_ptr(), io["dz"][1].data_ptr(), None]
    assert args[3:] == [0.3, 0.6, 4, None]


def test_klstm_net_and_bwd_step():
    eng = StubEngine()
    rng = np.random.default_rng(1)
    variables = {"lstm_1": {"w_gates": rng.random((13, 16)), "b_gates": rng.random(16)},
                 "lstm_2": {"w_gates": rng.random((7, 12)), "b_gates": rng.random(12)},
                 "linear": {"w": rng.random((3, 9)), "b": rng.random(9)}}
    net = types.SimpleNamespace(kernel_shape=(3, 3), layers=(4, 3), preprocess=_abi.PRE_LOGSIGN, tanh_output=True,
                                logsign_k=5.0, scale=0.25, variables=variables)
    dev = eng.klstm_net(net)
    assert isinstance(dev, _engine.HipEngine.KlstmNet) and len(dev.tensors) == 6 and eng.lib.calls == []
    t, c = dev.tensors, dev.c
    assert np.array_equal(t[4].numpy(), variables["linear"]["w"].astype(np.float32))
    assert (c.kw, c.kh, c.n_layers, list(c.hidden), c.preprocess, c.tanh_output, c.flags, c.logsign_k, c.scale) == \
        (3, 3, 2, [4, 3], _abi.PRE_LOGSIGN, 1, 0, 5.0, 0.25)
    assert list(c.w_gates) == [t[0].data_ptr(), t[2].data_ptr()] and list(c.b_gates) == [t[1].data_ptr(), t[3].data_ptr()]
    assert (c.w_lin, c.b_lin) == (t[4].data_ptr(), t[5].data_ptr())
    net.device_net = lambda engine: dev

    io = {k: f32(4) for k in ("g", "st_prev", "dx_next", "carry_out", "tc", "h_last", "dd")}
    io.update(carry_in=None, act=[f32(4), f32(4)], dz=[f32(4), f32(4)])
    eng.klstm_bwd_step(net, io, 4)
    assert eng.lib.symbols() == ["l2o_klstm_bwd_step"]
    args = args_of(eng)
    assert args[0] is dev.c and bytes(args[1]) == struct_of(_abi.KlstmBwdIO, **io) and args[2:] == [4, None]
    b = args[1]
    for k in ("g", "st_prev", "dx_next", "carry_in", "carry_out", "tc", "h_last", "dd"):
        assert getattr(b, k) == addr(io[k]), k
    assert list(b.act) == [a.data_ptr() for a in io["act"]] and list(b.dz) == [a.data_ptr() for a in io["dz"]]
    # every tensor is checked: contiguous fp32
    for bad in (dict(io, g=f32(8)[::2]), dict(io, dz=[f32(4), torch.zeros(4, dtype=torch.float64)])):
        with pytest.raises(AssertionError, match="contiguous fp32"):
            eng.klstm_bwd_step(net, bad, 4)


# ---- 2. the analytic unroll -------------------------------------------------------------------------------------------
def problem(B=2, D=4):
    return ProblemDesc(kind=_abi.PROB_LASSO, B_local=B, B_global=2 * B, D=D, M=3, l1=0.1, alpha=2.0, W=f32(B, 3, D),
                       y=f32(B, 3), C=None, x_scale=f32(B, D), w_shared=True)


def problem_struct(p):
    return struct_of(_abi.Problem, kind=p.kind, B_local=p.B_local, B_global=p.B_global, D=p.D, M=p.M,
                     flags=_abi.PROB_W_SHARED, l1=p.l1, alpha=p.alpha, W=p.W, y=p.y, C=p.C, x_scale=p.x_scale)


@pytest.mark.parametrize("mode", ["plain", "hist", "fx", "fx_hist"])
@pytest.mark.parametrize("name,rnnprop", CASES)
def test_unroll(name, rnnprop, mode):
    eng, spec, p, T = StubEngine(48), spec_of(ORACLE_CFGS[name]), problem(), 3
    wpack, x, st, fx_part = f32(5), f32(2, 4), f32(40), f32((T + 1) * 2)
    m, v = (f32(2, 4), f32(2, 4)) if rnnprop else (None, None)
    hist = None
    if "hist" in mode:
        hist = dict(st=f32(T, 40), g=f32(T, 8), g_final=f32(8))
        if rnnprop:
            hist.update(m=f32(T, 8), v=f32(T, 8))
    fx, x0 = (f32(T + 1), f32(2, 4)) if "fx" in mode else (None, None)
    eng.unroll(spec, wpack, p, x, st, m, v, T, 9, fx_part, hist=hist, fx=fx, x0=x0, zero_state=fx is not None)
    sym = "l2o_unroll_reduce" if fx is not None else "l2o_unroll_record" if hist else "l2o_unroll"
    assert eng.lib.symbols() == ["l2o_unroll_workspace_bytes", "l2o_unroll_workspace_layout", sym]
    size_args = args_of(eng, 0)
    assert bytes(size_args[0]) == net_cfg(spec) and bytes(size_args[1]) == problem_struct(p) and size_args[2] == T
    ws = eng._workspace
    assert ws.dtype == torch.uint8 and ws.numel() == 48 and not ws.any() and eng._last_ws is ws
    args = args_of(eng)
    assert bytes(args[0]) == net_cfg(spec) and args[1] == wpack.data_ptr() and bytes(args[2]) == problem_struct(p)
    state = [x.data_ptr(), st.data_ptr(), addr(m), addr(v)]
    if fx is not None:
        assert args[3] == x0.data_ptr() and args[4:8] == state
        assert args[8:14] == [T, 9, _abi.UNROLL_ZERO_STATE, fx_part.data_ptr(), fx.data_ptr(), ws.data_ptr()]
        h, tail = args[14], args[15:]
    else:
        assert args[3:7] == state and args[7:11] == [T, 9, fx_part.data_ptr(), ws.data_ptr()]
        h, tail = (args[11], args[12:]) if hist else (None, args[11:])
    assert tail == [None]
    if hist is None:
        assert h is None
    else:
        assert bytes(h) == struct_of(_abi.UnrollHist, **hist)
        assert [getattr(h, k) for k in ("st", "g", "m", "v", "g_final")] == [addr(hist.get(k)) for k in ("st", "g", "m", "v", "g_final")]


def test_unroll_workspace_is_reused_grown_and_absent():
    eng, spec, p = StubEngine(48), spec_of(ORACLE_CFGS["dm"]), problem()
    run = lambda: eng.unroll(spec, f32(5), p, f32(2, 4), f32(40), None, None, 2, 1, f32(6))
    run()
    ws0 = eng._workspace
    eng.lib.size = 16
    run()
    assert eng._workspace is ws0 and val(eng.lib.last("l2o_unroll")[10]) == ws0.data_ptr()
    eng.lib.size = 49
    run()
    ws1 = eng._workspace
    assert ws1 is not ws0 and ws1.numel() == 49 and not ws1.any() and eng._last_ws is ws1
    assert "l2o_unroll_workspace_init" not in eng.lib.symbols()      # (a fresh buffer is zero; the layout never moved)
    eng.lib.size = 0                                                  # a form without a workspace
    n_calls = len(eng.lib.calls)
    run()
    assert eng.lib.symbols()[n_calls:] == ["l2o_unroll_workspace_bytes", "l2o_unroll"]
    assert eng.lib.last("l2o_unroll")[10] is None and eng._last_ws is None and eng._workspace is ws1


# ---- 3. the small passes that keep a scratch buffer --------------------------------------------------------------------
def test_problem_hvp():
    eng, p = StubEngine(), problem(B=3)
    x, u, out = f32(3, 4), f32(3, 4), f32(3, 4)
    eng.problem_hvp(p, x, u, out)
    assert eng.lib.symbols() == ["l2o_problem_hvp"]
    s0 = eng._hvp_scratch
    args = args_of(eng)
    assert bytes(args[0]) == problem_struct(p) and args[1:] == [x.data_ptr(), u.data_ptr(), out.data_ptr(), s0.data_ptr(), None]
    assert s0.dtype == torch.float32 and s0.numel() == 3
    eng.problem_hvp(problem(B=2), f32(2, 4), f32(2, 4), f32(2, 4))
    assert eng._hvp_scratch is s0 and args_of(eng)[4] == s0.data_ptr()
    eng.problem_hvp(problem(B=4), f32(4, 4), f32(4, 4), f32(4, 4))
    s1 = eng._hvp_scratch
    assert s1 is not s0 and s1.numel() == 4 and args_of(eng)[4] == s1.data_ptr()


class DimsLib(RecordingLib):
    """... whose l2o_cwlstm_wgrad_dims answers (KA, KB)."""

    def __init__(self, size, ka, kb):
        RecordingLib.__init__(self, size)
        self.ka, self.kb = ka, kb

    def l2o_cwlstm_wgrad_dims(self, cc, ka, kb):
        self.calls.append(("l2o_cwlstm_wgrad_dims", (cc, ka, kb)))
        ka._obj.value, kb._obj.value = self.ka, self.kb
        return 0


def test_atb_wgrad_and_wgrad_compact_share_one_workspace():
    """l2o_atb_workspace_bytes answers in BYTES; the buffer is held as floats: 10 bytes are 3 floats, 12 still 3, 13 are 4."""
    eng, spec = StubEngine(), spec_of(ORACLE_CFGS["dm"])
    eng.lib = lib = DimsLib(10, 41, 5)
    A, B = f32(6, 41), f32(6, 5)
    out = eng.atb(A, B)
    assert lib.symbols() == ["l2o_atb_workspace_bytes", "l2o_atb"] and lib.calls[0][1] == (6, 41, 5)
    ws0 = eng._atb_ws
    assert ws0.dtype == torch.float32 and ws0.numel() == 3 and tuple(out.shape) == (41, 5) and out.dtype == torch.float32
    assert args_of(eng) == [A.data_ptr(), B.data_ptr(), 6, 41, 5, out.data_ptr(), ws0.data_ptr(), None]

    lib.size, n_calls = 12, len(lib.calls)
    out = eng.wgrad(spec, A, B)
    assert lib.symbols()[n_calls:] == ["l2o_cwlstm_wgrad_dims", "l2o_atb_workspace_bytes", "l2o_cwlstm_wgrad"]
    assert lib.calls[n_calls + 1][1] == (6, 41, 5) and eng._atb_ws is ws0 and tuple(out.shape) == (41, 5)
    args = args_of(eng)
    assert bytes(args[0]) == net_cfg(spec) and args[1:] == [A.data_ptr(), B.data_ptr(), 6, out.data_ptr(), ws0.data_ptr(), None]
    with pytest.raises(AssertionError):
        eng.wgrad(spec, f32(6, 40), B)

    lib.size, n_calls = 13, len(lib.calls)
    Ac, Bm = f32(3, 4, 1), f32(2, 4, 5)
    out = eng.wgrad_compact(spec, Ac, Bm)
    assert lib.symbols()[n_calls:] == ["l2o_cwlstm_wgrad_dims", "l2o_atb_workspace_bytes", "l2o_cwlstm_wgrad_compact"]
    assert lib.calls[n_calls + 1][1] == (8, 41, 5)
    ws1 = eng._atb_ws
    assert ws1 is not ws0 and ws1.numel() == 4 and tuple(out.shape) == (41, 5)
    args = args_of(eng)
    assert bytes(args[0]) == net_cfg(spec)
    assert args[1:] == [Ac.data_ptr(), Bm.data_ptr(), 2, 4, out.data_ptr(), ws1.data_ptr(), None]
    with pytest.raises(AssertionError):
        eng.wgrad_compact(spec, f32(3, 4, 2), Bm)
    lib.size = 4
    eng.atb(A, B)
    assert eng._atb_ws is ws1 and args_of(eng)[6] == ws1.data_ptr()


def test_colsum():
    eng = StubEngine(12)
    A = f32(5, 3)
    out = eng.colsum(A)
    assert eng.lib.symbols() == ["l2o_colsum_scratch_floats", "l2o_colsum"] and eng.lib.calls[0][1] == (1, 3)
    s0 = eng._colsum_scratch
    assert s0.dtype == torch.float32 and s0.numel() == 12 and tuple(out.shape) == (3,)
    assert args_of(eng) == [A.data_ptr(), 1, 5, 3, out.data_ptr(), 0, s0.data_ptr(), None]
    eng.lib.size = 7
    A3, mine = f32(2, 5, 3), f32(2, 3)
    assert eng.colsum(A3, out=mine, accumulate=True) is mine and eng.lib.calls[-2][1] == (2, 3)
    assert eng._colsum_scratch is s0 and args_of(eng) == [A3.data_ptr(), 2, 5, 3, mine.data_ptr(), 1, s0.data_ptr(), None]
    assert tuple(eng.colsum(A3).shape) == (2, 3)
    eng.lib.size = 13
    eng.colsum(A)
    s1 = eng._colsum_scratch
    assert s1 is not s0 and s1.numel() == 13 and args_of(eng)[6] == s1.data_ptr()


# ---- 4. the step-path optimizees ---------------------------------------------------------------------------------------
def image_net_case(kind, struct, batch_norm, nvars):
    entry = _engine.step_optimizee(kind)
    images, labels = f32(9, 12), i32(9)

    def desc(batch=4):
        return entry.desc(batch, batch_norm, images, labels)

    def want(d):
        return struct_of(struct, batch=d.batch, n_data=9, batch_norm=int(batch_norm), flags=0, images=images, labels=labels)
    return dict(entry=entry, desc=desc, want=want, nvars=nvars,
                unsupported="%s_fg: unsupported minibatch 4" % entry.stem,
                miscount=lambda n: "%s_fg: %d variables for batch_norm=%r" % (entry.stem, n, batch_norm))


def mlp_deep_case(hidden):
    images, labels = f32(9, 6), i32(9)

    def desc(batch=4):
        return _engine.MlpDeepDesc(6, hidden, 10, batch, 1, images, labels)

    def want(d):
        return struct_of(_abi.MlpDeep, n_in=6, n_out=10, batch=d.batch, activation=1, n_data=9, n_hidden_layers=len(hidden),
                         hidden=hidden, images=images, labels=labels)
    return dict(entry=_engine.step_optimizee(5), desc=desc, want=want, nvars=2 * len(hidden) + 2,
                unsupported="l2o_mlp_deep_fg: unsupported MLP shape %r" % (hidden,), miscount=None)


def vgg16_case():
    images, labels, channels = f32(9, 12), i32(9), (8, 16, 24, 32, 40)

    def desc(batch=4):
        return _engine.Vgg16Desc(batch, channels, images, labels)

    def want(d):
        return struct_of(_abi.Vgg16, batch=d.batch, n_data=9, flags=0, channels=channels, images=images, labels=labels)
    return dict(entry=_engine.step_optimizee(10), desc=desc, want=want, nvars=28,
                unsupported="l2o_vgg16_fg: unsupported minibatch 4 or channels (8, 16, 24, 32, 40)",
                miscount=lambda n: "l2o_vgg16_fg: %d variables (it takes 28)" % n)


FG_CASES = {
    "mlp_deep-2": lambda: mlp_deep_case((20, 12)),
    "mlp_deep-3": lambda: mlp_deep_case((20, 12, 7)),
    "mnist_conv-bn": lambda: image_net_case(6, _abi.MnistConv, True, 10),
    "mnist_conv": lambda: image_net_case(6, _abi.MnistConv, False, 6),
    "cifar_conv-bn": lambda: image_net_case(7, _abi.CifarConv, True, 10),
    "cifar_conv": lambda: image_net_case(7, _abi.CifarConv, False, 6),
    "lenet-bn": lambda: image_net_case(8, _abi.Lenet, True, 14),
    "lenet": lambda: image_net_case(8, _abi.Lenet, False, 10),
    "vgg16": vgg16_case,
    "nas-bn": lambda: image_net_case(11, _abi.Nas, True, 18),
    "nas": lambda: image_net_case(11, _abi.Nas, False, 10),
}
FG_METHODS = {5: "mlp_deep_fg", 6: "mnist_conv_fg", 7: "cifar_conv_fg", 8: "lenet_fg", 10: "vgg16_fg", 11: "nas_fg"}


@pytest.mark.parametrize("with_grads", [False, True])
@pytest.mark.parametrize("case", list(FG_CASES))
def test_indexed_fg_arguments(case, with_grads):
    k = FG_CASES[case]()
    entry, nv = k["entry"], k["nvars"]
    kind = [n for n in FG_METHODS if _engine.step_optimizee(n) is entry][0]
    assert entry.method == FG_METHODS[kind]
    eng, d = StubEngine(30), k["desc"]()
    fg = getattr(eng, FG_METHODS[kind])
    idx, ws, loss = i32(4), [f32(2) for _ in range(nv)], f32(1)
    grads = [f32(2) for _ in range(nv)] if with_grads else None
    fg(d, idx, ws, loss, grads)
    assert eng.lib.symbols() == [entry.stem + "_scratch_floats", entry.stem + "_fg"]
    assert type(val(eng.lib.calls[0][1][0])) is entry.struct and bytes(val(eng.lib.calls[0][1][0])) == k["want"](d)
    s0 = getattr(eng, entry.scratch)
    assert s0.dtype == torch.float32 and s0.numel() == 30
    args = args_of(eng)
    assert type(args[0]) is entry.struct and bytes(args[0]) == k["want"](d) and args[1] == idx.data_ptr()
    assert len(args[2]) == nv and list(args[2]) == [t.data_ptr() for t in ws] and args[3] == loss.data_ptr()
    if with_grads:
        assert len(args[4]) == nv and list(args[4]) == [t.data_ptr() for t in grads]
    else:
        assert args[4] is None
    assert args[5:] == [s0.data_ptr(), None]
    # the scratch: kept for a smaller request, replaced for a larger one
    eng.lib.size = 8
    fg(k["desc"](2), idx, ws, loss, grads)
    assert getattr(eng, entry.scratch) is s0 and args_of(eng)[5] == s0.data_ptr() and args_of(eng)[0].batch == 2
    eng.lib.size = 31
    fg(d, idx, ws, loss, grads)
    s1 = getattr(eng, entry.scratch)
    assert s1 is not s0 and s1.numel() == 31 and args_of(eng)[5] == s1.data_ptr()


@pytest.mark.parametrize("case", list(FG_CASES))
def test_indexed_fg_refusals(case):
    k = FG_CASES[case]()
    entry, nv = k["entry"], k["nvars"]
    eng, d = StubEngine(30), k["desc"]()
    fg = getattr(eng, entry.method)
    idx, ws, loss = i32(4), [f32(2) for _ in range(nv)], f32(1)
    if k["miscount"] is not None:
        for bad_ws, bad_grads, n in ((ws[:-1], None, nv - 1), (ws + [f32(2)], None, nv + 1), (ws, ws[:-1], nv),
                                     (ws[:-1], ws[:-1], nv - 1)):
            with pytest.raises(ValueError) as err:
                fg(d, idx, bad_ws, loss, bad_grads)
            assert type(err.value) is ValueError and str(err.value) == k["miscount"](n)
        assert [s for s in eng.lib.symbols() if not s.endswith("_scratch_floats")] == []
    # a size query of 0: the library has no kernel for the shape -- said before anything else is looked at
    eng = StubEngine(0)
    fg = getattr(eng, entry.method)
    for bad_ws in (ws, ws[:-1]):
        with pytest.raises(_abi.L2OUnsupported) as err:
            fg(d, idx, bad_ws, loss, None)
        assert str(err.value) == "libl2o_hip error -2: " + k["unsupported"] and err.value.code == _abi.L2O_ERR_UNSUPPORTED
    assert [s for s in eng.lib.symbols() if not s.endswith("_scratch_floats")] == []
    assert entry.scratch not in eng.__dict__


def test_vgg16_fg_refuses_other_than_five_blocks_without_asking():
    eng = StubEngine(30)
    d = _engine.Vgg16Desc(4, (8, 16, 24, 32), f32(9, 12), i32(9))
    with pytest.raises(_abi.L2OUnsupported) as err:
        eng.vgg16_fg(d, i32(4), [f32(2) for _ in range(28)], f32(1), None)
    assert str(err.value) == "libl2o_hip error -2: l2o_vgg16_fg: unsupported minibatch 4 or channels (8, 16, 24, 32)"
    assert eng.lib.calls == []


@pytest.mark.parametrize("with_grads", [False, True])
@pytest.mark.parametrize("inference", [False, True])
def test_confocal_fg_arguments(inference, with_grads):
    eng, d, nv = StubEngine(30), confocal_desc(inference), 13
    theta, loss = [f32(3) for _ in range(nv)], f32(1)
    sim = None if inference else [f32(3) for _ in range(nv)]
    grads = [f32(3) for _ in range(nv)] if with_grads else None
    eng.confocal_fg(d, theta, sim, loss, grads)
    assert eng.lib.symbols() == ["l2o_confocal_scratch_floats", "l2o_confocal_fg"]
    assert bytes(val(eng.lib.calls[0][1][0])) == confocal_struct(d)
    s0 = eng._confocal_scratch
    args = args_of(eng)
    assert bytes(args[0]) == confocal_struct(d) and len(args[1]) == nv and list(args[1]) == [t.data_ptr() for t in theta]
    assert (args[2] is None) if inference else (len(args[2]) == nv and list(args[2]) == [t.data_ptr() for t in sim])
    assert args[3] == loss.data_ptr()
    assert (list(args[4]) == [t.data_ptr() for t in grads] and len(args[4]) == nv) if with_grads else args[4] is None
    assert args[5:] == [s0.data_ptr(), None] and s0.numel() == 30 and s0.dtype == torch.float32
    eng.lib.size = 29
    eng.confocal_fg(d, theta, sim, loss, grads)
    assert eng._confocal_scratch is s0
    eng.lib.size = 31
    eng.confocal_fg(d, theta, sim, loss, grads)
    assert eng._confocal_scratch is not s0 and eng._confocal_scratch.numel() == 31
    assert args_of(eng)[5] == eng._confocal_scratch.data_ptr()
    # the refusals: a wrong variable count; a size query of 0, said first
    with pytest.raises(ValueError) as err:
        eng.confocal_fg(d, theta[:12], sim, loss, grads)
    assert type(err.value) is ValueError and str(err.value) == "l2o_confocal_fg: 12 variables for 2 points"
    eng.lib.size = 0
    with pytest.raises(_abi.L2OUnsupported) as err:
        eng.confocal_fg(d, theta[:12], sim, loss, grads)
    assert str(err.value) == ("libl2o_hip error -2: l2o_confocal_fg: batch in [1, 1024], num_points in [1, 8], ROI edges in "
                              "[2, 32] (got 3, 2, (2, 3, 2))")
