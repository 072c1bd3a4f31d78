"""The fused-unroll host paths without a GPU: what HipEngine's four fused methods (mlp_unroll, mlp_unroll_multi,
confocal_unroll, confocal_unroll_multi; plain and recording) hand to the library -- symbol, struct bytes, every pointer
array element by element, the cached workspace / scratch -- on an engine whose `lib` records instead of launching; the
launch memo and the buffer caches; the refusals and their texts; and the graph / Replicas side of the MLP forms on an
oracle-backed engine that claims the kernels (the confocal side: test_confocal_replicas_cpu.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle as O
from helpers import ORACLE_CFGS, make_params, spec_of
from oracle_engine import OracleEngine
from open_l2o_amd import _abi, _engine, meta, problems
from open_l2o_amd._engine import ConfocalDesc, HipEngine, MlpDesc
from open_l2o_amd._graph_core import _term_vars
from test_replica_training_cpu import make_replicas

SIZE_QUERIES = ("_scratch_floats", "_workspace_bytes")


class RecordingLib(object):
    """Stands in for libl2o_hip.so: every symbol records (symbol, args) and returns 0; the size queries return `size`."""

    def __init__(self, size=64):
        self.size, self.calls = size, []

    def __getattr__(self, name):
        if not name.startswith("l2o_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, args))
            return self.size if name.endswith(SIZE_QUERIES) else 0
        return fn

    def symbols(self):
        return [name for name, _ in self.calls]

    def last(self, name):
        return [args for sym, args in self.calls if sym == name][-1]


class StubEngine(HipEngine):
    def __init__(self, size=64):
        self.device = torch.device("cpu")
        self.lib = RecordingLib(size)
        self._workspace = self._last_ws = self._mlp_scratch = None

    def _stream(self):
        return None


def val(a):
    """What a recorded ctypes argument holds: the address of a c_void_p, the struct / array behind a byref."""
    if isinstance(a, C.c_void_p):
        return a.value
    return a._obj if type(a).__name__ == "CArgObject" else a


def addr(t):
    return None if t is None else t.data_ptr()


def elems(a):
    return None if a is None else list(a)


def f32(*shape):
    return torch.zeros(*shape, dtype=torch.float32)


def net_cfg(spec):
    assert tuple(spec.layers) == (20, 20)
    c = _abi.NetCfg(kind=spec.kind, preprocess=spec.preprocess, n_layers=2, hidden=20, tanh_output=int(spec.tanh_output),
                    scale=spec.scale, logsign_k=spec.logsign_k, beta1=spec.beta1, beta2=spec.beta2, options=_abi.options_word())
    return bytes(c)


def fill(array, ts):
    for k, t in enumerate(ts):
        array[k] = addr(t)


def hist_struct(cls, hist):
    h = cls()
    for k in ("st", "g", "m", "v"):
        if hist.get(k) is not None:
            fill(getattr(h, k), hist[k])
    return bytes(h)


def var_lists(nv, rnnprop, n=3):
    """xs, sts, ms, vs, scales of nv variables (DM: no moments; scales: some set, some not)."""
    xs, sts = [f32(n) for _ in range(nv)], [f32(8) for _ in range(nv)]
    ms = [f32(n) if rnnprop else None for _ in range(nv)]
    vs = [f32(n) if rnnprop else None for _ in range(nv)]
    scales = [f32(n) if k % 2 else None for k in range(nv)]
    return xs, sts, ms, vs, scales


def hist_of(nv, rnnprop, T, n=3):
    h = dict(st=[f32(T, 8) for _ in range(nv)], g=[f32(T + 1, n) for _ in range(nv)], m=None, v=None)
    if rnnprop:
        h.update(m=[f32(T + 1, n) for _ in range(nv)], v=[f32(T + 1, n) for _ in range(nv)])
    return h


def mlp_desc():
    return MlpDesc(n_in=6, n_hidden=20, n_out=10, batch=64, activation=0, images=f32(11, 6),
                   labels=torch.zeros(11, dtype=torch.int32))


def mlp_struct(d):
    return bytes(_abi.Mlp(n_in=d.n_in, n_hidden=d.n_hidden, n_out=d.n_out, batch=d.batch, activation=d.activation, n_data=11,
                          flags=0, images=d.images.data_ptr(), labels=d.labels.data_ptr()))


def confocal_struct(d):
    c = _abi.Confocal(batch=d.batch, num_points=d.num_points, inference=0 if d.img is None else 1, flags=0, img=addr(d.img))
    c.roi[0], c.roi[1], c.roi[2] = d.roi
    return bytes(c)


CASES = [("dm", False), ("rnnprop", True)]


# ---- 1. marshalling ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("record", [False, True])
@pytest.mark.parametrize("name,rnnprop", CASES)
def test_mlp_unroll_arguments(name, rnnprop, record):
    eng, spec, d, T = StubEngine(96), spec_of(ORACLE_CFGS[name]), mlp_desc(), 3
    wpack, idx, fx = f32(5), torch.zeros(T + 1, 64, dtype=torch.int32), f32(T + 1)
    xs, sts, ms, vs, scales = var_lists(4, rnnprop)
    hist = hist_of(4, rnnprop, T) if record else None
    eng.mlp_unroll(spec, wpack, d, idx, xs, sts, ms, vs, scales, T, 7, fx, hist=hist)
    sym = "l2o_mlp_unroll_record" if record else "l2o_mlp_unroll"
    assert eng.lib.symbols() == ["l2o_mlp_unroll_workspace_bytes", sym]
    args = [val(a) for a in eng.lib.calls[-1][1]]
    assert bytes(args[0]) == net_cfg(spec) and args[1] == wpack.data_ptr() and bytes(args[2]) == mlp_struct(d)
    assert args[3] == idx.data_ptr()
    for got, ts in zip(args[4:9], (xs, sts, ms, vs, scales)):
        assert len(got) == 4 and list(got) == [addr(t) for t in ts]
    assert args[9:12] == [T, 7, fx.data_ptr()]
    tail = args[12:]
    if record:
        assert bytes(tail.pop(0)) == hist_struct(_abi.MlpHist, hist)
    ws = eng._mlp_ws
    assert tail == [ws.data_ptr(), None] and eng._last_ws is ws
    assert ws.dtype == torch.uint8 and ws.numel() == 96 and not ws.any()


def mlp_instances(n, rnnprop, T):
    out = []
    for _ in range(n):
        xs, sts, ms, vs, scales = var_lists(4, rnnprop)
        out.append(dict(indices=torch.zeros(T + 1, 64, dtype=torch.int32), xs=xs, sts=sts, ms=ms, vs=vs, scales=scales,
                        fx=f32(T + 1)))
    return out


@pytest.mark.parametrize("record", [False, True])
@pytest.mark.parametrize("name,rnnprop", CASES)
def test_mlp_unroll_multi_arguments(name, rnnprop, record):
    eng, spec, d, T, n = StubEngine(160), spec_of(ORACLE_CFGS[name]), mlp_desc(), 2, 3
    wpack, insts = f32(5), mlp_instances(n, rnnprop, T)
    hists = [hist_of(4, rnnprop, T) for _ in range(n)] if record else None
    eng.mlp_unroll_multi(spec, wpack, d, insts, T, 4, hists=hists)
    sym = "l2o_mlp_unroll_multi_record" if record else "l2o_mlp_unroll_multi"
    assert eng.lib.symbols() == ["l2o_mlp_unroll_multi_workspace_bytes", sym]
    assert eng.lib.calls[0][1][1] == n
    args = [val(a) for a in eng.lib.calls[-1][1]]
    assert bytes(args[0]) == net_cfg(spec) and args[1] == wpack.data_ptr() and bytes(args[2]) == mlp_struct(d)
    want = (_abi.MlpInstance * n)()
    for w, i in zip(want, insts):
        w.indices, w.fx = i["indices"].data_ptr(), i["fx"].data_ptr()
        for field, k in (("x", "xs"), ("st", "sts"), ("m", "ms"), ("v", "vs"), ("x_scale", "scales")):
            fill(getattr(w, field), i[k])
    assert len(args[3]) == n and bytes(args[3]) == bytes(want)
    for got, i in zip(args[3], insts):                       # (element by element, in order)
        assert list(got.x) == [t.data_ptr() for t in i["xs"]] and list(got.st) == [t.data_ptr() for t in i["sts"]]
        assert list(got.m) == [addr(t) for t in i["ms"]] and list(got.v) == [addr(t) for t in i["vs"]]
        assert list(got.x_scale) == [addr(t) for t in i["scales"]]
    assert args[4:7] == [n, T, 4]
    tail = args[7:]
    if record:
        harr = tail.pop(0)
        assert len(harr) == n and bytes(harr) == b"".join(hist_struct(_abi.MlpHist, h) for h in hists)
    ws = eng._mlp_ws
    assert tail == [ws.data_ptr(), None] and eng._last_ws is ws
    assert ws.dtype == torch.uint8 and ws.numel() == 160 and not ws.any()


def confocal_desc(inference, batch=3, points=2, roi=(2, 3, 2)):
    return ConfocalDesc(batch=batch, num_points=points, roi=roi, img=f32(batch, int(np.prod(roi))) if inference else None)


@pytest.mark.parametrize("record", [False, True])
@pytest.mark.parametrize("name,rnnprop,inference", [("dm", False, False), ("rnnprop", True, False), ("dm", False, True)])
def test_confocal_unroll_arguments(name, rnnprop, inference, record):
    eng, spec, d, T = StubEngine(50), spec_of(ORACLE_CFGS[name]), confocal_desc(inference), 3
    nv = 13
    wpack, fx = f32(5), f32(T + 1)
    xs, sts, ms, vs, scales = var_lists(nv, rnnprop)
    if not rnnprop:
        scales = [None] * nv                                 # (the DM case: ms / vs / scales all absent -> NULL arrays)
    sim = None if inference else [f32(3) for _ in range(nv)]
    hist = hist_of(nv, rnnprop, T) if record else None
    eng.confocal_unroll(spec, wpack, d, xs, sts, ms, vs, scales, sim, T, 5, fx, hist=hist)
    sym = "l2o_confocal_unroll_record" if record else "l2o_confocal_unroll"
    assert eng.lib.symbols() == ["l2o_confocal_unroll_scratch_floats", sym]
    assert eng.lib.calls[0][1][1] == T
    args = [val(a) for a in eng.lib.calls[-1][1]]
    assert bytes(args[0]) == net_cfg(spec) and args[1] == wpack.data_ptr() and bytes(args[2]) == confocal_struct(d)
    for got, ts in zip(args[3:5], (xs, sts)):
        assert len(got) == nv and list(got) == [t.data_ptr() for t in ts]
    for got, ts in zip(args[5:8], (ms, vs, scales)):
        if rnnprop:
            assert len(got) == nv and list(got) == [addr(t) for t in ts]
        else:
            assert got is None
    assert elems(args[8]) == (None if inference else [t.data_ptr() for t in sim])
    assert args[9:12] == [T, 5, fx.data_ptr()]
    tail = args[12:]
    if record:
        assert bytes(tail.pop(0)) == hist_struct(_abi.ConfocalHist, hist)
    scr = eng._confocal_unroll_scratch
    assert tail == [scr.data_ptr(), None] and scr.dtype == torch.float32 and scr.numel() >= 50


def confocal_instances(n, rnnprop, inference, nv=13):
    out = []
    for _ in range(n):
        xs, sts, ms, vs, scales = var_lists(nv, rnnprop)
        out.append(dict(xs=xs, sts=sts, ms=ms, vs=vs, scales=scales, sim=None if inference else [f32(3) for _ in range(nv)],
                        img=f32(3, 12) if inference else None, fx=f32(4)))
    return out


@pytest.mark.parametrize("record", [False, True])
@pytest.mark.parametrize("name,rnnprop,inference", [("dm", False, False), ("rnnprop", True, False), ("dm", False, True)])
def test_confocal_unroll_multi_arguments(name, rnnprop, inference, record):
    eng, spec, d, T, n, nv = StubEngine(70), spec_of(ORACLE_CFGS[name]), confocal_desc(inference), 3, 2, 13
    wpack, insts = f32(5), confocal_instances(n, rnnprop, inference)
    hists = [hist_of(nv, rnnprop, T) for _ in range(n)] if record else None
    eng.confocal_unroll_multi(spec, wpack, d, insts, T, 6, hists=hists)
    sym = "l2o_confocal_unroll_multi_record" if record else "l2o_confocal_unroll_multi"
    assert eng.lib.symbols() == ["l2o_confocal_unroll_multi_scratch_floats", sym]
    assert eng.lib.calls[0][1][1:] == (n, T)
    args = [val(a) for a in eng.lib.calls[-1][1]]
    assert bytes(args[0]) == net_cfg(spec) and args[1] == wpack.data_ptr() and bytes(args[2]) == confocal_struct(d)
    want = (_abi.ConfocalInstance * n)()
    for w, i in zip(want, insts):
        w.fx, w.img = i["fx"].data_ptr(), addr(i["img"])
        for field, k in (("x", "xs"), ("st", "sts"), ("m", "ms"), ("v", "vs"), ("x_scale", "scales")):
            fill(getattr(w, field), i[k])
        if not inference:
            fill(w.sim, i["sim"])
    assert len(args[3]) == n and bytes(args[3]) == bytes(want)
    for got, i in zip(args[3], insts):
        assert list(got.x)[:nv] == [t.data_ptr() for t in i["xs"]] and list(got.st)[:nv] == [t.data_ptr() for t in i["sts"]]
        assert list(got.m)[:nv] == [addr(t) for t in i["ms"]] and list(got.v)[:nv] == [addr(t) for t in i["vs"]]
        assert list(got.x_scale)[:nv] == [addr(t) for t in i["scales"]]
        assert list(got.sim)[:nv] == ([None] * nv if inference else [t.data_ptr() for t in i["sim"]])
        assert got.img == addr(i["img"]) and got.fx == i["fx"].data_ptr()
    assert args[4:7] == [n, T, 6]
    tail = args[7:]
    if record:
        harr = tail.pop(0)
        assert len(harr) == n and bytes(harr) == b"".join(hist_struct(_abi.ConfocalHist, h) for h in hists)
    scr = eng._confocal_multi_scratch
    assert tail == [scr.data_ptr(), None] and scr.dtype == torch.float32 and scr.numel() >= 70


# ---- 2. caches ---------------------------------------------------------------------------------------------------------
def mlp_call(eng, fixed, T, hist=None):
    spec, wpack, d, idx, lists, fx = fixed
    eng.mlp_unroll(spec, wpack, d, idx, *lists, T, 1, fx, hist=hist)
    return eng.lib.calls[-1][1]


def mlp_fixed():
    return (spec_of(O.RNNPROP), f32(5), mlp_desc(), torch.zeros(12, 64, dtype=torch.int32), var_lists(4, True), f32(12))


def test_mlp_unroll_memo_hit_recording_bypass_and_eviction():
    eng, fixed = StubEngine(64), mlp_fixed()
    first = mlp_call(eng, fixed, 1)
    n_calls = len(eng.lib.calls)
    second = mlp_call(eng, fixed, 1)
    assert eng.lib.symbols()[n_calls:] == ["l2o_mlp_unroll"]                       # no size query on a hit
    assert all(a is b for a, b in zip(first[4:9], second[4:9]))                     # the identical ctypes arrays
    assert val(first[0]) is val(second[0]) and val(first[2]) is val(second[2])
    memo = eng._mlp_unroll_memo
    assert len(memo) == 1
    # a recording call neither reads nor enters the memo
    for _ in range(2):
        n_calls = len(eng.lib.calls)
        rec = mlp_call(eng, fixed, 1, hist=hist_of(4, True, 1))
        assert eng.lib.symbols()[n_calls:] == ["l2o_mlp_unroll_workspace_bytes", "l2o_mlp_unroll_record"]
        assert rec[4] is not first[4] and len(memo) == 1
    # eight entries at most: the ninth distinct key evicts the first
    for T in range(2, 9):
        mlp_call(eng, fixed, T)
    assert len(memo) == 8
    n_calls = len(eng.lib.calls)
    mlp_call(eng, fixed, 1)
    assert eng.lib.symbols()[n_calls:] == ["l2o_mlp_unroll"]                       # (still there)
    mlp_call(eng, fixed, 9)
    assert len(memo) == 8
    n_calls = len(eng.lib.calls)
    again = mlp_call(eng, fixed, 1)
    assert eng.lib.symbols()[n_calls:] == ["l2o_mlp_unroll_workspace_bytes", "l2o_mlp_unroll"]
    assert again[4] is not first[4] and len(memo) == 8


def test_larger_workspace_replaces_mlp_ws_and_rebuilds_the_stale_entry():
    eng, fixed = StubEngine(64), mlp_fixed()
    mlp_call(eng, fixed, 1)
    ws0 = eng._mlp_ws
    mlp_call(eng, fixed, 2)
    assert eng._mlp_ws is ws0                                                       # large enough: reused
    eng.lib.size = 128
    insts = mlp_instances(2, True, 3)
    eng.mlp_unroll_multi(fixed[0], fixed[1], fixed[2], insts, 3, 1)
    ws1 = eng._mlp_ws
    assert ws1 is not ws0 and ws1.numel() == 128 and not ws1.any() and ws1.dtype == torch.uint8
    n_calls = len(eng.lib.calls)
    args = mlp_call(eng, fixed, 1)                                                  # its memo entry holds ws0
    assert eng.lib.symbols()[n_calls:] == ["l2o_mlp_unroll_workspace_bytes", "l2o_mlp_unroll"]
    assert val(args[12]) == ws1.data_ptr() and eng._mlp_ws is ws1 and eng._last_ws is ws1
    n_calls = len(eng.lib.calls)
    eng.mlp_unroll_multi(fixed[0], fixed[1], fixed[2], insts, 3, 1)                 # the multi launch's entry: a hit
    assert eng.lib.symbols()[n_calls:] == ["l2o_mlp_unroll_multi"]


def test_confocal_scratch_buffers_are_reused_grown_and_separate():
    eng, spec, d = StubEngine(40), spec_of(O.DM_IDENTITY), confocal_desc(False)
    xs, sts, ms, vs, scales = var_lists(13, False)
    sim = [f32(3) for _ in range(13)]

    def single():
        eng.confocal_unroll(spec, f32(5), d, xs, sts, ms, vs, scales, sim, 2, 1, f32(3))
        return eng._confocal_unroll_scratch

    def multi():
        eng.confocal_unroll_multi(spec, f32(5), d, confocal_instances(2, False, False), 2, 1)
        return eng._confocal_multi_scratch
    s0, m0 = single(), multi()
    assert s0 is not m0 and s0.data_ptr() != m0.data_ptr()
    assert single() is s0 and multi() is m0
    eng.lib.size = 24                                                               # smaller: still large enough
    assert single() is s0 and multi() is m0
    eng.lib.size = 41
    s1, m1 = single(), multi()
    assert s1 is not s0 and m1 is not m0 and s1 is not m1 and s1.numel() >= 41 and m1.numel() >= 41
    assert val(eng.lib.last("l2o_confocal_unroll")[12]) == s1.data_ptr()
    assert val(eng.lib.last("l2o_confocal_unroll_multi")[7]) == m1.data_ptr()


# ---- 3. refusals -------------------------------------------------------------------------------------------------------
def test_a_size_of_zero_is_unsupported():
    eng, spec, d = StubEngine(0), spec_of(O.DM_IDENTITY), confocal_desc(False)
    xs, sts, ms, vs, scales = var_lists(13, False)
    sim = [f32(3) for _ in range(13)]
    with pytest.raises(_abi.L2OUnsupported) as err:
        eng.confocal_fg(d, xs, sim, f32(1), None)
    assert str(err.value) == ("libl2o_hip error -2: l2o_confocal_fg: batch in [1, 1024], num_points in [1, 8], ROI edges in "
                              "[2, 32] (got 3, 2, (2, 3, 2))")
    with pytest.raises(_abi.L2OUnsupported) as err:
        eng.confocal_unroll(spec, f32(5), d, xs, sts, ms, vs, scales, sim, 2, 1, f32(3))
    assert str(err.value) == ("libl2o_hip error -2: l2o_confocal_unroll: batch in [1, 1024], num_points in [1, 8], ROI edges "
                              "in [2, 32] (got 3, 2, (2, 3, 2))")
    with pytest.raises(_abi.L2OUnsupported) as err:
        eng.confocal_unroll_multi(spec, f32(5), d, confocal_instances(2, False, False), 2, 1)
    assert str(err.value) == ("libl2o_hip error -2: l2o_confocal_unroll_multi: batch in [1, 1024], num_points in [1, 8], ROI "
                              "edges in [2, 32], 1 to 32 instances (got 3, 2, (2, 3, 2), 2)")
    with pytest.raises(_abi.L2OUnsupported) as err:
        eng.mlp_unroll_multi(spec, f32(5), mlp_desc(), mlp_instances(2, False, 2), 2, 1)
    assert str(err.value) == "libl2o_hip error -2: l2o_mlp_unroll_multi: unsupported shape / instance count"
    assert [s for s in eng.lib.symbols() if not s.endswith(SIZE_QUERIES)] == []     # nothing was launched


def test_confocal_argument_errors():
    eng, spec, d = StubEngine(40), spec_of(O.DM_IDENTITY), confocal_desc(False)
    xs, sts, ms, vs, scales = var_lists(13, False)
    sim, wpack, fx, img = [f32(3) for _ in range(13)], f32(5), f32(3), f32(3, 12)

    def fg(theta=xs, sim=sim, grads=None, d=d):
        eng.confocal_fg(d, theta, sim, f32(1), grads)

    def unroll(xs=xs, sts=sts, sim=sim, d=d):
        eng.confocal_unroll(spec, wpack, d, xs, sts, ms, vs, scales, sim, 2, 1, fx)

    def multi(d=d, hists=None, **kw):
        insts = confocal_instances(2, False, False)
        insts[1].update(kw)
        eng.confocal_unroll_multi(spec, wpack, d, insts, 2, 1, hists=hists)
    count = r"^l2o_confocal_%s: %d variables for 2 points$"
    # a wrong variable count
    with pytest.raises(ValueError, match=count % ("fg", 12)):
        fg(theta=xs[:12])
    with pytest.raises(ValueError, match=count % ("fg", 13)):
        fg(grads=xs[:12])
    with pytest.raises(ValueError, match=count % ("unroll", 12)):
        unroll(xs=xs[:12])
    with pytest.raises(ValueError, match=count % ("unroll", 13)):
        unroll(sts=sts[:12])
    with pytest.raises(ValueError, match=count % ("unroll_multi", 12)):
        multi(xs=xs[:12])
    with pytest.raises(ValueError, match=count % ("unroll_multi", 13)):
        multi(sim=sim[:12])
    # sim given with img (inference mode takes img INSTEAD of the simulation parameters), or neither
    inf = confocal_desc(True)
    with pytest.raises(ValueError, match=count % ("fg", 13)):
        fg(d=inf)
    with pytest.raises(ValueError, match=count % ("fg", 13)):
        fg(sim=None)
    with pytest.raises(ValueError, match=count % ("unroll", 13)):
        unroll(d=inf)
    with pytest.raises(ValueError, match=count % ("unroll", 13)):
        unroll(sim=None)
    with pytest.raises(ValueError, match=count % ("unroll_multi", 13)):
        multi(d=inf, img=img)
    with pytest.raises(ValueError, match=count % ("unroll_multi", 13)):
        multi(sim=None)
    # a variable that is not [batch] floats, an image that is not [batch, V]
    floats = r"^l2o_confocal_%s: every variable holds \[batch\] floats, img \[batch, V\]$"
    bad = xs[:5] + [f32(4)] + xs[6:]
    with pytest.raises(ValueError, match=floats % "fg"):
        fg(theta=bad)
    with pytest.raises(ValueError, match=floats % "unroll"):
        unroll(xs=bad)
    with pytest.raises(ValueError, match=floats % "unroll_multi"):
        multi(xs=bad)
    small = ConfocalDesc(batch=3, num_points=2, roi=(2, 3, 2), img=f32(3, 11))
    with pytest.raises(ValueError, match=floats % "fg"):
        fg(d=small, sim=None)
    with pytest.raises(ValueError, match=floats % "unroll"):
        unroll(d=small, sim=None)
    insts = confocal_instances(2, False, True)
    insts[1]["img"] = f32(3, 11)
    with pytest.raises(ValueError, match=floats % "unroll_multi"):
        eng.confocal_unroll_multi(spec, wpack, inf, insts, 2, 1)
    # hists of the wrong length
    with pytest.raises(ValueError, match=r"^l2o_confocal_unroll_multi: one history per instance$"):
        multi(hists=[hist_of(13, False, 2)])
    with pytest.raises(ValueError, match=r"^mlp_unroll_multi: one history per instance$"):
        eng.mlp_unroll_multi(spec, wpack, mlp_desc(), mlp_instances(2, False, 2), 2, 1, hists=[hist_of(4, False, 2)])
    assert [s for s in eng.lib.symbols() if not s.endswith(SIZE_QUERIES)] == []     # nothing was launched


# ---- 4. graph and Replicas on an MLP engine that claims the kernels -----------------------------------------------------
class ClaimingMlp(OracleEngine):
    """An oracle-backed engine that claims the fused MLP kernels and records what their launches are given."""

    def __init__(self):
        super().__init__()
        self.asked, self.singles, self.multis = [], [], []

    def mlp_unroll_supported(self, spec, d):
        return 2

    def mlp_unroll(self, spec, wpack, d, indices, xs, sts, ms, vs, scales, T, step0, fx, hist=None):
        self.singles.append(dict(d=d, indices=indices, xs=xs, sts=sts, ms=ms, vs=vs, scales=scales, T=T, step0=step0, fx=fx,
                                 hist=hist))

    def mlp_unroll_multi_supported(self, spec, d, n):
        self.asked.append(n)
        return 1 <= n <= 8

    def mlp_unroll_multi(self, spec, wpack, d, instances, T, step0, hists=None):
        self.multis.append(dict(spec=spec, d=d, insts=list(instances), T=T, step0=step0, hists=hists))


@pytest.fixture
def claiming():
    eng = ClaimingMlp()
    old = _engine._default_engine
    _engine.set_default_engine(eng)
    yield eng
    _engine.set_default_engine(old)


def mnist_replicas(name, n, T, data=None):
    data = data or problems.synthetic_mnist(100, seed=22)
    params = make_params(ORACLE_CFGS[name], seed=42, trained_like=True)
    reps = make_replicas(name, params, data, [np.zeros((4 * (T + 1), 64), np.int64)] * n, T, seed=6)
    reps.reset()
    return reps


def feed_of(reps, step=1):
    return {reps.step: step} if reps.graphs[0].rnnprop else {}


@pytest.mark.parametrize("name", ["dm_logsign", "rnnprop"])
def test_mlp_instance_keys_and_variable_order(claiming, name):
    reps = mnist_replicas(name, 1, 2)
    g = reps.graphs[0]
    assert set(g.mlp_instance(dry=True)) == {"net", "desc"}
    inst = g.mlp_instance(feed_of(reps))
    assert set(inst) == {"net", "desc", "indices", "xs", "sts", "ms", "vs", "scales", "fx"}
    assert inst["net"] is g.slots[0].net and inst["desc"] is g._mlp_desc(g.terms[0]) and inst["indices"] is g._mlp_idx[0]
    by_name = {v.decl.name: j for j, v in enumerate(g.x)}
    js = [by_name[tv.name] for tv in _term_vars(g.terms[0])]                       # w1, b1, w2, b2
    assert [x.numel() for x in inst["xs"]] == [784 * 20, 20, 20 * 10, 10]
    slot_of = {s.var_index: s for s in g.slots}
    for k, j in enumerate(js):
        s = slot_of[j]
        assert inst["xs"][k].data_ptr() == g.x[j].value.data_ptr()
        assert inst["sts"][k] is s.state.packed and inst["ms"][k] is s.m and inst["vs"][k] is s.v
        assert (s.m is not None) == g.rnnprop
    assert inst["scales"] == [None] * 4
    assert inst["fx"] is g._fx_cache[2]["bufs"][0] and tuple(inst["fx"].shape) == (3,)
    if g.rnnprop:
        with pytest.raises(ValueError, match=r"^You must feed a value for placeholder 'step' \(DM/util.py:59-60\)$"):
            g.mlp_instance({})
    # the graph's own launch hands the same lists, in the same order, to the single-launch method
    g.launch(feed_of(reps, 3), True)
    assert g.last_path == "mlp_unroll" and len(claiming.singles) == 1
    one = claiming.singles[0]
    assert one["T"] == 2 and one["step0"] == (3 if g.rnnprop else 1) and one["hist"] is None and one["fx"] is inst["fx"]
    for k in ("xs", "sts", "ms", "vs"):
        assert [addr(t) for t in one[k]] == [addr(t) for t in inst[k]], k
    assert one["scales"] == [None] * 4 and one["indices"] is g._mlp_idx[0] and one["d"] is inst["desc"]
    rec = {}
    g.launch(feed_of(reps, 3), True, record=rec)
    assert g.last_path == "mlp_unroll" and claiming.singles[-1]["hist"] is g._mlp_record_plan["hist"]
    assert rec["plan"] is g._mlp_record_plan and rec["step0"] == one["step0"]


@pytest.mark.parametrize("no_recovery", [False, True])
def test_nine_replicas_go_out_as_8_1_in_order(claiming, monkeypatch, no_recovery):
    if no_recovery:
        monkeypatch.setenv("L2O_NO_RECOVERY", "1")
    reps = mnist_replicas("rnnprop", 9, 1)
    assert reps.xcd_supported()
    fx = reps.run(feed_of(reps, 5), form="xcd")
    assert fx.shape == (9,) and len(reps.fx_arrays) == 9
    assert reps.last_form == "xcd" and all(g.last_path == "mlp_xcd" for g in reps.graphs)
    assert [len(m["insts"]) for m in claiming.multis] == [8, 1]
    assert all(m["T"] == 1 and m["step0"] == 5 and m["hists"] is None for m in claiming.multis)
    sent = [i for m in claiming.multis for i in m["insts"]]
    assert [i["xs"][0].data_ptr() for i in sent] == [g.mlp_instance({g.step: 5})["xs"][0].data_ptr() for g in reps.graphs]
    assert len({i["xs"][0].data_ptr() for i in sent}) == 9 and all(m["d"] is sent[0]["desc"] for m in claiming.multis)
    assert claiming.asked and max(claiming.asked) <= 8
    for g in reps.graphs:                                    # the recovery snapshot, unless switched off
        assert ("_snap" in g.__dict__) == (not no_recovery)
        if not no_recovery:
            assert g._last_launch == {"restart": None, "snapshot": True, "commit": True}
            assert len(g._snap["bak"]) == len(g._snap["live"]) == 4 + 4 + 8


def test_launch_returns_the_instances_loss_buffers(claiming):
    reps = mnist_replicas("dm_logsign", 3, 2)
    out = reps.launch({})
    assert reps.last_form == "xcd" and all(g.last_path == "mlp_xcd" for g in reps.graphs)
    assert len(claiming.multis) == 1 and claiming.multis[0]["hists"] is None
    assert len(out) == 3 and all(a is i["fx"] for a, i in zip(out, claiming.multis[0]["insts"]))
    assert all(a is g._fx_cache[2]["bufs"][0] for a, g in zip(out, reps.graphs))
    assert all("_snap" not in g.__dict__ for g in reps.graphs)                     # (no recovery snapshot on this path)


def test_train_step_hands_one_history_per_instance(claiming):
    reps = mnist_replicas("rnnprop", 2, 1)
    reps.train_step(feed_of(reps, 1), 1e-3, form="xcd")     # (the stub writes no history: only the launch is looked at)
    assert reps.last_form == "xcd" and all(g.last_path == "mlp_xcd" for g in reps.graphs)
    assert len(claiming.multis) == 1
    launch = claiming.multis[0]
    assert len(launch["insts"]) == 2 and len(launch["hists"]) == 2 and launch["T"] == 1 and launch["step0"] == 1
    for g, inst, h in zip(reps.graphs, launch["insts"], launch["hists"]):
        assert h is g._mlp_record_plan["hist"] and inst["fx"] is g._fx_cache[1]["bufs"][0]
        assert set(h) == {"st", "g", "m", "v"} and all(len(h[k]) == 4 for k in h)


def test_disable_switch_and_two_data_sets(claiming, monkeypatch):
    reps = mnist_replicas("dm_logsign", 2, 2)
    assert reps.xcd_supported()
    monkeypatch.setenv("L2O_DISABLE_FUSED", "1")
    assert not reps.xcd_supported()
    with pytest.raises(_abi.L2OUnsupported):
        reps.run(form="xcd")
    monkeypatch.delenv("L2O_DISABLE_FUSED")
    # a replica over ANOTHER data set
    meta.set_random_seed(6)
    other = problems.synthetic_mnist(100, seed=23)
    extra = reps.optimizer._build_graph(problems.mnist(layers=(20,), batch_size=64, data=other), 2, None, False)
    extra.nets = reps.graphs[0].nets
    for s in extra.slots:
        s.net = reps.graphs[0].nets[s.key]
    reps.graphs.append(extra)
    reps.reset()
    with pytest.raises(ValueError, match=r"^Replicas.run: the replicas must be problems.mnist instances over ONE data set, "
                                         r"stepped by one \(20, 20\) LSTM network$"):
        reps.run(form="xcd")
    with pytest.raises(ValueError, match=r"^Replicas.train_step: the replicas must be problems.mnist instances over ONE data "
                                         r"set, stepped by one LSTM network, without second derivatives$"):
        reps.train_step({}, 1e-3, form="xcd")
    assert claiming.multis == []
