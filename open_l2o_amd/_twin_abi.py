"""ctypes binding of ``open_l2o_amd/csrc_twin/l2o_twin_abi.h``: libl2o_twin.so, the Twin-L2O minimax unroll.

A library and a prototype table of their own (``_abi.PROTOTYPES`` is the closed list of libl2o_hip.so).  As there, this is
the only way the Python host reaches the compute path: a missing or stale library is an error, never a fallback.
"""
from __future__ import annotations

import ctypes as C
import hashlib
import os

from ._abi import L2O_ERR_ARG, L2O_ERR_UNSUPPORTED, L2O_OK, L2OError, L2OUnsupported

_HERE = os.path.dirname(os.path.abspath(__file__))
# L2O_TWIN_LIB: an alternative build of the same library (timing ablations); its build id is not held to the tree's
LIB_PATH = os.environ.get("L2O_TWIN_LIB") or os.path.join(_HERE, "libl2o_twin.so")

MAX_HIDDEN, MAX_DIM = 96, 16
SADDLE, ROTATED_SADDLE, SEESAW, MATRIX_GAME = 1, 2, 3, 4


class TwinNet(C.Structure):
    """struct l2o_twin_net"""
    _fields_ = [("hidden", C.c_int32), ("n_in", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("w_ih1", "w_hh1", "b_ih1", "b_hh1", "w_ih2", "w_hh2", "b_ih2", "b_hh2",
                                          "w_out", "b_out")]


class TwinProblem(C.Structure):
    """struct l2o_twin_problem"""
    _fields_ = [("kind", C.c_int32), ("n_inst", C.c_int32), ("dim", C.c_int32), ("flags", C.c_int32), ("data", C.c_void_p)]


class TwinRun(C.Structure):
    """struct l2o_twin_run"""
    _fields_ = [("iter0", C.c_int32), ("n_iter", C.c_int32), ("n_sign", C.c_int32), ("rescale", C.c_float),
                ("out_mul", C.c_float), ("sign_lr", C.c_void_p)]


def _prototypes():
    P, vp = C.POINTER, C.c_void_p
    return {
        "l2o_twin_last_error": (C.c_char_p, []),
        "l2o_twin_build_id": (C.c_char_p, []),
        "l2o_twin_supported": (C.c_int, [P(TwinNet), P(TwinNet), P(TwinProblem)]),
        "l2o_twin_state_floats": (C.c_size_t, [P(TwinNet), C.c_int64]),
        "l2o_twin_unroll": (C.c_int, [P(TwinNet), P(TwinNet), P(TwinProblem), P(TwinRun), vp, vp, vp, vp, vp, vp, vp]),
    }


# every symbol l2o_twin_abi.h declares -> (restype, argtypes)
PROTOTYPES = _prototypes()

# what csrc_twin/Makefile hashes, in its order
_BUILD_ID_FILES = ("Makefile", "l2o_twin.h", "l2o_twin.hip", "l2o_twin_abi.h", "../csrc/l2o_common.h", "../csrc/l2o_host.h",
                   "../csrc/l2o_params.h", "../../include/l2o_abi.h")


def source_build_id():
    """What l2o_twin_build_id() of a library built from the sources in this tree returns, or None without the sources."""
    h = hashlib.sha256()
    try:
        for n in _BUILD_ID_FILES:
            with open(os.path.join(_HERE, "csrc_twin", n), "rb") as f:
                h.update(f.read())
    except OSError:
        return None
    return h.hexdigest()[:16]


_lib = None


def lib():
    """Load (once) and return libl2o_twin.so; refuse a missing one and a stale one (a symbol of PROTOTYPES it lacks, or a
    build id that is not the one of the sources in this tree)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("open_l2o_amd: %s is missing -- build it with `make -C open_l2o_amd/csrc_twin`.  There is no CPU "
                           "fallback." % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    missing = [name for name in PROTOTYPES if not hasattr(L, name)]
    if missing:
        raise RuntimeError("open_l2o_amd: %s has no %s: the library is stale -- rebuild it with `make -C "
                           "open_l2o_amd/csrc_twin`" % (LIB_PATH, ", ".join(missing)))
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    want, have = source_build_id(), L.l2o_twin_build_id().decode("ascii", "replace")
    if want is not None and have != want and not os.environ.get("L2O_TWIN_LIB"):
        raise RuntimeError("open_l2o_amd: %s was built from other sources (build id %s, this tree %s) -- rebuild it with "
                           "`make -C open_l2o_amd/csrc_twin`" % (LIB_PATH, have, want))
    _lib = L
    return L


_NET_FIELDS = (("w_ih1", "recurs.weight_ih"), ("w_hh1", "recurs.weight_hh"), ("b_ih1", "recurs.bias_ih"),
               ("b_hh1", "recurs.bias_hh"), ("w_ih2", "recurs2.weight_ih"), ("w_hh2", "recurs2.weight_hh"),
               ("b_ih2", "recurs2.bias_ih"), ("b_hh2", "recurs2.bias_hh"), ("w_out", "output.weight"), ("b_out", "output.bias"))


class Device(object):
    """Device copies of what a launch reads beside theta and the states -- the two networks ((hidden, n_in, {torch parameter
    name: array}) for min and max), the instance data (problem = (kind, n_inst, dim, data)) and the schedule (run: dict of
    iter0, n_iter, n_sign, rescale, out_mul, sign_lr) -- and the structs nets[0], nets[1], problem, run that point at them.
    `engine` supplies tensor(): a HipEngine."""

    def __init__(self, engine, nets, problem, run):
        self.keep, self.nets = [], []
        for hidden, n_in, params in nets:
            c = TwinNet()
            c.hidden, c.n_in = int(hidden), int(n_in)
            for field, name in _NET_FIELDS:
                t = engine.tensor(params[name])
                self.keep.append(t)
                setattr(c, field, t.data_ptr())
            self.nets.append(c)
        kind, n_inst, dim, data = problem
        data_d = engine.tensor(data)
        lr_d = engine.tensor(run["sign_lr"]) if len(run["sign_lr"]) else None
        self.keep += [data_d, lr_d]
        self.problem = TwinProblem(int(kind), int(n_inst), int(dim), 0, data_d.data_ptr())
        self.run = TwinRun(int(run["iter0"]), int(run["n_iter"]), int(run["n_sign"]), float(run["rescale"]),
                           float(run["out_mul"]), None if lr_d is None else lr_d.data_ptr())

    def unroll(self, theta, state_min, state_max, curve=None, fval=None, delta=None, stream=None):
        """l2o_twin_unroll on contiguous fp32 device tensors (None: NULL); returns its return code."""
        def ptr(t):
            if t is None:
                return None
            assert t.dtype.is_floating_point and t.element_size() == 4 and t.is_contiguous(), "C-ABI wants contiguous fp32"
            return C.c_void_p(t.data_ptr())
        return lib().l2o_twin_unroll(C.byref(self.nets[0]), C.byref(self.nets[1]), C.byref(self.problem), C.byref(self.run),
                                     ptr(theta), ptr(state_min), ptr(state_max), ptr(curve), ptr(fval), ptr(delta), stream)


def build_id():
    return lib().l2o_twin_build_id().decode("ascii", "replace")


def check(rc):
    """Turn a return code of libl2o_twin.so into the exception the host layer raises."""
    if rc == L2O_OK:
        return
    msg = lib().l2o_twin_last_error().decode("utf-8", "replace")
    if rc == L2O_ERR_UNSUPPORTED:
        raise L2OUnsupported(rc, msg)
    if rc == L2O_ERR_ARG:
        raise ValueError("libl2o_twin: " + msg)
    raise L2OError(rc, msg)
