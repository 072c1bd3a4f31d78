"""ctypes binding of the C ABI declared in the headers of ``include/``.

This is the ONLY way the Python host reaches the compute path: there is no
PyTorch / NumPy fallback.  If ``libl2o_hip.so`` is missing (not built) every
entry point raises ``RuntimeError`` -- the product path must fail loudly when
the HIP extension is absent.

Two tables carry everything that is per symbol: ``PROTOTYPES`` (header ->
symbol -> restype / argtypes; ``lib()`` declares exactly these and refuses a
library that lacks one) and ``STEP_FG`` (the (struct, stem) pair of every
step-path optimizee, from which their two prototypes each are made).
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# L2O_HIP_LIB: alternative build of the SAME library (timing ablations, scripts/ablate.sh)
LIB_PATH = os.environ.get("L2O_HIP_LIB") or os.path.join(_HERE, "libl2o_hip.so")

L2O_ABI_VERSION = 15
L2O_OK, L2O_ERR_ARG, L2O_ERR_UNSUPPORTED, L2O_ERR_HIP, L2O_ERR_TIMEOUT = 0, -1, -2, -3, -4

NET_CW, NET_RNNPROP = 0, 1
PRE_IDENTITY, PRE_LOGSIGN, PRE_FC_ELU = 0, 1, 2
PROB_SIMPLE, PROB_QUADRATIC, PROB_LASSO, PROB_RASTRIGIN, PROB_SQUARE_COS, PROB_MLP = 0, 1, 2, 3, 4, 5
PROB_MNIST_CONV = 6
PROB_CIFAR_CONV = 7
PROB_LENET = 8
PROB_CONFOCAL = 9
PROB_VGG16 = 10           # include/l2o_vgg16_abi.h (added after ABI v15)
PROB_NAS = 11             # include/l2o_nas_abi.h (added after ABI v15)

# option ids of include/l2o_abi.h ("options": per call, caller-owned -- the LIBRARY keeps no option state since ABI v9).
# This binding keeps the caller's side of it: one process-wide dict of non-default values (applied from the L2O_*
# environment variables once at import, changed by set_option) that NetSpec.to_c() / the problem and MLP descriptors
# encode into every struct they hand to the library.
# (id 8 was OPT_PAIR_NORMAL until ABI v11; since v13 it is OPT_MLP_XCD_WAVES)
OPT_PAIR, OPT_PAIR_PLAIN_STORES, OPT_UNROLL_CU, OPT_FG_TWO_PASS, OPT_MLP_GENERIC, OPT_BWD_BLOCKS, OPT_BWD_KERNEL, \
    OPT_MLP_UNROLL, OPT_MLP_XCD_WAVES, OPT_EXACT_GATES, OPT_WPACK_NO_CLEAR, OPT_MLP_HIER, OPT_ONE_LDS, \
    OPT_PAIR_FAST_LOAD = range(14)
OPT_DEFAULTS = {OPT_PAIR: 1, OPT_PAIR_PLAIN_STORES: 1, OPT_UNROLL_CU: 1, OPT_FG_TWO_PASS: 0, OPT_MLP_GENERIC: 0,
                OPT_BWD_BLOCKS: 0, OPT_BWD_KERNEL: 0, OPT_MLP_UNROLL: 1, OPT_MLP_XCD_WAVES: 0, OPT_EXACT_GATES: 0,
                OPT_WPACK_NO_CLEAR: 0, OPT_MLP_HIER: 1, OPT_ONE_LDS: 1, OPT_PAIR_FAST_LOAD: 1}
# l2o_last_unroll_form(): which kernel a fused launch ran (include/l2o_abi.h L2O_FORM_*)
FORM_NAMES = {1: "k_unroll", 2: "k_unroll_pair", 5: "k_unroll_lds", 6: "k_unroll_cu", 7: "k_unroll_cu8",
              8: "k_mlp_unroll (flat all-reduce)", 9: "k_mlp_unroll (XCD-hierarchical all-reduce)", 10: "k_mlp_unroll (generic loops)",
              11: "k_mlp_xcd (one optimizee instance per XCD)", 12: "k_cf_unroll (one workgroup per batch row)",
              13: "k_cf_unroll (several instances per launch: one workgroup per row of every instance)"}
FORMS_WITH_EXCHANGE = (2, 8, 9, 10, 11)    # workgroups wait for partner workgroups: can end in L2OPartnerTimeout
PROB_FG_TWO_PASS = 2      # l2o_problem.flags
MLP_GENERIC = 1           # l2o_mlp.flags
_options = {}
# The library never reads the environment; this binding applies two variables ONCE, when it is imported:
#   L2O_EXACT_GATES=1          the fmaf-chain-equal fp32 MFMA gate GEMM (an accuracy choice a user may want: DESIGN.md 4)
#                              It reaches the plain (non-recording) fused unroll on k_unroll (D <= 64) and k_unroll_pair, and
#                              routes 5..8-tile problems away from k_unroll_lds to those; k_unroll at 5..8 tiles is fp32 MFMA
#                              anyway.  It is accepted and IGNORED -- the gates stay bf16x3 -- by every recording launch, the
#                              streaming forms (k_unroll_cu / k_unroll_cu8: D > 128, or more rows than the resident forms
#                              hold) and l2o_mlp_unroll*: last_unroll_variant()["EXACT"] says what a launch ran.
#   L2O_OPTIONS=name=v,...     any option by name (pair, one_lds, unroll_cu, mlp_hier, ...): the A/B scripts' escape hatch.
# (Until round 5 every option had its own variable -- thirteen of them; tests and callers use set_option / option_scope.)
OPTION_NAMES = {"pair": OPT_PAIR, "pair_plain_stores": OPT_PAIR_PLAIN_STORES, "unroll_cu": OPT_UNROLL_CU,
                "fg_two_pass": OPT_FG_TWO_PASS, "mlp_generic": OPT_MLP_GENERIC, "bwd_blocks": OPT_BWD_BLOCKS,
                "bwd_kernel": OPT_BWD_KERNEL, "mlp_unroll": OPT_MLP_UNROLL, "exact_gates": OPT_EXACT_GATES,
                "mlp_hier": OPT_MLP_HIER, "one_lds": OPT_ONE_LDS, "mlp_xcd_waves": OPT_MLP_XCD_WAVES,
                "pair_fast_load": OPT_PAIR_FAST_LOAD}
if os.environ.get("L2O_EXACT_GATES"):
    _options[OPT_EXACT_GATES] = 1
for _item in filter(None, os.environ.get("L2O_OPTIONS", "").split(",")):
    _name, _, _val = _item.partition("=")
    if _name.strip() not in OPTION_NAMES:
        raise ValueError("L2O_OPTIONS: unknown option %r (known: %s)" % (_name, ", ".join(sorted(OPTION_NAMES))))
    _options[OPTION_NAMES[_name.strip()]] = int(_val)


def set_option(opt, value):
    """Change one kernel A/B switch for every later call of this process; returns the previous value."""
    if opt not in OPT_DEFAULTS:
        raise ValueError("unknown option %r" % (opt,))
    old = get_option(opt)
    value = int(value)
    if value == OPT_DEFAULTS[opt]:
        _options.pop(opt, None)
    else:
        if not 0 <= value <= (4095 if opt == OPT_BWD_BLOCKS else 7):
            raise ValueError("option %d: value %d out of range" % (opt, value))
        _options[opt] = value
    return old


class option_scope(object):
    """with option_scope({OPT_PAIR: 0}): ... -- the settings for the calls inside, restored afterwards."""

    def __init__(self, settings):
        self.settings = dict(settings)

    def __enter__(self):
        self.old = {o: set_option(o, v) for o, v in self.settings.items()}
        return self

    def __exit__(self, *exc):
        for o, v in self.old.items():
            set_option(o, v)
        return False


def get_option(opt):
    if opt not in OPT_DEFAULTS:
        return -1
    return _options.get(opt, OPT_DEFAULTS[opt])


def options_word():
    """l2o_net_cfg.options of the current settings: L2O_OPTW(o, v) words OR-ed together (0 = every default)."""
    w = 0
    for o, v in _options.items():
        if o == OPT_BWD_BLOCKS:
            w |= (v & 0xfff) << 48
        else:
            # (include/l2o_abi.h L2O_OPT_FIELD_: bits 48-59 are the BWD_BLOCKS count, option 12 uses that option's unused
            #  field, option 13 bits 60-63)
            w |= (8 | (v & 7)) << (4 * {OPT_ONE_LDS: OPT_BWD_BLOCKS, OPT_PAIR_FAST_LOAD: 15}.get(o, o))
    return w


class NetCfg(C.Structure):
    """struct l2o_net_cfg"""
    _fields_ = [
        ("kind", C.c_int32), ("preprocess", C.c_int32), ("n_layers", C.c_int32),
        ("hidden", C.c_int32), ("tanh_output", C.c_int32), ("reserved", C.c_int32),
        ("scale", C.c_double), ("logsign_k", C.c_double),
        ("beta1", C.c_double), ("beta2", C.c_double), ("options", C.c_uint64),
    ]


class Problem(C.Structure):
    """struct l2o_problem"""
    _fields_ = [
        ("kind", C.c_int32), ("B_local", C.c_int32), ("B_global", C.c_int32),
        ("D", C.c_int32), ("M", C.c_int32), ("flags", C.c_int32),
        ("l1", C.c_double), ("alpha", C.c_double),
        ("W", C.c_void_p), ("y", C.c_void_p), ("C", C.c_void_p), ("x_scale", C.c_void_p),
    ]


class Mlp(C.Structure):
    """struct l2o_mlp"""
    _fields_ = [
        ("n_in", C.c_int32), ("n_hidden", C.c_int32), ("n_out", C.c_int32), ("batch", C.c_int32),
        ("activation", C.c_int32), ("n_data", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32),
        ("images", C.c_void_p), ("labels", C.c_void_p),
    ]


class MlpHist(C.Structure):            # per variable (w1, b1, w2, b2) history of l2o_mlp_unroll_record
    """struct l2o_mlp_hist"""
    _fields_ = [("st", C.c_void_p * 4), ("g", C.c_void_p * 4), ("m", C.c_void_p * 4), ("v", C.c_void_p * 4)]


class MlpDeep(C.Structure):
    """struct l2o_mlp_deep"""
    _fields_ = [("n_in", C.c_int32), ("n_out", C.c_int32), ("batch", C.c_int32), ("activation", C.c_int32),
                ("n_data", C.c_int32), ("n_hidden_layers", C.c_int32), ("hidden", C.c_int32 * 3), ("reserved", C.c_int32),
                ("images", C.c_void_p), ("labels", C.c_void_p)]


class ImageNet(C.Structure):
    """What struct l2o_mnist_conv, l2o_cifar_conv and l2o_lenet all are: the header declares the same fields three times."""
    _fields_ = [("batch", C.c_int32), ("n_data", C.c_int32), ("batch_norm", C.c_int32), ("flags", C.c_int32),
                ("images", C.c_void_p), ("labels", C.c_void_p)]


class MnistConv(ImageNet):
    """struct l2o_mnist_conv"""


class CifarConv(ImageNet):
    """struct l2o_cifar_conv"""


class Lenet(ImageNet):
    """struct l2o_lenet"""


class Nas(ImageNet):
    """struct l2o_nas"""


class Confocal(C.Structure):
    """struct l2o_confocal"""
    _fields_ = [("batch", C.c_int32), ("num_points", C.c_int32), ("roi", C.c_int32 * 3), ("inference", C.c_int32),
                ("flags", C.c_int32), ("img", C.c_void_p)]


CONFOCAL_MAX_VARS = 49     # L2O_CONFOCAL_MAX_VARS: 6 * 8 points + 1


class ConfocalHist(C.Structure):       # per variable history of l2o_confocal_unroll_record
    """struct l2o_confocal_hist"""
    _fields_ = [("st", C.c_void_p * CONFOCAL_MAX_VARS), ("g", C.c_void_p * CONFOCAL_MAX_VARS),
                ("m", C.c_void_p * CONFOCAL_MAX_VARS), ("v", C.c_void_p * CONFOCAL_MAX_VARS)]


CONFOCAL_MAX_INSTANCES = 32     # L2O_CONFOCAL_MAX_INSTANCES


class ConfocalInstance(C.Structure):   # one replica of l2o_confocal_unroll_multi
    """struct l2o_confocal_instance"""
    _fields_ = [(n, C.c_void_p * CONFOCAL_MAX_VARS) for n in ("x", "st", "m", "v", "x_scale", "sim")] + \
               [("img", C.c_void_p), ("fx", C.c_void_p)]


class MlpInstance(C.Structure):        # one replica of l2o_mlp_unroll_multi
    """struct l2o_mlp_instance"""
    _fields_ = [("indices", C.c_void_p), ("x", C.c_void_p * 4), ("st", C.c_void_p * 4), ("m", C.c_void_p * 4),
                ("v", C.c_void_p * 4), ("x_scale", C.c_void_p * 4), ("fx", C.c_void_p)]


class Vgg16(C.Structure):
    """struct l2o_vgg16"""
    _fields_ = [("batch", C.c_int32), ("n_data", C.c_int32), ("flags", C.c_int32), ("channels", C.c_int32 * 5),
                ("images", C.c_void_p), ("labels", C.c_void_p)]


# the step-path optimizees: (descriptor struct, symbol stem), in the order of their problem kinds.  Every one exports
# <stem>_fg(const struct *, 6 pointers) -> int and <stem>_scratch_floats(const struct *) -> size_t: PROTOTYPES holds both per
# pair.  A new step-path optimizee appends its pair here and gives it a place in PROTOTYPES.
STEP_FG = ((MlpDeep, "l2o_mlp_deep"), (MnistConv, "l2o_mnist_conv"), (CifarConv, "l2o_cifar_conv"), (Lenet, "l2o_lenet"),
           (Confocal, "l2o_confocal"), (Vgg16, "l2o_vgg16"), (Nas, "l2o_nas"))


class GenNet(C.Structure):
    """struct l2o_gen_net"""
    _fields_ = [("n_layers", C.c_int32), ("hidden", C.c_int32 * 3), ("in_dim", C.c_int32), ("direct_inputs", C.c_int32),
                ("w_gates", C.c_void_p * 3), ("b_gates", C.c_void_p * 3), ("w_lin", C.c_void_p), ("b_lin", C.c_void_p),
                ("w_fc", C.c_void_p), ("b_fc", C.c_void_p)]


class GenBwdIO(C.Structure):
    """struct l2o_gen_bwd_io"""
    _fields_ = [(n, C.c_void_p) for n in ("g", "m", "v", "st_prev", "dx_next", "carry_in", "carry_out")] + \
               [("act", C.c_void_p * 3), ("dz", C.c_void_p * 3)] + \
               [(n, C.c_void_p) for n in ("tc", "h_last", "dd", "feats", "du", "dg")]


class KlstmNet(C.Structure):
    """struct l2o_klstm_net"""
    _fields_ = [("kw", C.c_int32), ("kh", C.c_int32), ("n_layers", C.c_int32), ("hidden", C.c_int32 * 2),
                ("preprocess", C.c_int32), ("tanh_output", C.c_int32), ("flags", C.c_int32), ("logsign_k", C.c_double),
                ("scale", C.c_double), ("w_gates", C.c_void_p * 2), ("b_gates", C.c_void_p * 2), ("w_lin", C.c_void_p),
                ("b_lin", C.c_void_p)]


class KlstmBwdIO(C.Structure):
    """struct l2o_klstm_bwd_io"""
    _fields_ = [(n, C.c_void_p) for n in ("g", "st_prev", "dx_next", "carry_in", "carry_out")] + \
               [("act", C.c_void_p * 2), ("dz", C.c_void_p * 2)] + [(n, C.c_void_p) for n in ("tc", "h_last", "dd")]


TWIN_MAX_HIDDEN, TWIN_MAX_DIM = 96, 16                                          # L2O_TWIN_MAX_* (include/l2o_twin_abi.h)
TWIN_SADDLE, TWIN_ROTATED_SADDLE, TWIN_SEESAW, TWIN_MATRIX_GAME = 1, 2, 3, 4    # l2o_twin_problem.kind


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


TWIN_TRAIN_MAX_ITER = 64                                                        # L2O_TWIN_TRAIN_MAX_ITER (include/l2o_twin_train_abi.h)


class TwinSegment(C.Structure):
    """struct l2o_twin_segment"""
    _fields_ = [("run", TwinRun), ("loss_scale", C.c_float), ("inst_weight", C.c_void_p)]


class TwinGrad(C.Structure):
    """struct l2o_twin_grad"""
    _fields_ = [(n, C.c_void_p) for n in ("w_ih1", "w_hh1", "b_ih1", "b_hh1", "w_ih2", "w_hh2", "b_ih2", "b_hh2",
                                          "w_out", "b_out")]


class NetWeights(C.Structure):
    """struct l2o_net_weights"""
    _fields_ = [(n, C.c_void_p) for n in ("w_gates1", "b_gates1", "w_gates2", "b_gates2", "w_lin", "b_lin",
                                          "w_fc", "b_fc", "wpack")]


class BwdIO(C.Structure):
    """struct l2o_bwd_io"""
    _fields_ = [(n, C.c_void_p) for n in ("g", "m", "v", "st_prev", "dx_next", "carry_in", "carry_out", "act1",
                                          "dz1", "act2", "dz2", "h2", "dd", "feats", "du")] + \
               [("a_stride", C.c_int64), ("b_stride", C.c_int64), ("dg", C.c_void_p)]


UNROLL_ZERO_STATE = 1     # l2o_unroll_reduce flags
PROB_W_SHARED = 1     # l2o_problem.flags: W is one [M, D] matrix for every problem


class StepSeg(C.Structure):
    """struct l2o_step_seg"""
    _fields_ = [("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("st", C.c_void_p), ("x", C.c_void_p),
                ("B", C.c_int64), ("D", C.c_int64), ("st_out", C.c_void_p), ("m_out", C.c_void_p), ("v_out", C.c_void_p)]


class BwdSeg(C.Structure):
    """struct l2o_bwd_seg"""
    _fields_ = [(n, C.c_void_p) for n in ("g", "m", "v", "st_prev", "dx_next")] + [("B", C.c_int64), ("D", C.c_int64)]


class BwdUnrollSeg(C.Structure):
    """struct l2o_bwd_unroll_seg"""
    _fields_ = [("B", C.c_int64), ("D", C.c_int64), ("g_final", C.c_void_p)]


class UnrollHist(C.Structure):
    """struct l2o_unroll_hist"""
    _fields_ = [(n, C.c_void_p) for n in ("st", "g", "m", "v", "g_final")]


def _step_fg(pairs):
    """The two prototypes of every (struct, stem) pair of STEP_FG in `pairs`, in the headers' order."""
    out = {}
    for struct, stem in pairs:
        out[stem + "_fg"] = (C.c_int, [C.POINTER(struct)] + [C.c_void_p] * 6)
        out[stem + "_scratch_floats"] = (C.c_size_t, [C.POINTER(struct)])
    return out


def _prototypes():
    P, vp, i32, i64, dbl, flt, I, Z = C.POINTER, C.c_void_p, C.c_int32, C.c_int64, C.c_double, C.c_float, C.c_int, C.c_size_t
    cfg, prob, mlp, conf = P(NetCfg), P(Problem), P(Mlp), P(Confocal)
    bwd_unroll = [cfg, P(NetWeights), P(BwdUnrollSeg), i32, vp, i32, i64, vp, vp, vp, vp, vp]
    twin = [P(TwinNet), P(TwinNet), P(TwinProblem)]
    return {
        "l2o_abi.h": {
            "l2o_abi_version": (I, []),
            "l2o_last_error": (C.c_char_p, []),
            "l2o_build_id": (C.c_char_p, []),
            "l2o_last_unroll_form": (I, []),
            "l2o_last_unroll_variant": (I, []),
            "l2o_coresident_workgroups": (i32, [vp, vp]),
            "l2o_wpack_floats": (Z, [cfg]),
            "l2o_wpack_host": (I, [cfg] + [vp] * 9),
            "l2o_state_floats": (Z, [i64, i64]),
            "l2o_state_pack": (I, [vp, vp, vp, vp, vp, i64, i64, vp]),
            "l2o_state_unpack": (I, [vp, vp, vp, vp, vp, i64, i64, vp]),
            "l2o_problem_fg": (I, [prob, vp, vp, vp, vp]),
            "l2o_problem_hvp": (I, [prob, vp, vp, vp, vp, vp]),
            "l2o_mlp_fg": (I, [mlp] + [vp] * 12),
            "l2o_mlp_scratch_floats": (Z, [mlp]),
            "l2o_mlp_unroll": (I, [cfg, vp, mlp, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp]),
            "l2o_mlp_unroll_record": (I, [cfg, vp, mlp, vp, vp, vp, vp, vp, vp, i32, i32, vp, P(MlpHist), vp, vp]),
            "l2o_mlp_unroll_supported": (I, [cfg, mlp, vp]),
            "l2o_mlp_unroll_workspace_bytes": (Z, [mlp]),
            "l2o_mlp_unroll_multi": (I, [cfg, vp, mlp, P(MlpInstance), i32, i32, i32, vp, vp]),
            "l2o_mlp_unroll_multi_record": (I, [cfg, vp, mlp, P(MlpInstance), i32, i32, i32, P(MlpHist), vp, vp]),
            "l2o_mlp_unroll_multi_supported": (I, [cfg, mlp, i32, vp]),
            "l2o_mlp_unroll_multi_workspace_bytes": (Z, [mlp, i32]),
            **_step_fg(STEP_FG[:5]),
            "l2o_cwlstm_step": (I, [cfg, vp, vp, vp, vp, dbl, dbl, vp, vp, i64, i64, vp]),
            "l2o_cwlstm_step_multi": (I, [cfg, vp, P(StepSeg), i32, dbl, dbl, vp]),
            "l2o_cwlstm_step_generic": (I, [cfg, P(GenNet), vp, vp, vp, vp, dbl, dbl, vp, vp, i64, vp]),
            "l2o_cwlstm_bwd_step_generic": (I, [cfg, P(GenNet), P(GenBwdIO), dbl, dbl, i64, vp]),
            "l2o_gen_state_floats": (Z, [P(GenNet), i64]),
            "l2o_cwlstm_bwd_step": (I, [cfg, P(NetWeights), P(BwdIO), dbl, dbl, i64, i64, vp]),
            "l2o_cwlstm_bwd_multi": (I, [cfg, P(NetWeights), P(BwdSeg), i32, vp, vp, vp, vp, dbl, dbl, vp]),
            "l2o_cwlstm_bwd_unroll": (I, bwd_unroll),
            "l2o_cwlstm_bwd_unroll_compact": (I, bwd_unroll),
            "l2o_cwlstm_wgrad_compact": (I, [cfg, vp, vp, i32, i64, vp, vp, vp]),
            "l2o_unroll": (I, [cfg, vp, prob, vp, vp, vp, vp, i32, i32, vp, vp, vp]),
            "l2o_unroll_record": (I, [cfg, vp, prob, vp, vp, vp, vp, i32, i32, vp, vp, P(UnrollHist), vp]),
            "l2o_unroll_reduce": (I, [cfg, vp, prob, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, P(UnrollHist), vp]),
            "l2o_unroll_workspace_init": (I, [vp, Z, vp]),
            "l2o_unroll_workspace_layout": (i64, [cfg, prob]),
            "l2o_cwlstm_wgrad": (I, [cfg, vp, vp, i64, vp, vp, vp]),
            "l2o_cwlstm_wgrad_dims": (i32, [cfg, P(i32), P(i32)]),
            "l2o_unroll_supported": (I, [cfg, prob]),
            "l2o_unroll_record_supported": (I, [cfg, prob]),
            "l2o_adam_step": (I, [vp, vp, vp, vp, i64, flt, dbl, dbl, dbl, vp]),
            "l2o_adam_step_guarded": (I, [vp, vp, vp, vp, i64, flt, dbl, dbl, dbl, vp, vp]),
            "l2o_adam_step_gather": (I, [vp, vp, vp, vp, vp, i64, flt, dbl, dbl, dbl, vp, vp]),
            "l2o_wpack_device": (I, [cfg, P(NetWeights), vp, vp]),
            "l2o_unroll_workspace_bytes": (Z, [cfg, prob, i32]),
            "l2o_unroll_status": (I, [vp]),
            "l2o_reduce_fx": (I, [vp, i32, i32, i32, vp, vp]),
            "l2o_atb": (I, [vp, vp, i64, i32, i32, vp, vp, vp]),
            "l2o_atb_workspace_bytes": (Z, [i64, i32, i32]),
            "l2o_suffix_sums": (I, [vp, vp, vp, i64, i32, vp]),
            "l2o_colsum": (I, [vp, i64, i64, i32, vp, i32, vp, vp]),
            "l2o_colsum_scratch_floats": (Z, [i64, i32]),
            "l2o_lincomb": (I, [vp, vp, flt, vp, flt, vp, flt, i64, vp]),
            "l2o_rnnprop_input_adjoint": (I, [vp, i64, i32, i32, vp, vp, vp, vp, dbl, dbl, dbl, dbl, vp, vp, vp, i64, vp]),
        },
        "l2o_confocal_unroll_abi.h": {       # the fused confocal unroll
            "l2o_confocal_unroll": (I, [cfg, vp, conf, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp]),
            "l2o_confocal_unroll_record": (I, [cfg, vp, conf, vp, vp, vp, vp, vp, vp, i32, i32, vp, P(ConfocalHist), vp, vp]),
            "l2o_confocal_unroll_supported": (I, [cfg, conf, vp]),
            "l2o_confocal_unroll_scratch_floats": (Z, [conf, i32]),
        },
        "l2o_confocal_multi_abi.h": {        # several confocal instances per fused launch
            "l2o_confocal_unroll_multi": (I, [cfg, vp, conf, P(ConfocalInstance), i32, i32, i32, vp, vp]),
            "l2o_confocal_unroll_multi_record": (I, [cfg, vp, conf, P(ConfocalInstance), i32, i32, i32, P(ConfocalHist), vp, vp]),
            "l2o_confocal_unroll_multi_supported": (I, [cfg, conf, i32, vp]),
            "l2o_confocal_unroll_multi_scratch_floats": (Z, [conf, i32, i32]),
        },
        "l2o_mlp_hvp_abi.h": {               # the Hessian-vector product of the MLP optimizee (second_derivatives=True)
            "l2o_mlp_hvp": (I, [P(MlpDeep)] + [vp] * 6),
            "l2o_mlp_hvp_scratch_floats": (Z, [P(MlpDeep)]),
        },
        "l2o_vgg16_abi.h": _step_fg(STEP_FG[5:6]),           # problems.vgg16_cifar10
        "l2o_nas_abi.h": _step_fg(STEP_FG[6:7]),             # problems.NAS
        "l2o_klstm_abi.h": {                 # networks.KernelDeepLSTM
            "l2o_klstm_supported": (I, [P(KlstmNet)]),
            "l2o_klstm_state_floats": (Z, [P(KlstmNet), i64]),
            "l2o_klstm_step": (I, [P(KlstmNet), vp, vp, vp, vp, i64, vp]),
            "l2o_klstm_bwd_step": (I, [P(KlstmNet), P(KlstmBwdIO), i64, vp]),
        },
        "l2o_twin_abi.h": {                  # twin.unroll: the Twin-L2O minimax evaluation unroll
            "l2o_twin_supported": (I, twin),
            "l2o_twin_state_floats": (Z, [P(TwinNet), i64]),
            "l2o_twin_unroll": (I, twin + [P(TwinRun)] + [vp] * 7),
        },
        "l2o_twin_train_abi.h": {            # twin.meta_gradient: one segment of the Twin-L2O meta-training
            "l2o_twin_train_floats": (Z, twin + [i32]),
            "l2o_twin_train_forward": (I, twin + [P(TwinSegment)] + [vp] * 8),
            "l2o_twin_train_backward": (I, twin + [P(TwinSegment), vp, P(TwinGrad), P(TwinGrad), vp]),
        },
    }


# THE prototype table: header of include/ -> {symbol: (restype, argtypes)}, every symbol the header declares, in this
# binding's order.  declare() gives a loaded library exactly these prototypes and refuses one that lacks any of them
# (tests/test_abi_headers_cpu.py holds the table, the structs and the constants above to the headers' text).
PROTOTYPES = _prototypes()


class L2OError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libl2o_hip error %d: %s" % (code, msg))
        self.code = code


class L2OUnsupported(L2OError):
    """L2O_ERR_UNSUPPORTED: no fused kernel for this configuration."""


class L2OPartnerTimeout(L2OError):
    """L2O_ERR_TIMEOUT (l2o_unroll_status): a workgroup of a kernel that exchanges data with partner workgroups gave up
    waiting -- that launch's outputs are invalid.  Recoverable: the host re-runs the unroll on an exchange-free form."""


def source_build_id():
    """What l2o_build_id() of a library built from the sources in this tree returns (csrc/Makefile: sha256 over the .hip
    translation units, every header of csrc/ and include/ and the Makefile in make's $(sort) order), or None without the
    sources."""
    import glob
    import hashlib
    csrc = os.path.join(_HERE, "csrc")
    names = ["Makefile"] + \
        [os.path.basename(p) for ext in ("*.hip", "*.h") for p in glob.glob(os.path.join(csrc, ext))] + \
        ["../../include/" + os.path.basename(p) for p in glob.glob(os.path.join(csrc, "../../include/*.h"))]
    h = hashlib.sha256()
    try:
        for n in sorted(names):
            with open(os.path.join(csrc, n), "rb") as f:
                h.update(f.read())
    except OSError:
        return None
    return h.hexdigest()[:16]


_lib = None


def build_id():
    """l2o_build_id() of the loaded library (16 hex digits)."""
    return lib().l2o_build_id().decode("ascii", "replace")


def last_unroll_form():
    """(name, dispatches) of the kernel the last fused unroll call of this thread launched, or (None, 0)."""
    w = int(lib().l2o_last_unroll_form())
    return FORM_NAMES.get(w & 0xff), w >> 8


def last_unroll_variant():
    """The template arguments of the kernel the last l2o_unroll* call of this thread launched (l2o_last_unroll_variant:
    include/l2o_abi.h L2O_VARIANT_*), as a dict; an argument that template does not have is 0.  EXACT is what ran, not
    what OPT_EXACT_GATES asked for."""
    w = int(lib().l2o_last_unroll_variant())
    return {"CH": w & 0xf, "HIST": (w >> 4) & 1, "EXACT": (w >> 5) & 1, "FAST": (w >> 6) & 1, "KR": (w >> 8) & 7,
            "NV": (w >> 12) & 3}


def declare(library):
    """Give every symbol of PROTOTYPES its restype / argtypes on the loaded `library` and return it.  The library is built
    from this tree, so one that lacks a listed symbol is a stale file: it is refused whole, at load."""
    missing = [name for protos in PROTOTYPES.values() for name in protos if not hasattr(library, name)]
    if missing:
        raise RuntimeError("open_l2o_amd: %s has no %s: the library is stale (built from older sources) -- rebuild it with "
                           "`make -C open_l2o_amd/csrc`" % (LIB_PATH, ", ".join(missing)))
    for protos in PROTOTYPES.values():
        for name, (restype, argtypes) in protos.items():
            fn = getattr(library, name)
            fn.restype, fn.argtypes = restype, argtypes
    return library


def lib():
    """Load (once) and return the C-ABI library; raise loudly if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "open_l2o_amd: %s is missing -- build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` or `make -C open_l2o_amd/csrc`.  There is no CPU fallback." % LIB_PATH)
    L = declare(C.CDLL(LIB_PATH))
    if L.l2o_abi_version() != L2O_ABI_VERSION:
        raise RuntimeError("libl2o_hip.so ABI version %d != binding version %d"
                           % (L.l2o_abi_version(), L2O_ABI_VERSION))
    _lib = L
    return L


def check(rc):
    """Turn a C-ABI return code into the Python exception the host layer raises."""
    if rc == L2O_OK:
        return
    msg = lib().l2o_last_error().decode("utf-8", "replace")
    if rc == L2O_ERR_UNSUPPORTED:
        raise L2OUnsupported(rc, msg)
    if rc == L2O_ERR_TIMEOUT:
        raise L2OPartnerTimeout(rc, msg)
    if rc == L2O_ERR_ARG:
        raise ValueError("libl2o_hip: " + msg)
    raise L2OError(rc, msg)
