"""The whole ctypes binding, open_l2o_amd/_abi.py, held to the text of the headers of include/: every function's restype and
argtypes in _abi.PROTOTYPES, every struct's fields, every integer constant; the counts, sizes and the order of l2o_abi.h's
symbols pinned as literals; the prototypes on the loaded library; the refusal of a stale library.  A new header adds its
rows to FUNCTIONS and SIZEOF here and nothing else."""
import ctypes as C
import hashlib
import os
import re

import pytest

import __graft_entry__
from open_l2o_amd import _abi, _engine, networks

INCLUDE = os.path.join(__graft_entry__.ROOT, "include")

# header -> functions it declares
FUNCTIONS = {"l2o_abi.h": 66, "l2o_confocal_unroll_abi.h": 4, "l2o_confocal_multi_abi.h": 4, "l2o_mlp_hvp_abi.h": 2,
             "l2o_vgg16_abi.h": 2, "l2o_nas_abi.h": 2, "l2o_klstm_abi.h": 4, "l2o_twin_abi.h": 3, "l2o_twin_train_abi.h": 3}
# struct -> sizeof
SIZEOF = {"l2o_net_cfg": 64, "l2o_problem": 72, "l2o_mlp": 48, "l2o_mlp_hist": 128, "l2o_mlp_deep": 56, "l2o_mnist_conv": 32,
          "l2o_cifar_conv": 32, "l2o_lenet": 32, "l2o_nas": 32, "l2o_confocal": 40, "l2o_confocal_hist": 1568,
          "l2o_confocal_instance": 2368, "l2o_mlp_instance": 176, "l2o_vgg16": 48, "l2o_gen_net": 104, "l2o_gen_bwd_io": 152,
          "l2o_klstm_net": 96, "l2o_klstm_bwd_io": 96, "l2o_twin_net": 88, "l2o_twin_problem": 24, "l2o_twin_run": 32,
          "l2o_twin_segment": 48, "l2o_twin_grad": 80, "l2o_net_weights": 72, "l2o_bwd_io": 144, "l2o_step_seg": 80,
          "l2o_bwd_seg": 56, "l2o_bwd_unroll_seg": 24, "l2o_unroll_hist": 40}
# #define L2O_<name> <integer> without an _abi.<name>: test_constants_without_a_namesake covers each by name
NO_NAMESAKE = ["ABI_VERSION", "OK", "ERR_ARG", "ERR_HIP", "ERR_TIMEOUT", "ERR_UNSUPPORTED", "OPT_COUNT_", "VGG16_VARS",
               "KLSTM_MAX_HIDDEN", "KLSTM_MAX_LAYERS", "KLSTM_MAX_SIDE", "FORM_UNROLL", "FORM_UNROLL_PAIR", "FORM_UNROLL_LDS",
               "FORM_UNROLL_CU", "FORM_UNROLL_CU8", "FORM_MLP_UNROLL", "FORM_MLP_UNROLL_HIER", "FORM_MLP_UNROLL_GENERIC",
               "FORM_MLP_XCD", "FORM_CONFOCAL_UNROLL", "FORM_CONFOCAL_MULTI"]
# functions whose pointers to scalars are bound as POINTER(scalar), not c_void_p
TYPED_SCALAR_POINTERS = ("l2o_cwlstm_wgrad_dims",)

SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "size_t": C.c_size_t,
           "float": C.c_float, "double": C.c_double}
# C struct name -> its class: the classes of _abi whose docstring is "struct <c name>"
CLASSES = {cls.__doc__[7:]: cls for cls in vars(_abi).values()
           if isinstance(cls, type) and issubclass(cls, C.Structure) and re.fullmatch(r"struct \w+", cls.__doc__ or "")}


def _text(header):
    with open(os.path.join(INCLUDE, header)) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


HEADERS = sorted(os.listdir(INCLUDE))
TEXT = {h: _text(h) for h in HEADERS}
DEFINES = [(name, int(v)) for h in HEADERS
           for name, v in re.findall(r"^#define L2O_(\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", TEXT[h], flags=re.M)]
STRUCTS = [(name, body) for h in HEADERS for name, body in re.findall(r"typedef struct (\w+) \{(.*?)\} \1;", TEXT[h], flags=re.S)]


def c_type(decl, returns=False, typed=False):
    """The ctypes type of a C return type or parameter."""
    tokens = re.findall(r"\w+|\*", re.sub(r"\bconst\b", "", decl))
    base, stars = tokens[0], tokens.count("*")
    if not stars:
        return SCALARS[base]
    if stars == 1 and base in CLASSES:
        return C.POINTER(CLASSES[base])
    if stars == 1 and returns and base == "char":
        return C.c_char_p
    if stars == 1 and typed and base in SCALARS:
        return C.POINTER(SCALARS[base])
    return C.c_void_p


def fields_of(body):
    """The _fields_ of a struct body: `type a, *b, c[N];` declarations, N a number or a #define of any header."""
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        base, rest = re.fullmatch(r"(?:const\s+)?(\w+)\b(.*)", decl, flags=re.S).groups()
        for item in rest.split(","):
            stars, name, length = re.fullmatch(r"\s*(\**)\s*(\w+)\s*(?:\[(\w+)\])?\s*", item).groups()
            t = C.c_void_p if stars else SCALARS.get(base) or CLASSES[base]
            if length:
                t = t * (int(length) if length.isdigit() else dict(DEFINES)[length[len("L2O_"):]])
            fields.append((name, t))
    return fields


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_abi.LIB_PATH):
        __graft_entry__.build()
    return _abi.lib()


# -- keys and counts ---------------------------------------------------------------------------------------------------
def test_keys_and_counts():
    assert sorted(_abi.PROTOTYPES) == HEADERS
    assert {h: len(protos) for h, protos in _abi.PROTOTYPES.items()} == FUNCTIONS
    names = [name for protos in _abi.PROTOTYPES.values() for name in protos]
    assert len(names) == len(set(names)) == 90                                    # (no symbol under two headers)
    # l2o_abi.h's list and its order, as before the table existed (sha256 of the names joined by blanks)
    first = tuple(_abi.PROTOTYPES["l2o_abi.h"])
    assert hashlib.sha256(" ".join(first).encode()).hexdigest()[:16] == "9551088b6b88e711"
    assert first[23:33] == (
        "l2o_mlp_deep_fg", "l2o_mlp_deep_scratch_floats", "l2o_mnist_conv_fg", "l2o_mnist_conv_scratch_floats",
        "l2o_cifar_conv_fg", "l2o_cifar_conv_scratch_floats", "l2o_lenet_fg", "l2o_lenet_scratch_floats",
        "l2o_confocal_fg", "l2o_confocal_scratch_floats")


# -- functions ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("header", HEADERS)
def test_functions(header):
    parsed = {}
    for ret, name, params in re.findall(r"((?:const\s+)?\w+\s*\*?)\s*\b(l2o_\w+)\s*\(([^()]*)\)\s*;", TEXT[header]):
        params = [] if params.strip() == "void" else params.split(",")
        parsed[name] = (c_type(ret, returns=True), [c_type(p, typed=name in TYPED_SCALAR_POINTERS) for p in params])
    assert set(parsed) == set(re.findall(r"\b(l2o_\w+)\s*\(", TEXT[header])) == set(_abi.PROTOTYPES[header])
    for name, proto in _abi.PROTOTYPES[header].items():
        assert parsed[name] == proto, name


def test_step_fg_prototypes():
    table = {name: proto for protos in _abi.PROTOTYPES.values() for name, proto in protos.items()}
    for struct, stem in _abi.STEP_FG:
        assert table[stem + "_fg"] == (C.c_int, [C.POINTER(struct)] + [C.c_void_p] * 6)
        assert table[stem + "_scratch_floats"] == (C.c_size_t, [C.POINTER(struct)])
    assert [stem for _, stem in _abi.STEP_FG] == ["l2o_mlp_deep", "l2o_mnist_conv", "l2o_cifar_conv", "l2o_lenet",
                                                  "l2o_confocal", "l2o_vgg16", "l2o_nas"]


# -- the loaded library ------------------------------------------------------------------------------------------------
def test_loaded_library_carries_the_table(lib):
    for protos in _abi.PROTOTYPES.values():
        for name, (restype, argtypes) in protos.items():
            assert getattr(lib, name).restype is restype and getattr(lib, name).argtypes == argtypes, name
            assert restype in (C.c_int, C.c_int32, C.c_int64, C.c_size_t, C.c_char_p) and type(argtypes) is list, name
            if name.endswith(("_floats", "_bytes")):
                assert restype is C.c_size_t, name                                # (ctypes' default int would truncate it)
    assert lib.l2o_abi_version() == 15 and _abi.source_build_id() == _abi.build_id()


class _Without(object):
    """Stands in for a loaded library that exports every listed symbol but `missing`."""

    def __init__(self, *missing):
        for protos in _abi.PROTOTYPES.values():
            for name in protos:
                if name not in missing:
                    setattr(self, name, type("fn", (), {})())


def test_a_library_that_lacks_a_listed_symbol_is_refused_at_load():
    whole = _Without()
    assert _abi.declare(whole) is whole
    assert whole.l2o_nas_scratch_floats.restype is C.c_size_t and whole.l2o_klstm_step.argtypes[0] is C.POINTER(_abi.KlstmNet)
    for missing in (("l2o_klstm_bwd_step",), ("l2o_abi_version",), ("l2o_confocal_unroll_multi", "l2o_vgg16_fg"),
                    ("l2o_twin_train_forward",)):
        stale = _Without(*missing)
        with pytest.raises(RuntimeError) as ei:
            _abi.declare(stale)
        assert str(ei.value) == ("open_l2o_amd: %s has no %s: the library is stale (built from older sources) -- rebuild it "
                                 "with `make -C open_l2o_amd/csrc`" % (_abi.LIB_PATH, ", ".join(missing)))
        assert not hasattr(stale.l2o_build_id, "restype")                         # (refused whole: nothing was declared)


# -- structs -----------------------------------------------------------------------------------------------------------
def test_every_header_struct_has_its_class():
    names = [name for name, _ in STRUCTS]
    assert len(names) == len(set(names)) == 29 and set(names) == set(CLASSES) == set(SIZEOF)


@pytest.mark.parametrize("name,body", STRUCTS, ids=[name for name, _ in STRUCTS])
def test_struct(name, body):
    cls = CLASSES[name]
    assert fields_of(body) == cls._fields_
    assert C.sizeof(cls) == SIZEOF[name]


# -- constants ---------------------------------------------------------------------------------------------------------
def test_constants_with_a_namesake():
    defines = dict(DEFINES)
    assert len(defines) == len(DEFINES)                                           # (no name defined twice)
    assert sorted(n for n in defines if not hasattr(_abi, n)) == sorted(NO_NAMESAKE)
    for name, value in defines.items():
        assert name in NO_NAMESAKE or getattr(_abi, name) == value, name
    assert len(defines) - len(NO_NAMESAKE) == 44
    assert {n: v for n, v in DEFINES if n.startswith("TWIN_")} == {
        "TWIN_MAX_HIDDEN": 96, "TWIN_MAX_DIM": 16, "TWIN_SADDLE": 1, "TWIN_ROTATED_SADDLE": 2, "TWIN_SEESAW": 3,
        "TWIN_MATRIX_GAME": 4, "TWIN_TRAIN_MAX_ITER": 64}


def test_constants_without_a_namesake():
    defines = dict(DEFINES)
    assert defines["ABI_VERSION"] == _abi.L2O_ABI_VERSION == 15
    codes = ("OK", "ERR_ARG", "ERR_UNSUPPORTED", "ERR_HIP", "ERR_TIMEOUT")
    assert [defines[n] for n in codes] == [getattr(_abi, "L2O_" + n) for n in codes] == [0, -1, -2, -3, -4]
    forms = [v for n, v in DEFINES if n.startswith("FORM_")]
    assert len(forms) == 11 and sorted(forms) == sorted(_abi.FORM_NAMES)
    assert defines["OPT_COUNT_"] == len(_abi.OPT_DEFAULTS) and sorted(_abi.OPT_DEFAULTS) == list(range(defines["OPT_COUNT_"]))
    assert defines["VGG16_VARS"] == _engine.STEP_OPTIMIZEES[_abi.PROB_VGG16].nvars(None)
    K = networks.KernelDeepLSTM
    assert (defines["KLSTM_MAX_SIDE"], defines["KLSTM_MAX_LAYERS"], defines["KLSTM_MAX_HIDDEN"]) == \
        (K.MAX_SIDE, K.MAX_LAYERS, K.MAX_HIDDEN)
