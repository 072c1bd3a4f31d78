"""Learning 2 Learn problems -- the optimizee registry of the reference
(``DM/problems.py``, DM = /root/reference/Model_Free_L2O/"L2O-DM and L2O-RNNProp"/),
session-less.

Same module-level factories, same argument names and defaults.  Each factory
returns a zero-argument ``build`` object, exactly like the reference returns a
``build`` closure; calling it declares the problem's variables through
:func:`get_variable` (the analogue of ``tf.get_variable``, which is what
``meta._get_variables`` intercepts at DM/meta.py:102-128) and returns a
:class:`Loss` description.  The arithmetic itself -- forward value and gradient
(DM/meta.py:322, 344) -- is done by the HIP kernels selected through ``Loss.terms``
(``l2o_problem_fg`` / ``l2o_unroll``); nothing here computes on the CPU.

Extensions over the reference (all optional, defaults unchanged):
  * ``lasso(..., num_rows=None)``  rectangular per-problem A like ``lasso_fixed``;
  * ``quadratic/lasso/rastrigin(..., data=dict)``  inject W/y/x0 arrays (parity tests).
"""
from __future__ import annotations

import collections
import sys

import numpy as np

from . import _abi

# ---------------------------------------------------------------------------
# variable declaration plumbing (tf.get_variable analogue)
# ---------------------------------------------------------------------------
VarDecl = collections.namedtuple("VarDecl", "name shape initializer trainable")
# one analytic loss term: kind (an _abi.PROB_* id), the trainable variable it is a
# function of, its constants by role, hyper-parameters and an ensemble weight
Term = collections.namedtuple("Term", "kind var consts hyper weight")
Loss = collections.namedtuple("Loss", "variables terms")

_scope = []          # variable_scope stack (ensemble uses "problem_i")
_decls = None        # active collection list while a build() runs


def _full_name(name):
    return "/".join(_scope + [name])


class _SharedVarDecl(VarDecl):
    """A constant with ONE copy for the whole batch (leading dimension 1; never batch-sharded)."""
    __slots__ = ()
    shared = True


def get_variable(name, shape, dtype="float32", initializer=None, trainable=True, shared=False):
    """Declare an optimizee variable (the reference calls ``tf.get_variable`` here;
    DM/meta.py:88-155 relies on that to harvest / substitute variables)."""
    if dtype not in ("float32", np.float32):
        raise ValueError("only float32 optimizees are implemented (got %r)" % (dtype,))
    cls = _SharedVarDecl if shared else VarDecl
    decl = cls(_full_name(name), tuple(int(s) for s in shape), initializer, bool(trainable))
    if _decls is not None:
        _decls.append(decl)
    return decl


# initializer descriptors (resolved on the device by meta.Variable)
def random_normal_initializer(mean=0.0, stddev=1.0):
    return ("normal", float(mean), float(stddev))


def random_uniform_initializer(minval=0.0, maxval=1.0):
    return ("uniform", float(minval), float(maxval))


def ones_initializer():
    return ("ones",)


def zeros_initializer():
    return ("zeros",)


def constant_initializer(value):
    return ("constant", np.asarray(value, dtype=np.float32))


class _Build(object):
    """Callable returned by the factories (the reference returns the closure ``build``)."""

    def __init__(self, name, fn):
        self.__name__ = name
        self._fn = fn

    def __call__(self):
        global _decls
        outer = _decls
        _decls = []
        try:
            terms = self._fn()
            variables = _decls
        finally:
            _decls = outer
        if outer is not None:          # nested (ensemble): hand declarations to the parent
            outer.extend(variables)
        return Loss(variables, terms)


def _maybe_const(data, key, shape, default):
    if data is not None and key in data:
        arr = np.asarray(data[key], dtype=np.float32).reshape(shape)
        return constant_initializer(arr)
    return default


# ---------------------------------------------------------------------------
# the registry (names, arguments and defaults of DM/problems.py)
# ---------------------------------------------------------------------------
def simple():
    """Simple problem: f(x) = x^2.  DM/problems.py:41-53."""

    def build():
        x = get_variable("x", shape=[], initializer=ones_initializer())
        return [Term(_abi.PROB_SIMPLE, x, {}, {}, 1.0)]

    return _Build("simple", build)


def simple_multi_optimizer(num_dims=2):
    """Multidimensional simple problem.  DM/problems.py:56-70."""

    def build():
        coords = [get_variable("x_{}".format(i), shape=[], initializer=ones_initializer())
                  for i in range(num_dims)]
        return [Term(_abi.PROB_SIMPLE, c, {}, {}, 1.0) for c in coords]

    return _Build("simple_multi_optimizer", build)


def quadratic(batch_size=128, num_dims=10, stddev=0.01, dtype="float32", data=None):
    """Quadratic problem: f(x) = ||Wx - y||.  DM/problems.py:73-101."""

    def build():
        x = get_variable("x", shape=[batch_size, num_dims], dtype=dtype,
                         initializer=_maybe_const(data, "x", [batch_size, num_dims],
                                                  random_normal_initializer(stddev=stddev)))
        w = get_variable("w", shape=[batch_size, num_dims, num_dims], dtype=dtype,
                         initializer=_maybe_const(data, "w", [batch_size, num_dims, num_dims],
                                                  random_uniform_initializer()), trainable=False)
        y = get_variable("y", shape=[batch_size, num_dims], dtype=dtype,
                         initializer=_maybe_const(data, "y", [batch_size, num_dims],
                                                  random_uniform_initializer()), trainable=False)
        return [Term(_abi.PROB_QUADRATIC, x, {"W": w, "y": y}, {}, 1.0)]

    return _Build("quadratic", build)


def lasso(batch_size=128, num_dims=10, stddev=0.01, l=0.005, dtype="float32", num_rows=None, data=None):
    """lasso problem: f(x) = 0.5*||Wx - y||2 + lamada *||x||1.  DM/problems.py:103-134."""
    rows = num_dims if num_rows is None else int(num_rows)

    def build():
        x = get_variable("x", shape=[batch_size, num_dims], dtype=dtype,
                         initializer=_maybe_const(data, "x", [batch_size, num_dims],
                                                  random_normal_initializer(stddev=stddev)))
        w = get_variable("w", shape=[batch_size, rows, num_dims], dtype=dtype,
                         initializer=_maybe_const(data, "w", [batch_size, rows, num_dims],
                                                  random_uniform_initializer()), trainable=False)
        y = get_variable("y", shape=[batch_size, rows, 1], dtype=dtype,
                         initializer=_maybe_const(data, "y", [batch_size, rows, 1],
                                                  random_uniform_initializer()), trainable=False)
        return [Term(_abi.PROB_LASSO, x, {"W": w, "y": y}, {"l1": float(l)}, 1.0)]

    return _Build("lasso", build)


def lasso_fixed(data_A, data_b, stddev=0.01, l=0.005, dtype="float32"):
    """lasso problem on given data A [B,M,N], b [B,M,1].  DM/problems.py:137-175.
    A 2-D ``data_A`` [M,N] is ONE sensing matrix shared by all B problems (the
    kernels then read it with batch stride 0 -- 512 KiB instead of 128 MiB for config 3)."""
    a = np.asarray(data_A, dtype=np.float32)
    b = np.asarray(data_b, dtype=np.float32)
    shared = a.ndim == 2
    if shared:
        a = a[None]
    if a.ndim != 3 or b.ndim != 3 or b.shape[1] != a.shape[1] or (not shared and b.shape[0] != a.shape[0]):
        raise ValueError("lasso_fixed expects data_A [B,M,N] (or one shared [M,N]) and data_b [B,M,1]")

    def build():
        x = get_variable("x", shape=[b.shape[0], a.shape[2]], dtype=dtype,
                         initializer=random_normal_initializer(stddev=stddev))
        w = get_variable("w", shape=a.shape, dtype=dtype, initializer=constant_initializer(a),
                         trainable=False, shared=shared)
        y = get_variable("y", shape=b.shape, dtype=dtype, initializer=constant_initializer(b),
                         trainable=False)
        return [Term(_abi.PROB_LASSO, x, {"W": w, "y": y}, {"l1": float(l)}, 1.0)]

    return _Build("lasso_fixed", build)


def rastrigin(batch_size=128, num_dims=10, alpha=10, stddev=1, dtype="float32", data=None):
    """Rastrigin-like problem.  DM/problems.py:177-213."""

    def build():
        x = get_variable("x", shape=[batch_size, num_dims, 1], dtype=dtype,
                         initializer=_maybe_const(data, "x", [batch_size, num_dims, 1],
                                                  random_normal_initializer(stddev=stddev)))
        A = get_variable("A", shape=[batch_size, num_dims, num_dims], dtype=dtype,
                         initializer=_maybe_const(data, "A", [batch_size, num_dims, num_dims],
                                                  random_normal_initializer(stddev=stddev)), trainable=False)
        B = get_variable("B", shape=[batch_size, num_dims, 1], dtype=dtype,
                         initializer=_maybe_const(data, "B", [batch_size, num_dims, 1],
                                                  random_normal_initializer(stddev=stddev)), trainable=False)
        C = get_variable("C", shape=[batch_size, num_dims, 1], dtype=dtype,
                         initializer=_maybe_const(data, "C", [batch_size, num_dims, 1],
                                                  random_normal_initializer(stddev=stddev)), trainable=False)
        return [Term(_abi.PROB_RASTRIGIN, x, {"W": A, "y": B, "C": C}, {"alpha": float(alpha)}, 1.0)]

    return _Build("rastrigin", build)


def square_cos(batch_size=128, num_dims=10, stddev=0.01, dtype="float32", data=None):
    """f = mean_b [ ||w x - y||^2 - sum_i (wcos (10 cos(2*3.1415926 x)))_i + 10 D ].  DM/problems.py:959-994."""

    def build():
        x = get_variable("x", shape=[batch_size, num_dims], dtype=dtype,
                         initializer=_maybe_const(data, "x", [batch_size, num_dims],
                                                  random_normal_initializer(stddev=stddev)))
        w = get_variable("w", shape=[batch_size, num_dims, num_dims], dtype=dtype,
                         initializer=_maybe_const(data, "w", [batch_size, num_dims, num_dims],
                                                  random_uniform_initializer()), trainable=False)
        y = get_variable("y", shape=[batch_size, num_dims], dtype=dtype,
                         initializer=_maybe_const(data, "y", [batch_size, num_dims],
                                                  random_uniform_initializer()), trainable=False)
        wcos = get_variable("wcos", shape=[batch_size, num_dims, num_dims], dtype=dtype,
                            initializer=_maybe_const(data, "wcos", [batch_size, num_dims, num_dims],
                                                     random_uniform_initializer()), trainable=False)
        return [Term(_abi.PROB_SQUARE_COS, x, {"W": w, "y": y, "wcos": wcos}, {}, 1.0)]

    return _Build("square_cos", build)


def ensemble(problems, weights=None):
    """Ensemble of problems: sum of (weighted) losses.  DM/problems.py:215-245."""
    if weights and len(weights) != len(problems):
        raise ValueError("len(weights) != len(problems)")
    build_fns = [getattr(sys.modules[__name__], p["name"])(**p["options"]) for p in problems]

    def build():
        terms = []
        for i, build_fn in enumerate(build_fns):
            _scope.append("problem_{}".format(i))
            try:
                sub = build_fn()
            finally:
                _scope.pop()
            for t in sub.terms:
                terms.append(t._replace(weight=t.weight * (weights[i] if weights else 1.0)))
        return terms

    return _Build("ensemble", build)


_nn_initializers = {                                # DM/problems.py:35-38
    "w": random_normal_initializer(mean=0, stddev=0.01),
    "b": random_normal_initializer(mean=0, stddev=0.01),
}


def synthetic_mnist(num_examples=2048, seed=0, label_noise=0.0):
    """A deterministic stand-in for the MNIST arrays (no dataset ships with this repo and
    there is no network): images [N,28,28,1] in [0,1], labels [N] in 0..9.
    ``label_noise``: that fraction of the labels is re-drawn uniformly AFTER the images were formed.  The clean
    set (0.0) is separable -- a trained optimizer drives the MLP's cross-entropy from ln 10 to ~1e-5 in 200 steps,
    where a relative error of the loss measures nothing; with 0.1 the achievable loss is ~0.5 (about where the
    784-20-10 MLP gets on the real digits in 200 steps), which is what bench.py's config 5 and the
    trained-parity test use."""
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, 10, size=num_examples).astype(np.int64)
    protos = rng.random((10, 28 * 28)) < 0.2
    images = (protos[labels] * rng.random((num_examples, 28 * 28))).astype(np.float32)
    if label_noise > 0.0:
        flip = rng.random(num_examples) < label_noise
        labels = np.where(flip, rng.integers(0, 10, size=num_examples), labels).astype(np.int64)
    return {"images": images.reshape(num_examples, 28, 28, 1), "labels": labels}


class MnistDataMissing(FileNotFoundError, NotImplementedError):
    """No MNIST arrays: neither ``data=`` nor L2O_MNIST_NPZ.  A FileNotFoundError (what problems.mnist raises) and a
    NotImplementedError (what util.get_config("mnist_conv") raised before the conv net was implemented)."""


def _load_mnist(mode, name="mnist"):
    import os
    path = os.environ.get("L2O_MNIST_NPZ")
    if not path:
        raise MnistDataMissing(
            "problems.%s needs the MNIST arrays: pass data={'images': [N,28,28,1], 'labels': [N]} "
            "(problems.synthetic_mnist() gives an offline stand-in) or point L2O_MNIST_NPZ at an .npz with "
            "'{mode}_images' / '{mode}_labels' (the reference downloads them, DM/problems.py:267-272)" % name)
    z = np.load(path)
    return {"images": z["%s_images" % mode], "labels": z["%s_labels" % mode]}


def mnist(layers, activation="sigmoid", batch_size=128, mode="train", data=None, sampler=None):
    """Mnist classification with a multi-layer perceptron.  DM/problems.py:254-288.

    ``layers=(20,)`` (util.get_config("mnist")) has the fused persistent unrolls; more hidden layers (``(20, 20)``:
    "mnist_deeper", DM/util.py:157-163; up to three of <= 32 units) run on the step-granular kernels (l2o_mlp_deep_fg).
    ``data`` / ``sampler(n_evals, batch, n_data) -> indices`` are ours (offline / parity tests);
    by default every evaluation draws a fresh uniform minibatch like the reference (:282-284)."""
    if activation not in ("sigmoid", "relu"):
        raise ValueError("{} activation not supported".format(activation))
    layers = tuple(layers)
    if not 1 <= len(layers) <= 3 or any(not 1 <= int(h) <= 32 for h in layers):
        raise NotImplementedError("problems.mnist is implemented for one to three hidden layers of at most 32 units "
                                  "(got layers=%r)" % (layers,))
    if data is None:
        data = _load_mnist(mode)
    images = np.asarray(data["images"], np.float32)
    labels = np.asarray(data["labels"]).astype(np.int32)
    n_in = int(np.prod(images.shape[1:]))

    def build():
        _scope.append("mlp")
        try:
            widths = [n_in] + [int(h) for h in layers] + [10]       # snt.nets.MLP(list(layers) + [10]), DM/problems.py:275
            vs = []
            for l in range(len(widths) - 1):
                vs.append(get_variable("linear_%d/w" % l, [widths[l], widths[l + 1]], initializer=_nn_initializers["w"]))
                vs.append(get_variable("linear_%d/b" % l, [widths[l + 1]], initializer=_nn_initializers["b"]))
        finally:
            _scope.pop()
        hyper = {"images": images, "labels": labels, "batch_size": int(batch_size), "activation": activation,
                 "sampler": sampler, "layers": tuple(int(h) for h in layers)}
        return [Term(_abi.PROB_MLP, tuple(vs), {}, hyper, 1.0)]

    return _Build("mnist", build)


def _image_net_data(name, shape, data, batch_size):
    """What the image-net factories do with their arrays: images as ONE contiguous float32 [N, pixels] array (its id keys the
    graph's upload cache) and int32 labels; refuses images that are not ``shape`` and minibatches outside 2 .. 1024."""
    images = np.asarray(data["images"], np.float32)
    labels = np.asarray(data["labels"]).astype(np.int32)
    pixels = int(np.prod(shape))
    if int(np.prod(images.shape[1:])) != pixels:
        raise ValueError("problems.%s takes %s images (got %r)" % (name, "x".join(str(n) for n in shape), images.shape))
    if not 2 <= int(batch_size) <= 1024:
        raise NotImplementedError("problems.%s is implemented for minibatches of 2 to 1024 (got %d)" % (name, batch_size))
    return np.ascontiguousarray(images.reshape(len(images), pixels)), labels


def _conv_net_variables(in_channels, fc_rows, batch_norm):
    """The variables of the two-conv-layer nets of mnist_conv and cifar10, in the graph's order."""
    w = _nn_initializers["w"]
    vs = [get_variable("conv_layer1/weights1", [3, 3, in_channels, 16], initializer=w),
          get_variable("conv_layer1/biases1", [16], initializer=zeros_initializer())]
    if batch_norm:
        vs += [get_variable("batch_normalization/gamma", [16], initializer=ones_initializer()),
               get_variable("batch_normalization/beta", [16], initializer=zeros_initializer())]
    vs += [get_variable("conv_layer2/weights1", [5, 5, 16, 32], initializer=w),
           get_variable("conv_layer2/biases1", [32], initializer=zeros_initializer())]
    if batch_norm:
        vs += [get_variable("batch_normalization_1/gamma", [32], initializer=ones_initializer()),
               get_variable("batch_normalization_1/beta", [32], initializer=zeros_initializer())]
    return vs + [get_variable("fc_weights", [fc_rows, 10], initializer=w),
                 get_variable("fc_bias", [10], initializer=zeros_initializer())]


def _image_net_term(kind, vs, images, labels, batch_size, batch_norm, sampler):
    hyper = {"images": images, "labels": labels, "batch_size": int(batch_size), "batch_norm": batch_norm, "sampler": sampler}
    return [Term(kind, tuple(vs), {}, hyper, 1.0)]


def mnist_conv(batch_norm=True, batch_size=128, mode="train", data=None, sampler=None):
    """Mnist classification with a small conv net.  DM/problems.py:291-352.

    conv 3x3x1x16 VALID -> [batch norm] -> ReLU -> max-pool 2 -> conv 5x5x16x32 VALID -> [batch norm] -> ReLU -> max-pool 2
    -> fc 512x10 -> ReLU (the reference's quirk) -> mean softmax cross-entropy; batch norm is tf.layers.batch_normalization(
    training=True): batch statistics, biased variance, eps 1e-3; its moving averages are read by nothing and are not
    declared.  Forward and gradient: l2o_mnist_conv_fg (the step-granular path; no fused unroll).  ``data`` / ``sampler``
    as for :func:`mnist`; a fresh uniform minibatch per evaluation by default."""
    if data is None:
        data = _load_mnist(mode, "mnist_conv")
    images, labels = _image_net_data("mnist_conv", (28, 28, 1), data, batch_size)
    batch_norm = bool(batch_norm)

    def build():
        return _image_net_term(_abi.PROB_MNIST_CONV, _conv_net_variables(1, 512, batch_norm), images, labels, batch_size,
                               batch_norm, sampler)

    return _Build("mnist_conv", build)


def synthetic_cifar10(num_examples=2048, seed=0, label_noise=0.0):
    """A deterministic stand-in for the CIFAR-10 arrays (no dataset ships with this repo and there is no network): images
    [N,32,32,3] (NHWC) in [0,1], labels [N] in 0..9.  Every class has a prototype of 8x8 colour blocks of 4x4 pixels; an
    image is 0.6 x its class's prototype plus 0.4 x uniform noise, so the classes separate under the net's stride-2 convs
    and pools.  ``label_noise``: that fraction of the labels is re-drawn uniformly AFTER the images were formed (as in
    :func:`synthetic_mnist`)."""
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, 10, size=num_examples).astype(np.int64)
    protos = rng.random((10, 8, 8, 3)).repeat(4, axis=1).repeat(4, axis=2)
    images = (0.6 * protos[labels] + 0.4 * rng.random((num_examples, 32, 32, 3))).astype(np.float32)
    if label_noise > 0.0:
        flip = rng.random(num_examples) < label_noise
        labels = np.where(flip, rng.integers(0, 10, size=num_examples), labels).astype(np.int64)
    return {"images": images, "labels": labels}


class Cifar10DataMissing(FileNotFoundError, NotImplementedError):
    """No CIFAR-10 arrays: neither ``data=`` nor the binary files.  A FileNotFoundError (the files are missing) and a
    NotImplementedError (what util.get_config("cifar_conv") raised before the conv net was implemented)."""


_CIFAR10_FOLDER = "cifar-10-batches-bin"          # DM/problems.py:43


def _load_cifar10(path, mode):
    """The reference's binary files (DM/problems.py:378-401) read with NumPy: records of one label byte and 3072 image
    bytes in CHW order; the images come back HWC and divided by 255.  L2O_CIFAR10_DIR, when set, replaces ``path``.  Never
    downloads."""
    import os
    if mode == "train":
        names = ["data_batch_%d.bin" % i for i in range(1, 6)]
    elif mode == "test":
        names = ["test_batch.bin"]
    else:
        raise ValueError("Mode {} not recognised".format(mode))
    root = os.environ.get("L2O_CIFAR10_DIR") or path
    files = [os.path.join(root, _CIFAR10_FOLDER, n) for n in names]
    missing = [f for f in files if not os.path.isfile(f)]
    if missing:
        raise Cifar10DataMissing(
            "problems.cifar10 needs the CIFAR-10 binary files: %s is missing (looked under %r; set L2O_CIFAR10_DIR to the "
            "directory that holds %s/, or pass data={'images': [N,32,32,3], 'labels': [N]} -- problems.synthetic_cifar10() "
            "gives an offline stand-in; nothing is downloaded)" % (missing[0], root, _CIFAR10_FOLDER))
    raw = np.concatenate([np.fromfile(f, np.uint8) for f in files])
    if raw.size % 3073:
        raise ValueError("CIFAR-10 binary files hold records of 3073 bytes (got %d bytes)" % raw.size)
    rec = raw.reshape(-1, 3073)
    images = rec[:, 1:].reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1).astype(np.float32) / 255.0
    return {"images": images, "labels": rec[:, 0].astype(np.int64)}


def cifar10(path, batch_norm=True, batch_size=128, num_threads=4, min_queue_examples=1000, mode="train", data=None,
            sampler=None):
    """Cifar10 classification with a convolutional network.  DM/problems.py:369-458.

    conv 3x3x3x16 stride 2 VALID -> [batch norm] -> ReLU -> max-pool 2 -> conv 5x5x16x32 stride 2 VALID -> [batch norm] ->
    ReLU -> max-pool 2 -> fc 32x10 -> ReLU (the reference's quirk) -> mean softmax cross-entropy; batch norm as in
    :func:`mnist_conv`.  Forward and gradient: l2o_cifar_conv_fg (the step-granular path; no fused unroll).

    The data come from ``data`` ({'images': [N,32,32,3] in [0,1], 'labels': [N]}) or else from the reference's binary files
    under ``<path>/cifar-10-batches-bin/`` (``L2O_CIFAR10_DIR``, when set, replaces ``path``); nothing is downloaded.  Every
    evaluation draws a fresh uniform minibatch of ``batch_size`` rows (or ``sampler(n_evals, batch, n_data)``'s); the
    reference dequeues from a tf.RandomShuffleQueue fed by ``num_threads`` readers with ``min_queue_examples`` kept back,
    which draws differently.  ``num_threads`` and ``min_queue_examples`` are accepted for the reference's signature and
    have no effect."""
    del num_threads, min_queue_examples
    if data is None:
        data = _load_cifar10(path, mode)
    images, labels = _image_net_data("cifar10", (32, 32, 3), data, batch_size)
    batch_norm = bool(batch_norm)

    def build():
        return _image_net_term(_abi.PROB_CIFAR_CONV, _conv_net_variables(3, 32, batch_norm), images, labels, batch_size,
                               batch_norm, sampler)

    return _Build("cifar10", build)


def LeNet(path, conv_channels=None, linear_layers=None, batch_norm=True, batch_size=128, num_threads=4,
          min_queue_examples=1000, mode="train", data=None, sampler=None):
    """LeNet-5 on CIFAR-10 with sigmoids, max-pooling and Sonnet batch norm.  DM/problems.py:461-537, as
    util.get_config("lenet") (DM/util.py:176-184) calls it: ``conv_channels=(6, 16)``, ``linear_layers=(120, 84)``.

    conv 5x5x3x6 VALID -> [batch norm] -> sigmoid -> max-pool 2 -> conv 5x5x6x16 VALID -> [batch norm] -> sigmoid ->
    max-pool 2 -> flatten (400) -> linear 400x120 -> [batch norm] -> sigmoid -> linear 120x84 -> [batch norm] -> sigmoid ->
    linear 84x10 -> mean softmax cross-entropy.  Batch norm is snt.BatchNorm in training mode: batch statistics, biased
    variance, eps 1e-3, an offset ``beta`` and no scale.  Sonnet keeps beta's shape with singleton axes ([1,1,1,6],
    [1,120]); they are declared flat here ([6], [120]), which changes no arithmetic.  Its moving averages are not trainable
    and nothing reads them in training mode: they are not declared.  Every ``w`` and ``b`` is drawn from N(0, 0.01^2).
    Forward and gradient: l2o_lenet_fg (the step-granular path; no fused unroll).

    Only ``conv_channels=(6, 16)``, ``linear_layers=(120, 84)`` is implemented (the reference cannot build the ``None``
    defaults either).  The data and the minibatches come as in :func:`cifar10`; ``num_threads`` and ``min_queue_examples``
    are accepted for the reference's signature and have no effect."""
    del num_threads, min_queue_examples
    shape = (None if conv_channels is None else tuple(conv_channels),
             None if linear_layers is None else tuple(linear_layers))
    if shape != ((6, 16), (120, 84)):
        raise NotImplementedError("problems.LeNet is implemented for conv_channels=(6, 16), linear_layers=(120, 84) "
                                  "(got conv_channels=%r, linear_layers=%r)" % (conv_channels, linear_layers))
    if data is None:
        data = _load_cifar10(path, mode)
    images, labels = _image_net_data("LeNet", (32, 32, 3), data, batch_size)
    batch_norm = bool(batch_norm)

    def build():
        w, b = _nn_initializers["w"], _nn_initializers["b"]
        vs = []
        for i, sh in enumerate([(5, 5, 3, 6), (5, 5, 6, 16)]):
            vs += [get_variable("conv_net_2d/conv_2d_%d/w" % i, sh, initializer=w),
                   get_variable("conv_net_2d/conv_2d_%d/b" % i, [sh[3]], initializer=b)]
            if batch_norm:
                vs.append(get_variable("conv_net_2d/batch_norm_%d/beta" % i, [sh[3]], initializer=zeros_initializer()))
        widths = [400, 120, 84, 10]
        for i in range(3):
            vs += [get_variable("mlp/linear_%d/w" % i, [widths[i], widths[i + 1]], initializer=w),
                   get_variable("mlp/linear_%d/b" % i, [widths[i + 1]], initializer=b)]
            if batch_norm and i < 2:
                vs.append(get_variable("mlp/batch_norm%s/beta" % ("" if i == 0 else "_1"), [widths[i + 1]],
                                       initializer=zeros_initializer()))
        return _image_net_term(_abi.PROB_LENET, vs, images, labels, batch_size, batch_norm, sampler)

    return _Build("LeNet", build)


def confocal_microscopy_3d(batch_size=128, num_points=5, ROI=[28, 28, 28], stddev=0.01, dtype="float32", inference=False,
                           data=None, fused=False):
    """3-D point-spread-function fitting.  DM/problems.py:701-956 (util.get_config: batch_size=32, num_points=5).

    Per batch row, ``num_points`` Gaussian point-spread functions, each integrated over the voxels of the ``ROI`` = [Rx, Ry,
    Rz] volume, plus a background value: pred = sum_p I0 Ex[ix] Ey[iy] Ez[iz] / 8 + bg_var with
    E[k] = erf((k + .5 - c) / (sqrt2 sigma)) - erf((k - .5 - c) / (sqrt2 sigma)).  The trainable values are raw: I0 = 0.5 +
    1.5 t, c = 0.5 + (R - 1.5) t per axis, sigma_xy = sigma_z = 2 + 2 t (the quantiles of uniform priors, not clipped).
    loss = mean_b sum_v (pred - l2_normalize(target))^2, the target being the same sum over the non-trainable ``*_sim``
    variables (re-drawn on every reset), or with ``inference=True`` a supplied volume.  Forward and gradient:
    l2o_confocal_fg (the step-granular path, the default).

    ``fused`` (an extension, default off): where one (20, 20) LSTM net steps every variable, run the unroll as ONE persistent
    launch (l2o_confocal_unroll: one workgroup per batch row) instead of the step-granular launches; the graph falls back
    to those wherever the fused form does not apply (``last_path`` tells which ran).  Several such instances of one shape
    (replicas.Replicas, run and train_step) share launches of up to 32 -- one workgroup per row of EVERY instance, form
    "rows" (l2o_confocal_unroll_multi) --, with results bit-identical to their own launches.

    Variables as the reference declares them, each [batch_size, 1]: per point I_var_i, x_var_i, y_var_i, z_var_i,
    sigmaxy_var_i, sigmaz_var_i ~ U[0, 1); then per point the non-trainable I_sim_i, x_sim_i, y_simi (the reference's
    spelling), z_sim_i, sigmaxy_sim_i, sigmaz_sim_i ~ U[0, 1); then bg_var ~ N(0, stddev^2); then the non-trainable bg_sim
    ~ U[0, 1).  With ``inference=True`` there are no ``*_sim`` variables.

    ``data`` (an extension): a variable name present in the dict fixes that variable's initial value; with
    ``inference=True`` ``data["img"]`` [batch_size, Rx Ry Rz] is required (the reference feeds a placeholder there), its
    flat voxel index being (iy Rx + ix) Rz + iz, TF's default meshgrid order.
    Implemented for batch_size in [1, 1024], num_points in [1, 8] and ROI edges in [2, 32]."""
    roi = tuple(int(r) for r in ROI)
    batch_size, num_points, inference = int(batch_size), int(num_points), bool(inference)
    if len(roi) != 3 or not (1 <= batch_size <= 1024 and 1 <= num_points <= 8 and all(2 <= r <= 32 for r in roi)):
        raise NotImplementedError("problems.confocal_microscopy_3d is implemented for batch_size in [1, 1024], num_points "
                                  "in [1, 8] and three ROI edges in [2, 32] (got batch_size=%d, num_points=%d, ROI=%r)"
                                  % (batch_size, num_points, list(ROI)))
    img = None
    if inference:
        if data is None or "img" not in data:
            raise ValueError("problems.confocal_microscopy_3d(inference=True) needs data['img'] of shape [batch_size, "
                             "Rx * Ry * Rz] (the reference feeds a placeholder)")
        img = np.ascontiguousarray(np.asarray(data["img"], np.float32).reshape(batch_size, roi[0] * roi[1] * roi[2]))

    def build():
        parts = ("I", "x", "y", "z", "sigmaxy", "sigmaz")

        def var(name, default, trainable):
            return get_variable(name, shape=[batch_size, 1], dtype=dtype, trainable=trainable,
                                initializer=_maybe_const(data, name, [batch_size, 1], default))

        tr = [var("%s_var_%d" % (p, i), random_uniform_initializer(), True) for i in range(num_points) for p in parts]
        sim = []
        if not inference:
            sim = [var(("y_sim%d" if p == "y" else p + "_sim_%d") % i, random_uniform_initializer(), False)
                   for i in range(num_points) for p in parts]
        tr.append(var("bg_var", random_normal_initializer(stddev=stddev), True))
        if not inference:
            sim.append(var("bg_sim", random_uniform_initializer(), False))
        hyper = {"batch_size": batch_size, "num_points": num_points, "roi": roi, "inference": inference, "img": img,
                 "fused": bool(fused)}
        return [Term(_abi.PROB_CONFOCAL, tuple(tr), {"sim": tuple(sim)}, hyper, 1.0)]

    return _Build("confocal_microscopy_3d", build)


def vgg16_cifar10(path, batch_norm=False, batch_size=128, num_threads=4, min_queue_examples=1000, mode="train", data=None,
                  sampler=None, channels=(64, 128, 256, 512, 512)):
    """Cifar10 classification with VGG-16.  DM/problems.py:637-694 and DM/vgg16.py:44-98, as util.get_config("vgg16")
    (DM/util.py:192-197) calls it.

    Five blocks of (2, 2, 3, 3, 3) layers of widths ``channels``, each layer conv 3x3 stride 1 SAME + bias -> ReLU, each
    block closed by max-pool 2x2 stride 2 (32 -> 16 -> 8 -> 4 -> 2 -> 1) -> flatten (512) -> linear 512x10 + bias ->
    softmax -> mean softmax cross-entropy that takes those PROBABILITIES as its logits (the reference's quirk):
    loss = mean_b -log softmax(p_b)[label_b] with p_b = softmax(z_b), which lies in about [1.46, 2.46].  The reference has
    commented its two hidden fc layers and their dropouts out, and nothing reads its ``batch_norm``, ``is_training`` or
    ``keep_prob``: ``batch_norm`` is accepted for the reference's signature and has no effect.  Conv and fc weights are
    drawn from N(0, 0.01^2), the conv biases are 0 and ``fc/biases`` is the constant 1.0.  Forward and gradient:
    l2o_vgg16_fg (the step-granular path; no fused unroll; first-order meta-gradients only).

    ``channels`` (an extension): the widths of the five blocks, each a multiple of 8 in [8, 512]; the default is the
    reference's net, 14 719 818 coordinates in 28 variables.  The data and the minibatches come as in :func:`cifar10`;
    ``num_threads`` and ``min_queue_examples`` are accepted for the reference's signature and have no effect."""
    del batch_norm, num_threads, min_queue_examples
    try:
        channels = tuple(int(c) for c in channels)
    except TypeError:
        channels = (channels,)
    if len(channels) != 5 or any(c % 8 or not 8 <= c <= 512 for c in channels):
        raise NotImplementedError("problems.vgg16_cifar10 is implemented for five channels, each a multiple of 8 in [8, 512] "
                                  "(got channels=%r)" % (channels,))
    if data is None:
        data = _load_cifar10(path, mode)
    images, labels = _image_net_data("vgg16_cifar10", (32, 32, 3), data, batch_size)

    def build():
        w = random_normal_initializer(stddev=0.01)
        vs, c_in = [], 3
        for b, (layers, c_out) in enumerate(zip((2, 2, 3, 3, 3), channels)):
            for i in range(layers):
                name = "block%d_conv%d" % (b + 1, i + 1)
                vs += [get_variable(name + "/weights", [3, 3, c_in, c_out], initializer=w),
                       get_variable(name + "/biases", [c_out], initializer=zeros_initializer())]
                c_in = c_out
        vs += [get_variable("fc/weights", [c_in, 10], initializer=w),
               get_variable("fc/biases", [10], initializer=ones_initializer())]
        term, = _image_net_term(_abi.PROB_VGG16, vs, images, labels, batch_size, False, sampler)
        term.hyper["channels"] = channels
        return [term]

    return _Build("vgg16_cifar10", build)


def NAS(path, batch_norm=True, batch_size=128, num_threads=4, min_queue_examples=1000, mode="train", data=None,
        sampler=None):
    """Cifar10 classification with a NAS cell.  DM/problems.py:540-634, as util.get_config("nas") (DM/util.py:185-190) calls
    it.

    With L(x) = relu([batch norm](conv 3x3 stride 1 SAME to 16 channels + bias)): node0 = L(image), n02 = L(node0), node1 =
    L(node0), n13 = L(node1), node2 = avg_pool 3x3 stride 1 SAME (node1) + n02 (the pool divides by the number of valid
    cells), node3 = node2 + n13 + node0 -> mean over the 1024 positions -> fc 16x10 -> ReLU (the reference's quirk) -> mean
    softmax cross-entropy; batch norm as in :func:`mnist_conv`.  The variables, in the reference's creation order: per layer
    (``node0``, ``node0_onto_node2``, ``node1``, ``node1_onto_node3``) ``weights1``, ``biases1`` and with batch norm
    ``batch_normalization[_i]/gamma`` and ``beta``, then ``fc_weights`` and ``fc_bias``: 18 variables and 7 706 coordinates
    with batch norm, 10 and 7 578 without.  Forward and gradient: l2o_nas_fg (the step-granular path; no fused unroll;
    first-order meta-gradients only).

    The data and the minibatches come as in :func:`cifar10`; ``num_threads`` and ``min_queue_examples`` are accepted for the
    reference's signature and have no effect."""
    del num_threads, min_queue_examples
    if data is None:
        data = _load_cifar10(path, mode)
    images, labels = _image_net_data("NAS", (32, 32, 3), data, batch_size)
    batch_norm = bool(batch_norm)

    def build():
        w = random_normal_initializer(stddev=0.01)
        vs, c_in = [], 3
        for i, name in enumerate(("node0", "node0_onto_node2", "node1", "node1_onto_node3")):
            vs += [get_variable(name + "/weights1", [3, 3, c_in, 16], initializer=w),
                   get_variable(name + "/biases1", [16], initializer=zeros_initializer())]
            if batch_norm:
                bn = "batch_normalization" + ("_%d" % i if i else "")
                vs += [get_variable(bn + "/gamma", [16], initializer=ones_initializer()),
                       get_variable(bn + "/beta", [16], initializer=zeros_initializer())]
            c_in = 16
        vs += [get_variable("fc_weights", [16, 10], initializer=w),
               get_variable("fc_bias", [10], initializer=zeros_initializer())]
        return _image_net_term(_abi.PROB_NAS, vs, images, labels, batch_size, batch_norm, sampler)

    return _Build("NAS", build)


def _not_on_hot_path(name, where):
    def factory(*args, **kwargs):
        raise NotImplementedError(
            "problems.%s (%s) is outside the accelerated hot path of this build; see DESIGN.md "
            "'out of scope'" % (name, where))
    factory.__name__ = name
    return factory


# neural-network / data-dependent optimizees of the reference (conv nets, TF queues,
# downloads).  Declared so that `getattr(problems, name)` fails with a clear message.
# util.get_config("cifar-multi") (DM/util.py:212-230) calls cifar10 with conv_channels / linear_layers, which the
# reference's own cifar10 does not take
cifar_multi = _not_on_hot_path("cifar10(conv_channels=..., linear_layers=...)", "DM/util.py:212")
