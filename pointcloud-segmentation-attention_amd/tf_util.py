"""Shared-MLP layers of pointnet2_tensorflow/utils/tf_util.py, inference mode, on gfx950.

tf_util.conv2d / conv1d with a 1x1 kernel (tf_util.py:52-117, :120-185) are per-point dense
layers: conv, bias_add, batch_norm (tf.contrib.layers.batch_norm, :512-531), activation. In
inference mode (is_training=False) the batch norm is the per-channel affine map
    bn(x) = (x - moving_mean) * gamma / sqrt(moving_variance + eps) + beta,  eps = 1e-3
so a layer is  y = act((x W + b) * scale + shift). Layers are packed once (pn2_mlp_pack) into
the matrix-core operand layout of csrc/mlp.hip and then run fused with the grouping / the
interpolation before them and the pooling after them (pointnet_util.pointnet_sa_module,
pointnet_fp_module) or on plain rows (conv2d / conv1d here).

Parameters live in a ParamStore keyed by the reference's TF variable names
("layer1/conv0/weights", ".../biases", ".../bn/gamma", ".../bn/beta", ".../bn/moving_mean",
".../bn/moving_variance"), so a TF checkpoint's variables, exported to a dict of arrays, load
unchanged. Missing variables are created with the reference's initialisers (xavier weights,
zero biases, gamma 1, beta 0, moving mean 0, moving variance 1; tf_util.py:24-49).

Training mode (is_training=True: batch norm on batch statistics, tf_util.py:512-531) runs on
the HIP training layer torch.ops.pn2.mlp_layer_train (csrc/mlp_train.hip) through mlp_train
(and bn_train for a batch norm on its own), for the variables of a store made trainable with ParamStore.trainable(): device-resident
leaves with gradients, moving averages updated in place on the device. The segmentation head's
last operations train on csrc/head_train.hip: dropout (tf_util.py:594-612) and
sparse_softmax_cross_entropy (the tf.losses call of pointnet2_sem_seg.get_loss).

Precision. The packed inference layers are fp32 by default and can be packed for the bf16
matrix cores instead: ParamStore(precision="bf16") or store.set_precision("bf16") makes every
packed_mlp / packed_dense of that store bf16 unless the call names a precision itself (the
models name "fp32" for fc2, whose 21 logits decide the argmax, and for the attention's query
Dense, which is not matrix-core work). The numerical contract of a bf16 layer is written at
pn2_mlp_pack_bf16 in include/pn2hip.h: operands rounded to bf16 (nearest even), exact products,
fp32 sums and fp32 everything else. The inference precision never reaches training:
is_training=True on a trainable store ignores it.

Training precision. The HIP training layers are fp32 by default and have a bf16 matrix-core mode
of their own, also an opt-in: ParamStore(train_precision="bf16") or
store.set_train_precision("bf16") makes every layer that mlp_train runs for that store (the SA,
MSG and FP modules' MLPs, the attention SA modules' MLP and mlp2, conv2d / conv1d with
is_training=True) run its three GEMMs, the forward product, the input gradient and the weight
gradient, on the bf16 matrix cores (torch.ops.pn2.mlp_layer_train_bf16 and its namesakes) unless
the call names precision="fp32" itself (the models do for fc2). The contract is written beside
the inference one in include/pn2hip.h: operands rounded to bf16 per step, exact products, fp32
sums; the variables stay fp32 master copies, and the batch statistics, the activation and its
backward, the fused max pool, the moving averages, Adam, the attention's projections
(attn_kv_train), bn_train, the head's dropout and loss and the geometry stay fp32. The two
settings are independent: a store with only precision="bf16" still trains in fp32. What bf16
training does to a converged mIoU has not been measured (there is no dataset here).
"""
import math

import numpy as np
import torch

from . import _torch_ops
from ._lib import (PN2_MLP_BF16, PN2_MLP_MAX_LAYERS, PN2_MLP_RELU, InvalidArgumentError,
                   MlpLayer, check, device_tensor, lib, ptr, stream_of)

BN_EPSILON = 1e-3  # tf.contrib.layers.batch_norm's default epsilon
MOVING_SUFFIXES = ("moving_mean", "moving_variance")  # batch norm's non-trainable variables
CONV_SUFFIXES = ("weights", "biases", "bn/gamma", "bn/beta", "bn/moving_mean",
                 "bn/moving_variance")
DENSE_SUFFIXES = ("kernel", "bias")
BN_SUFFIXES = ("gamma", "beta", "moving_mean", "moving_variance")
# of a packed inference layer (pn2_mlp_pack / pn2_mlp_pack_bf16) and of a HIP training layer
PRECISIONS = ("fp32", "bf16")


def check_precision(precision):
    if precision not in PRECISIONS:
        raise InvalidArgumentError(f"precision must be one of {PRECISIONS}, got {precision!r}")
    return precision


# What runs a layer whose input row the fused MLP kernel refuses (1,280 channels and up; the
# attention networks have such layers): "hip", the K-streamed kernel (pn2_dense_wide, and the
# HIP training layers in training), or "torch", a matmul and a hand-written batch norm from torch
# ops (attention_layer._layer_torch). ParamStore(wide_layers=...) selects it per store. The
# default stays "torch", what these layers ran on before the kernel existed: the kernel is
# faster at 1,536 and 2,304 input channels and slower at the pooling model's widest layers
# (profiles/dense_wide/summary.json); "hip" is the tested opt-in.
WIDE_LAYERS = ("hip", "torch")
WIDE_LAYERS_DEFAULT = "torch"


def check_wide_layers(value):
    if value not in WIDE_LAYERS:
        raise InvalidArgumentError(f"wide_layers must be one of {WIDE_LAYERS}, got {value!r}")
    return value


class ParamStore(dict):
    """TF variable name -> float32 tensor, with the reference's initialisers for misses."""

    def __init__(self, *args, seed=0, device="cuda", precision="fp32", train_precision="fp32",
                 wide_layers=WIDE_LAYERS_DEFAULT, **kw):
        super().__init__()
        self.seed = seed
        self.device = device
        self.precision = check_precision(precision)
        self.train_precision = check_precision(train_precision)
        self.wide_layers = check_wide_layers(wide_layers)
        self.is_trainable = False
        self._packed = {}
        self._stamps = {}
        for k, v in dict(*args, **kw).items():
            self[k] = v

    def __setitem__(self, name, value):
        # checkpoint arrays (numpy or torch) are kept as float32 CPU tensors; a trainable store
        # keeps them on its device, as leaves that require a gradient (moving statistics: not)
        t = torch.as_tensor(value, dtype=torch.float32).detach()
        if self.is_trainable:
            t = t.to(self.device, copy=True).contiguous()
            t.requires_grad_(not name.endswith(MOVING_SUFFIXES))
        else:
            t = t.cpu()
        super().__setitem__(name, t)

    def trainable(self, device="cuda"):
        """Make the store trainable: every variable moves to `device`; conv / dense weights,
        biases, gamma and beta become leaves with requires_grad=True (existing ones now, later
        ones when they are created), the moving statistics plain device tensors that mlp_train
        updates in place. Returns the store. With a trainable store, is_training=True runs the
        HIP training layers (mlp_train); build the optimiser from parameters() after the model
        has run once, so that every variable exists."""
        if self.is_trainable and torch.device(self.device) == torch.device(device):
            return self
        self.device = device
        self.is_trainable = True
        for name in list(self):
            self[name] = dict.__getitem__(self, name)
        self.invalidate()
        return self

    def set_precision(self, precision):
        """The precision of the store's packed inference layers from now on: "fp32" (the
        default) or "bf16" (the opt-in matrix-core mode; see the module docstring). Drops the
        packed copies, so the next call packs again. Training (is_training=True) ignores it.
        Returns the store."""
        self.precision = check_precision(precision)
        self.invalidate()
        return self

    def set_train_precision(self, precision):
        """The precision of the store's HIP training layers from now on: "fp32" (the default) or
        "bf16" (the opt-in matrix-core mode of mlp_train; see the module docstring). Independent
        of set_precision. The training layers pack per step, so nothing is dropped. Returns the
        store."""
        self.train_precision = check_precision(precision)
        return self

    def parameters(self):
        """The trainable variables (torch.optim.Adam(store.parameters()))."""
        for t in self.values():
            if t.requires_grad:
                yield t

    def state_dict(self):
        """TF variable name -> float32 numpy array on the CPU (loads back with ParamStore(d))."""
        return {k: v.detach().cpu().numpy().copy() for k, v in self.items()}

    def stamp(self, scopes, suffixes):
        """In-place versions of the variables `scopes` x `suffixes` that exist (trainable store:
        an optimiser step or a moving-average update changes it), or None."""
        if not self.is_trainable:
            return None
        found = (dict.get(self, f"{s}/{k}") for s in scopes for k in suffixes)
        return tuple((id(t), t._version) for t in found if t is not None)

    def cached(self, key, scopes, suffixes, make):
        """The packed object cached under `key`, rebuilt with make() when a variable it was
        packed from has changed since."""
        stamp = self.stamp(scopes, suffixes)
        hit = self._packed.get(key)
        if hit is None or self._stamps.get(key) != stamp:
            hit = make()
            self._packed[key] = hit
            self._stamps[key] = self.stamp(scopes, suffixes)
        return hit

    def _init(self, name, shape, kind):
        if kind == "xavier":  # tf.contrib.layers.xavier_initializer(): glorot uniform
            fan_in = int(np.prod(shape[:-1]))
            fan_out = int(np.prod(shape[:-2])) * int(shape[-1])
            lim = math.sqrt(6.0 / (fan_in + fan_out))
            # deterministic per variable name
            g = np.random.default_rng([self.seed] + [ord(c) for c in name])
            return g.uniform(-lim, lim, size=shape).astype(np.float32)
        value = {"zeros": 0.0, "ones": 1.0}[kind]
        return np.full(shape, value, dtype=np.float32)

    def get(self, name, shape, kind):
        if name not in self:
            self[name] = torch.from_numpy(self._init(name, shape, kind))
        t = self[name]
        if tuple(t.shape) != tuple(shape):
            t = t.reshape(shape)
        return t

    def conv(self, scope, cin, cout, bn=True):
        """The variables tf_util.conv2d(..., scope) creates (kernel [1,1,cin,cout])."""
        p = {"weights": self.get(f"{scope}/weights", (1, 1, cin, cout), "xavier").reshape(
            cin, cout), "biases": self.get(f"{scope}/biases", (cout,), "zeros")}
        if bn:
            p["gamma"] = self.get(f"{scope}/bn/gamma", (cout,), "ones")
            p["beta"] = self.get(f"{scope}/bn/beta", (cout,), "zeros")
            p["moving_mean"] = self.get(f"{scope}/bn/moving_mean", (cout,), "zeros")
            p["moving_variance"] = self.get(f"{scope}/bn/moving_variance", (cout,), "ones")
        return p

    def dense(self, scope, cin, cout):
        """The variables of a tf.layers.Dense(cout) built under `scope` (glorot-uniform kernel,
        zero bias: the Keras defaults)."""
        return {"weights": self.get(f"{scope}/kernel", (cin, cout), "xavier"),
                "biases": self.get(f"{scope}/bias", (cout,), "zeros")}

    def bn(self, scope, c):
        """The variables of a standalone batch_norm_template(scope) (tf_util.py:512-531)."""
        return {"gamma": self.get(f"{scope}/gamma", (c,), "ones"),
                "beta": self.get(f"{scope}/beta", (c,), "zeros"),
                "moving_mean": self.get(f"{scope}/moving_mean", (c,), "zeros"),
                "moving_variance": self.get(f"{scope}/moving_variance", (c,), "ones")}

    def invalidate(self):
        """Drop packed copies (call after changing parameters in place)."""
        self._packed.clear()
        self._stamps.clear()


_default_store = None


def default_store():
    """The process-wide store (the analogue of TF's default graph variables)."""
    global _default_store
    if _default_store is None:
        _default_store = ParamStore()
    return _default_store


class PackedLayer:
    """One conv layer in pn2_mlp_pack's layout, or with precision="bf16" in
    pn2_mlp_pack_bf16's (device buffer) + its struct pn2_mlp_layer."""

    def __init__(self, weights, biases=None, gamma=None, beta=None, moving_mean=None,
                 moving_variance=None, relu=True, eps=BN_EPSILON, device="cuda",
                 precision="fp32"):
        self.precision = check_precision(precision)
        # a trainable store's variables are packed by value (no autograd through the packing)
        weights, biases, gamma, beta, moving_mean, moving_variance = (
            v.detach() if isinstance(v, torch.Tensor) else v
            for v in (weights, biases, gamma, beta, moving_mean, moving_variance))
        w = torch.as_tensor(weights, dtype=torch.float32)
        if w.dim() == 4:  # TF conv2d kernel [1,1,cin,cout]
            w = w.reshape(w.shape[-2], w.shape[-1])
        if w.dim() != 2:
            raise InvalidArgumentError("weights must be (cin, cout) or [1, 1, cin, cout]")
        self.cin, self.cout = int(w.shape[0]), int(w.shape[1])
        self.relu = bool(relu)
        dev = torch.device(device)
        w = w.to(dev).contiguous()
        b = None if biases is None else torch.as_tensor(biases, dtype=torch.float32).to(dev)
        scale = shift = None
        if gamma is not None:
            # inference batch norm (tf_util.py:512-531): (x - mean) * gamma / sqrt(var + eps) + beta
            g = torch.as_tensor(gamma, dtype=torch.float64)
            var = torch.as_tensor(moving_variance, dtype=torch.float64)
            mean = torch.as_tensor(moving_mean, dtype=torch.float64)
            bt = torch.as_tensor(beta, dtype=torch.float64)
            s64 = g / torch.sqrt(var + eps)
            scale = s64.to(torch.float32).to(dev).contiguous()
            shift = (bt - mean * s64).to(torch.float32).to(dev).contiguous()
        bf16 = self.precision == "bf16"
        size, pack = ((lib().pn2_mlp_packed_size_bf16, lib().pn2_mlp_pack_bf16) if bf16 else
                      (lib().pn2_mlp_packed_size, lib().pn2_mlp_pack))
        nbytes = int(size(self.cin, self.cout))
        self.buf = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=dev)
        check(pack(ptr(w), ptr(b), ptr(scale), ptr(shift), self.cin, self.cout, ptr(self.buf),
                   nbytes, stream_of(self.buf)), "mlp_pack_bf16" if bf16 else "mlp_pack")
        self.scale, self.shift, self.bias = scale, shift, b  # kept for the training path

    def struct(self):
        return MlpLayer(self.buf.data_ptr(), self.cin, self.cout,
                        (PN2_MLP_RELU if self.relu else 0) |
                        (PN2_MLP_BF16 if self.precision == "bf16" else 0))


class SharedMLP:
    """A chain of PackedLayers run as one fused kernel (at most PN2_MLP_MAX_LAYERS)."""

    def __init__(self, layers):
        if not 1 <= len(layers) <= PN2_MLP_MAX_LAYERS:
            raise InvalidArgumentError(f"1..{PN2_MLP_MAX_LAYERS} layers per fused MLP")
        for a, b in zip(layers, layers[1:]):
            if a.cout != b.cin:
                raise InvalidArgumentError("consecutive layers must chain cout -> cin")
        self.layers = list(layers)
        self.cin, self.cout = layers[0].cin, layers[-1].cout
        self._table = (MlpLayer * len(layers))(*[l.struct() for l in layers])

    def table(self):
        return self._table, len(self.layers)

    def __call__(self, x):
        """Per-point MLP over the last axis: x (..., cin) -> (..., cout) (pn2_shared_mlp)."""
        x = device_tensor(x, "inputs", torch.float32)
        if int(x.shape[-1]) != self.cin:
            raise InvalidArgumentError(f"inputs have {int(x.shape[-1])} channels, the MLP "
                                       f"expects {self.cin}")
        rows = x.numel() // self.cin
        out = torch.empty(tuple(x.shape[:-1]) + (self.cout,), dtype=torch.float32,
                          device=x.device)
        tab, n = self.table()
        check(lib().pn2_shared_mlp(ptr(x), rows, self.cin, n, tab, ptr(out), stream_of(x)),
              "shared_mlp")
        return out


class WideLayer:
    """One fp32 PackedLayer run on the K-streamed kernel (torch.ops.pn2.dense_wide over
    pn2_dense_wide): any input width, the layers pn2_shared_mlp refuses included."""

    def __init__(self, layer):
        if layer.precision != "fp32":
            raise InvalidArgumentError("the K-streamed kernel is fp32 only: pack the layer fp32")
        self.layer = layer
        self.cin, self.cout = layer.cin, layer.cout

    def __call__(self, x):
        """x (..., cin) -> (..., cout)."""
        x = device_tensor(x, "inputs", torch.float32)
        if int(x.shape[-1]) != self.cin:
            raise InvalidArgumentError(f"inputs have {int(x.shape[-1])} channels, the layer "
                                       f"expects {self.cin}")
        return _torch_ops.call("dense_wide", x, self.layer.buf, self.cin, self.cout,
                               self.layer.relu)


def packed_mlp(store, scopes, cin, widths, bn=True, relu=True, precision=None):
    """SharedMLP over the store's variables for conv scopes `scopes` (one per width), cached
    per scope tuple. `relu` applies to every layer (tf_util.conv2d's activation_fn), and so
    does `precision` ("fp32" / "bf16"; None: the store's)."""
    precision = check_precision(store.precision if precision is None else precision)
    key = (tuple(scopes), cin, tuple(widths), bn, relu, precision)

    def make():
        layers, c = [], cin
        for scope, w in zip(scopes, widths):
            p = store.conv(scope, c, w, bn=bn)
            layers.append(PackedLayer(p["weights"], p["biases"], p.get("gamma"), p.get("beta"),
                                      p.get("moving_mean"), p.get("moving_variance"), relu=relu,
                                      device=store.device, precision=precision))
            c = w
        return SharedMLP(layers)

    return store.cached(key, scopes, CONV_SUFFIXES, make)


def packed_dense(store, scope, cin, cout, precision=None):
    """SharedMLP of one tf.layers.Dense (no activation) over the store's variables, cached.
    `precision`: "fp32" / "bf16"; None: the store's."""
    precision = check_precision(store.precision if precision is None else precision)
    key = ("dense", scope, cin, cout, precision)

    def make():
        p = store.dense(scope, cin, cout)
        return SharedMLP([PackedLayer(p["weights"], p["biases"], relu=False, device=store.device,
                                      precision=precision)])

    return store.cached(key, [scope], DENSE_SUFFIXES, make)


def bn_affine(store, scope, c, device):
    """Inference batch norm as (scale, shift) device tensors: x * scale + shift."""
    key = ("bn", scope, c)

    def make():
        p = {k: v.detach() for k, v in store.bn(scope, c).items()}
        s64 = p["gamma"].double() / torch.sqrt(p["moving_variance"].double() + BN_EPSILON)
        shift = p["beta"].double() - p["moving_mean"].double() * s64
        return (s64.float().to(device), shift.float().to(device))

    return store.cached(key, [scope], BN_SUFFIXES, make)


def conv2d(inputs, num_output_channels, kernel_size, scope, stride=[1, 1], padding='SAME',
           data_format='NHWC', use_xavier=True, stddev=1e-3, weight_decay=None,
           activation_fn=torch.relu, bn=False, bn_decay=None, is_training=None, params=None,
           precision=None):
    """tf_util.conv2d (tf_util.py:120-185) for the 1x1 kernels PointNet++ uses, NHWC.
    Extra keyword `params`: the ParamStore (default: default_store()). is_training=True needs a
    trainable store (ParamStore.trainable()) and runs mlp_train: batch-statistics batch norm,
    gradients for the input and every variable. Extra keyword `precision`: of the packed
    inference layer ("fp32" / "bf16"; None: the store's). The training layer follows the store's
    train_precision, except that precision="fp32" on the call keeps it fp32 in training too."""
    if list(kernel_size) != [1, 1] or list(stride) != [1, 1] or data_format != 'NHWC':
        raise NotImplementedError("pn2hip's conv2d is the 1x1 NHWC shared MLP of PointNet++")
    store = params if params is not None else default_store()
    if is_training and not store.is_trainable:
        raise NotImplementedError("conv2d: is_training=True needs a trainable store: call "
                                  "ParamStore.trainable() on `params` (a plain store runs the "
                                  "fused inference-mode layer only)")
    if activation_fn not in (None, torch.relu, torch.nn.functional.relu):
        raise NotImplementedError("conv2d: activation must be relu or None")
    if is_training:
        layers = torch_layers(store, [scope], int(inputs.shape[-1]), [num_output_channels],
                              bn=bn, relu=activation_fn is not None)
        if precision is not None:
            check_precision(precision)
        # "bf16" on the call names the inference pack: training follows the store's own setting
        return mlp_train(inputs, layers, bn_decay,
                         precision="fp32" if precision == "fp32" else None)
    mlp = packed_mlp(store, [scope], int(inputs.shape[-1]), [num_output_channels], bn=bn,
                     relu=activation_fn is not None, precision=precision)
    return mlp(inputs)


def conv1d(inputs, num_output_channels, kernel_size, scope, stride=1, padding='SAME',
           data_format='NHWC', use_xavier=True, stddev=1e-3, weight_decay=None,
           activation_fn=torch.relu, bn=False, bn_decay=None, is_training=None, params=None,
           precision=None):
    """tf_util.conv1d (tf_util.py:52-117) with kernel 1 (the segmentation heads' fc layers)."""
    if kernel_size != 1 or stride != 1:
        raise NotImplementedError("pn2hip's conv1d is the kernel-1 per-point layer")
    return conv2d(inputs, num_output_channels, [1, 1], scope, data_format=data_format,
                  activation_fn=activation_fn, bn=bn, bn_decay=bn_decay,
                  is_training=is_training, params=params, precision=precision)


def mlp_torch(x, layers, is_training=False, bn_decay=None):
    """The same layers composed from differentiable torch ops (the training path; batch norm
    with batch statistics over every axis but the channel axis when is_training, as
    tf.contrib.layers.batch_norm does, moving averages updated with decay bn_decay or 0.9)."""
    for L in layers:
        p = L.params
        y = x @ p["weights"].to(x.device)
        if p.get("biases") is not None:
            y = y + p["biases"].to(x.device)
        if p.get("gamma") is not None:
            gamma, beta = p["gamma"].to(x.device), p["beta"].to(x.device)
            if is_training:
                dims = tuple(range(y.dim() - 1))
                mean = y.mean(dim=dims)
                var = y.var(dim=dims, unbiased=False)
                decay = 0.9 if bn_decay is None else float(bn_decay)
                with torch.no_grad():
                    p["moving_mean"].mul_(decay).add_((1 - decay) * mean.detach().cpu())
                    p["moving_variance"].mul_(decay).add_((1 - decay) * var.detach().cpu())
            else:
                mean = p["moving_mean"].to(x.device)
                var = p["moving_variance"].to(x.device)
            y = (y - mean) * (gamma / torch.sqrt(var + BN_EPSILON)) + beta
        x = torch.relu(y) if L.relu else y
    return x


def mlp_train(x, layers, bn_decay=None, pool=None, precision=None):
    """The layers of mlp_torch(x, layers, is_training=True) on the HIP training kernels
    (torch.ops.pn2.mlp_layer_train: conv + bias + batch-statistics batch norm + ReLU, with
    autograd for x and every variable), for the variables of a trainable ParamStore. The moving
    averages are updated in place on the device by mlp_torch's rule: decay bn_decay (0.9 when
    None) with the biased batch variance.

    pool="max": x is (..., ns, cin) and the last layer runs fused with the max over the ns
    axis (torch.ops.pn2.mlp_layer_train_pool): the result, (..., cout), has the bits of
    mlp_train(x, layers).max(dim=-2).values, and neither the last activation nor its gradient is
    materialised.

    precision: "fp32", "bf16" (the layers' GEMMs on the bf16 matrix cores:
    torch.ops.pn2.mlp_layer_train_bf16 / _pool_bf16; see the module docstring) or None: each
    layer's own train_precision, which torch_layers takes from the store."""
    if precision is not None:
        check_precision(precision)
    if pool not in (None, "max"):
        raise InvalidArgumentError(f"mlp_train fuses max pooling only, got pool={pool!r}")
    if pool and not layers:
        raise InvalidArgumentError("mlp_train: pool needs at least one layer")
    decay = 0.9 if bn_decay is None else float(bn_decay)
    x = device_tensor(x, "inputs", torch.float32)
    for i, L in enumerate(layers):
        p = L.params
        bn = p.get("gamma") is not None
        rows = x.numel()
        op = "mlp_layer_train_pool" if pool and i == len(layers) - 1 else "mlp_layer_train"
        if (precision or getattr(L, "train_precision", "fp32")) == "bf16":
            op += "_bf16"
        x, _, mean, var = _torch_ops.call(
            op, x, p["weights"], p.get("biases"), p.get("gamma") if bn else None,
            p.get("beta") if bn else None, BN_EPSILON, bool(L.relu))[:4]
        if bn and rows > 0:  # no rows: no batch statistics, the moving averages stay
            with torch.no_grad():
                p["moving_mean"].mul_(decay).add_((1 - decay) * mean)
                p["moving_variance"].mul_(decay).add_((1 - decay) * var)
    return x


def bn_train(x, params, bn_decay=None, relu=False):
    """Batch-statistics batch norm of x (..., C) on its own (tf_util.py:512-531 with
    is_training=True; the batch norm after the attention, attention_layer.py:261) on the HIP
    training kernels (torch.ops.pn2.bn_train, autograd for x, gamma and beta), for the variables
    `params` = store.bn(scope, C) of a trainable ParamStore. The moving averages are updated in
    place on the device by mlp_train's rule: decay bn_decay (0.9 when None), biased batch
    variance, no update when x has no rows."""
    decay = 0.9 if bn_decay is None else float(bn_decay)
    x = device_tensor(x, "inputs", torch.float32)
    out, mean, var = _torch_ops.call("bn_train", x, params["gamma"], params["beta"], BN_EPSILON,
                                     bool(relu))
    if x.numel() > 0:
        with torch.no_grad():
            params["moving_mean"].mul_(decay).add_((1 - decay) * mean)
            params["moving_variance"].mul_(decay).add_((1 - decay) * var)
    return out


def dropout(inputs, is_training, scope, keep_prob=0.5, noise_shape=None, seed=None):
    """tf_util.dropout (tf_util.py:594-612) on the HIP kernel (torch.ops.pn2.dropout,
    csrc/head_train.hip): with is_training, inputs / keep_prob where the mask keeps an element, 0
    elsewhere; without it, `inputs` itself. The mask is Philox4x32-10 of (seed, element index),
    so no mask tensor is kept and autograd applies the same op to the gradient. Extra keyword
    `seed`: a Python int; None draws one from torch's default CPU generator (so
    torch.manual_seed makes a run reproducible, and nothing touches the device). It creates no
    variables, so it takes no store; `scope` is the reference's name scope only."""
    if noise_shape is not None:
        raise NotImplementedError("dropout: noise_shape is not supported (the reference never "
                                  "passes one)")
    if not is_training:
        return inputs
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, ()))
    return _torch_ops.call("dropout", device_tensor(inputs, "inputs", torch.float32),
                           float(keep_prob), int(seed))


def sparse_softmax_cross_entropy(labels, logits, weights=1.0):
    """tf.losses.sparse_softmax_cross_entropy(labels, logits, weights) with its default reduction
    SUM_BY_NONZERO_WEIGHTS (the loss of pointnet2_sem_seg.get_loss): sum of weights * (logsumexp
    (logits) - logits[label]) over the number of non-zero weights, 0 when there is none. logits
    (..., C) float32, labels (...) integer, weights a Python scalar or a float32 tensor of the
    labels' shape. One HIP kernel pass each way (torch.ops.pn2.softmax_xent); the gradient flows
    to the logits only."""
    logits = device_tensor(logits, "logits", torch.float32)
    if isinstance(labels, torch.Tensor) and labels.dtype in (torch.int64, torch.int16,
                                                             torch.uint8, torch.int8):
        labels = labels.to(torch.int32)
    labels = device_tensor(labels, "labels", torch.int32)
    if isinstance(weights, torch.Tensor) and weights.dim() > 0:
        return _torch_ops.call("softmax_xent", logits, labels,
                               device_tensor(weights, "weights", torch.float32))[0]
    w = float(weights)
    loss = _torch_ops.call("softmax_xent", logits, labels, None)[0]
    # a scalar w weights every row alike: w * the mean, and no row is present at w = 0
    return torch.zeros_like(loss) if w == 0.0 else loss * w


class TorchLayer:
    """A conv layer's raw variables for mlp_torch and mlp_train; train_precision: of the HIP
    training layer mlp_train runs for it."""

    def __init__(self, params, relu=True, train_precision="fp32"):
        self.params, self.relu = params, relu
        self.train_precision = check_precision(train_precision)


def torch_layers(store, scopes, cin, widths, bn=True, relu=True):
    layers, c = [], cin
    for scope, w in zip(scopes, widths):
        layers.append(TorchLayer(store.conv(scope, c, w, bn=bn), relu=relu,
                                 train_precision=store.train_precision))
        c = w
    return layers
