"""Per-group attention reduction of attention_points/attention_scannet/attention_layer.py.

attention_reduce is the reduction core of AttentionLayer.call (:35-42) as one gfx950 kernel.
AttentionLayer mirrors the reference layer (:10-45): its Dense query/key/value projections
(:24-26) are plain torch Linear layers (dense contractions are outside the hot path), the
reduction is the kernel. The SA attention modules instantiate it with key_dim = output_dim = 4
and num_heads = C/4 (:256-258, :313-315): csrc/attn.hip. The attention networks (:128-210,
pooling_attention_layer.py) instantiate it with key_dim = output_dim = out_dim, 8 to 512, and 16
heads: csrc/attn_net.hip, which also holds the head mixing of InnerAttentionLayer (:48-78). The
networks' layers are at the end of this module.
"""
import ctypes
import functools

import torch

from . import pointnet_util, tf_grouping, tf_sampling, tf_util
from ._lib import (PN2_ATTN_MAX_LAYERS, PN2_MLP_MAX_LAYERS, AttnLayer, InvalidArgumentError,
                   MlpLayer, aligned_device_tensor, check, device_tensor, lib, ptr, stream_of)
from ._torch_ops import call


def attention_reduce(Q, K, V, key_dim=4):
    """Q (B,M,C), K,V (B,M,ns,C) -> (B,M,C), C = key_dim*heads.

    Per group and head h, with kd = key_dim: K_h = the contiguous block [kd*ns*h, kd*ns*(h+1)) of
    the group's flattened K (the tf.reshape reinterpretation of :35-36), s = K_h q_h / sqrt(kd)
    (:37-38), a = softmax(s) (:39), out[kd*h : kd*(h+1)] = a^T V_h (:40-42). key_dim = 4 (the SA
    attention modules) is torch.ops.pn2.attn_reduce; any other multiple of 4 up to 512 (the
    attention networks, key_dim = out_dim) is torch.ops.pn2.attn_reduce_kd (csrc/attn_net.hip).
    """
    if Q.dim() == 4 and Q.shape[2] == 1:  # the reference's (B,M,1,C) query vectors (:259)
        Q = Q.squeeze(2)
    if Q.dim() != 3 or K.dim() != 4 or tuple(V.shape) != tuple(K.shape):
        raise InvalidArgumentError("attention_reduce expects Q (B,M,C), K and V (B,M,ns,C)")
    B, M, ns, C = (int(s) for s in K.shape)
    key_dim = int(key_dim)
    if key_dim < 4 or key_dim > 512 or key_dim % 4 != 0:
        raise InvalidArgumentError("attention_reduce expects key_dim % 4 == 0, 4 <= key_dim <= 512")
    if tuple(Q.shape) != (B, M, C) or C % key_dim != 0:
        raise InvalidArgumentError("attention_reduce expects Q (B,M,C) with C a multiple of "
                                   f"{key_dim}")
    tensors = (device_tensor(Q, "Q", torch.float32), device_tensor(K, "K", torch.float32),
               device_tensor(V, "V", torch.float32))
    # torch.ops.pn2.attn_reduce (autograd: pn2_attn_reduce_grad, _torch_ops.py)
    if key_dim == 4:
        return call("attn_reduce", *tensors)
    return call("attn_reduce_kd", *tensors, key_dim)


def attention_reduce_layers(qkvs):
    """attention_reduce of several layers that share nsample (the SSG stack's four SA layers)
    in ONE launch (pn2_attn_reduce_layers): qkvs = [(Q, K, V)], returns [out] per layer,
    each exactly attention_reduce(Q, K, V) (an nsample outside {8, 16, 32, 64, 128}, or a layer
    too large for the one-launch task arithmetic, runs as attention_reduce runs it). All layers
    share one nsample. Inference only (no autograd)."""
    if not 1 <= len(qkvs) <= PN2_ATTN_MAX_LAYERS:
        raise InvalidArgumentError(f"attention_reduce_layers: 1..{PN2_ATTN_MAX_LAYERS} layers")
    arr = (AttnLayer * len(qkvs))()
    outs, keep, B, ns = [], [], None, None
    for i, (Q, K, V) in enumerate(qkvs):
        if Q.dim() == 4 and Q.shape[2] == 1:
            Q = Q.squeeze(2)
        Q = aligned_device_tensor(Q, "Q", torch.float32)
        K = aligned_device_tensor(K, "K", torch.float32)
        V = aligned_device_tensor(V, "V", torch.float32)
        if Q.dim() != 3 or K.dim() != 4 or tuple(V.shape) != tuple(K.shape):
            raise InvalidArgumentError("attention_reduce_layers expects Q (B,M,C), K and V "
                                       "(B,M,ns,C)")
        b, M, n, C = (int(s) for s in K.shape)
        if tuple(Q.shape) != (b, M, C) or C % 4 != 0 or (B is not None and (b, n) != (B, ns)):
            raise InvalidArgumentError("attention_reduce_layers: Q (B,M,C), C % 4 == 0, one B "
                                       "and one nsample for all layers")
        B, ns = b, n
        out = torch.empty((B, M, C), dtype=torch.float32, device=Q.device)
        arr[i] = AttnLayer(Q.data_ptr(), K.data_ptr(), V.data_ptr(), M, n, C, out.data_ptr())
        outs.append(out)
        keep += [Q, K, V]
    check(lib().pn2_attn_reduce_layers(ctypes.addressof(arr), len(qkvs), B,
                                       stream_of(outs[0])), "attention_reduce_layers")
    return outs


def attention_reduce_grad(Q, K, V, grad_out):
    """(dQ, dK, dV) of attention_reduce for the incoming gradient grad_out (B,M,C): the
    gradient TF's autodiff takes through attention_layer.py:35-42 (pn2_attn_reduce_grad)."""
    return tuple(call("attn_reduce_grad", device_tensor(Q, "Q", torch.float32),
                                        device_tensor(K, "K", torch.float32),
                                        device_tensor(V, "V", torch.float32),
                                        device_tensor(grad_out, "grad_out", torch.float32)))


class AttentionLayer(torch.nn.Module):
    """attention_layer.py:10-45 with output_dim = key_dim: 4 in the SA attention modules
    (:256-258, :313-315), out_dim = 8 .. 512 with the default 16 heads in the attention networks
    (:142, :185, pooling_attention_layer.py:17).

    forward([input, query]): input (B,M,ns,in_dim), query (B,M,1,query_dim) or (B,M,query_dim)
    -> (B,M,num_heads*key_dim). in_dim defaults to num_heads*key_dim, query_dim to in_dim (the
    pooling layer's query is new_xyz: query_dim = 3).
    """

    def __init__(self, output_dim, key_dim, num_heads=16, in_dim=None, query_dim=None):
        super().__init__()
        if output_dim != key_dim:
            # (:35-36) reshapes V, whose width is output_dim * num_heads, with key_dim: the
            # reference's own graph is ill-formed unless the two agree
            raise NotImplementedError(
                f"AttentionLayer(output_dim={output_dim}, key_dim={key_dim}): the reference "
                "reshapes the values with key_dim, so it is defined for output_dim == key_dim only")
        if key_dim < 4 or key_dim > 512 or key_dim % 4 != 0:
            raise NotImplementedError("AttentionLayer runs key_dim % 4 == 0, 4 <= key_dim <= 512 "
                                      f"(float4 rows in csrc/attn_net.hip), got {key_dim}")
        self.output_dim, self.key_dim, self.num_heads = output_dim, key_dim, num_heads
        width = key_dim * num_heads
        in_dim = in_dim if in_dim is not None else width
        query_dim = query_dim if query_dim is not None else in_dim
        self.query_net = torch.nn.Linear(query_dim, width)  # tf.layers.Dense (:24)
        self.key_net = torch.nn.Linear(in_dim, width)       # (:25)
        self.value_net = torch.nn.Linear(in_dim, width)     # (:26)

    def forward(self, inputs):
        x, query = inputs
        Q = self.query_net(query)
        K = self.key_net(x).contiguous()
        V = self.value_net(x).contiguous()
        return attention_reduce(Q.reshape(Q.shape[0], Q.shape[1], -1).contiguous(), K, V,
                                self.key_dim)


def _attention_scopes(scope):
    # tf.layers.Dense names inside the Keras layer, in build order (:24-26)
    base = f"{scope}/ScannetAttentionLayer"
    return f"{base}/dense", f"{base}/dense_1", f"{base}/dense_2"


def pointnet_sa_module_attention(xyz, points, npoint, radius, nsample, mlp, mlp2, group_all,
                                 is_training, bn_decay, scope, bn=True, pooling='max', knn=False,
                                 use_xyz=True, use_nchw=False, params=None, and_pooling=False):
    """attention_layer.py:229-276 (and_pooling=True: :279-338, attention + max pool).

    Returns (new_xyz, new_points (B, npoint, mlp[-1] or mlp2[-1]), idx). Variables:
    '<scope>/conv<i>/...' (the MLP), '<scope>/ScannetAttentionLayer/dense{,_1,_2}/{kernel,bias}'
    (query, key, value), '<scope>/<scope>/{gamma,beta,moving_mean,moving_variance}' (the batch
    norm after the attention, :261), '<scope>/conv_post_<i>/...' (mlp2).

    is_training=True on a trainable store (ParamStore.trainable()) runs the HIP training layers:
    tf_util.mlp_train for the MLP and mlp2, attention_train for the AttentionLayer, its batch
    norm and the pool, with gradients for every variable. On a plain store is_training=True (or
    inputs that require a gradient) runs the differentiable torch composition."""
    store = params if params is not None else tf_util.default_store()
    pu = pointnet_util
    xyz = device_tensor(xyz, "xyz", torch.float32)
    C = int(mlp[-1])
    if C % 4:
        raise InvalidArgumentError("attention SA needs mlp[-1] % 4 == 0 (heads of 4)")
    scopes = [f"{scope}/conv{i}" for i in range(len(mlp))]
    qs, ks, vs = _attention_scopes(scope)
    empty = pu._is_empty_points(points)
    cin = (0 if empty else int(points.shape[2])) + (3 if (use_xyz or empty) else 0)
    training = is_training or pu._needs_grad(xyz, points)
    if group_all:
        new_xyz, grouped, idx, _ = pu.sample_and_group_all(xyz, points, use_xyz)
    elif training or knn:
        new_xyz, grouped, idx, _ = pu.sample_and_group(npoint, radius, nsample, xyz, points, knn,
                                                       use_xyz)
    else:
        _, new_xyz = tf_sampling.farthest_point_sample_and_gather(npoint, xyz)
        idx, _ = tf_grouping.query_ball_point(radius, nsample, xyz, new_xyz)
    # is_training on a trainable store: the HIP training layers, gradients for every variable
    hip_train = bool(is_training) and store.is_trainable
    if hip_train:
        X = tf_util.mlp_train(grouped, tf_util.torch_layers(store, scopes, cin, mlp, bn=bn),
                              bn_decay)
        out = attention_train(X, store, scope, C, bn_decay, and_pooling)
    elif training:
        X = tf_util.mlp_torch(grouped, tf_util.torch_layers(store, scopes, cin, mlp, bn=bn),
                              is_training, bn_decay)
        dense = lambda sc, x: x @ store.dense(sc, C, C)["weights"].to(x.device) + \
            store.dense(sc, C, C)["biases"].to(x.device)  # noqa: E731
        Q = dense(qs, X[:, :, 0])
        out = attention_reduce(Q.contiguous(), dense(ks, X).contiguous(), dense(vs, X).contiguous())
        p = store.bn(f"{scope}/{scope}", C)
        layer = tf_util.TorchLayer({"weights": torch.eye(C), "biases": None, **p}, relu=False)
        out = tf_util.mlp_torch(out, [layer], is_training, bn_decay)
        if and_pooling:
            out = out + X.max(dim=2).values
    else:
        fused = tf_util.packed_mlp(store, scopes, cin, mlp, bn=bn)
        out = group_mlp_attention(xyz, points, new_xyz, idx, fused, store, scope, and_pooling,
                                  use_xyz=use_xyz)
    if mlp2:
        post = [f"{scope}/conv_post_{i}" for i in range(len(mlp2))]
        if hip_train:
            out = tf_util.mlp_train(out, tf_util.torch_layers(store, post, C, mlp2, bn=bn),
                                    bn_decay)
        elif training:
            out = tf_util.mlp_torch(out, tf_util.torch_layers(store, post, C, mlp2, bn=bn),
                                    is_training, bn_decay)
        else:
            out = tf_util.packed_mlp(store, post, C, mlp2, bn=bn)(out)
    return new_xyz, out, idx


def attention_train(X, store, scope, C, bn_decay=None, and_pooling=False):
    """Training tail of the attention SA layers on the per-point MLP output X (B,M,ns,C), for a
    trainable store: torch.ops.pn2.attn_kv_train (the Dense query of each group's first
    neighbour, :259; key and value projected together in one GEMM; the reduction; with
    and_pooling the max over ns, :303), then the batch-statistics batch norm '<scope>/<scope>'
    (:261, tf_util.bn_train) and + the max. Autograd reaches X and all eight variables."""
    q, k, v = (store.dense(s, C, C) for s in _attention_scopes(scope))
    att, pmax = call("attn_kv_train", device_tensor(X, "X", torch.float32), q["weights"],
                     q["biases"], k["weights"], k["biases"], v["weights"], v["biases"],
                     bool(and_pooling))[:2]
    out = tf_util.bn_train(att, store.bn(f"{scope}/{scope}", C), bn_decay)
    return out + pmax if and_pooling else out


def group_mlp_attention(xyz, points, new_xyz, idx, mlp, store, scope, and_pooling=False,
                        use_xyz=True):
    """The whole inference SA-attention layer after sampling and ball query in ONE kernel
    (pn2_group_mlp_attention): group + MLP `mlp`, Dense q/k/v, the reduction per head, the
    batch norm '<scope>/<scope>' and (and_pooling) + max pool; the per-point features never
    leave the chip. -> (B, M, C)."""
    pu = pointnet_util
    xyz = device_tensor(xyz, "xyz", torch.float32)
    new_xyz = device_tensor(new_xyz, "new_xyz", torch.float32)
    idx = device_tensor(idx, "idx", torch.int32)
    B, N = int(xyz.shape[0]), int(xyz.shape[1])
    M, ns = int(idx.shape[1]), int(idx.shape[2])
    if pu._is_empty_points(points):
        points, Cin = None, 0
    else:
        points = device_tensor(points, "points", torch.float32)
        Cin = int(points.shape[2])
    C = mlp.cout
    # the query Dense is VALU work on the fp32 layout: fp32 whatever the store's precision
    qs, ks, vs = _attention_scopes(scope)
    qkv = [tf_util.packed_dense(store, qs, C, C, precision="fp32"),
           tf_util.packed_dense(store, ks, C, C), tf_util.packed_dense(store, vs, C, C)]
    table = (type(mlp.table()[0][0]) * 3)(*[d.layers[0].struct() for d in qkv])
    scale, shift = tf_util.bn_affine(store, f"{scope}/{scope}", C, xyz.device)
    out = torch.empty((B, M, C), dtype=torch.float32, device=xyz.device)
    flags = pu.PN2_USE_XYZ if use_xyz else 0
    tab, n = mlp.table()
    check(lib().pn2_group_mlp_attention(ptr(xyz), ptr(points), ptr(new_xyz), ptr(idx), B, N, Cin,
                                        M, ns, flags, n, tab, table, ptr(scale), ptr(shift),
                                        1 if and_pooling else 0, ptr(out), stream_of(xyz)),
          "group_mlp_attention")
    return out


def sa_attention_tail(X, store, scope, C, and_pooling=False):
    """Inference tail of the attention SA layers on the per-point MLP output X (B,M,ns,C):
    the Dense query (first neighbour, :259), key and value projections on the matrix cores,
    the reduction kernel, the batch norm (:261) and, for _and_pooling, + max over ns (:303)."""
    qs, ks, vs = _attention_scopes(scope)
    K = tf_util.packed_dense(store, ks, C, C)(X)
    V = tf_util.packed_dense(store, vs, C, C)(X)
    Q = tf_util.packed_dense(store, qs, C, C, precision="fp32")(X[:, :, 0].contiguous())
    out = attention_reduce(Q, K, V)
    scale, shift = tf_util.bn_affine(store, f"{scope}/{scope}", C, X.device)
    out = out * scale + shift
    if and_pooling:  # pooling='max' only (:296-299)
        out = out + pointnet_util.group_pool(X, "max").squeeze(2)
    return out


def pointnet_sa_module_attention_and_pooling(xyz, points, npoint, radius, nsample, mlp, mlp2,
                                             group_all, is_training, bn_decay, scope, bn=True,
                                             pooling='max', knn=False, use_xyz=True,
                                             use_nchw=False, params=None):
    """attention_layer.py:279-338: attention output (after its batch norm) + max pool."""
    if pooling != 'max':
        raise ValueError("Pooling must be max for this implementation")
    return pointnet_sa_module_attention(xyz, points, npoint, radius, nsample, mlp, mlp2,
                                        group_all, is_training, bn_decay, scope, bn, pooling, knn,
                                        use_xyz, use_nchw, params, and_pooling=True)


# ------------------------------------------------------------------ the attention networks
# attention_points/attention_scannet/attention_layer.py:48-210: InnerAttentionLayer,
# FeedForwardLayer, InnerAttentionBlock, AttentionNetLayer, AttentionNetMLPLayer, store-based under
# the reference's names and constructor arguments. Every class takes `scope=` (its variables are
# '<scope>/...', hierarchical: INTEGRATION.md has the table and the TF1 `dense_<n>` order) and
# `params=` (the ParamStore; default tf_util.default_store()). Calling a layer takes
# is_training (None: the constructor's): on a trainable store it selects the HIP training layers.

@functools.lru_cache(maxsize=None)
def plan_accepts(cin, widths):
    """Whether the fused MLP kernel takes a chain cin -> widths (pn2_shared_mlp_plan: host only,
    the packed pointers are checked for alignment and never read). It refuses when a layer's
    input row does not fit the LDS: 1027 input channels fit, 1280 do not."""
    if not 1 <= len(widths) <= PN2_MLP_MAX_LAYERS:
        return False
    tab, c = (MlpLayer * len(widths))(), int(cin)
    for i, w in enumerate(widths):
        tab[i] = MlpLayer(1 << 20, c, int(w), 0)
        c = int(w)
    R, tpw = ctypes.c_int(0), ctypes.c_int(0)
    return lib().pn2_shared_mlp_plan(32, int(cin), len(widths), tab, ctypes.addressof(R),
                                     ctypes.addressof(tpw)) == 0


@functools.lru_cache(maxsize=None)
def wide_accepts(cin, cout):
    """Whether the K-streamed kernel takes a layer cin -> cout (pn2_dense_wide_plan: host only).
    It takes every positive width; the grid bounds cout at 32 * 8 * 65,535."""
    tab = (MlpLayer * 1)(MlpLayer(1 << 20, int(cin), int(cout), 0))
    out = [ctypes.c_int(0) for _ in range(3)]
    return lib().pn2_dense_wide_plan(32, int(cin), tab, *(ctypes.addressof(o) for o in out)) == 0


def _layer_torch(x, L, is_training, bn_decay):
    """One layer from differentiable torch ops (mlp_torch's arithmetic; the moving averages are
    updated where they live): what a layer the fused kernel refuses runs on with
    ParamStore(wide_layers="torch"), and with is_training on a plain store."""
    p = L.params
    y = x @ p["weights"].to(x.device)
    if p.get("biases") is not None:
        y = y + p["biases"].to(x.device)
    if p.get("gamma") is not None:
        if is_training:
            dims = tuple(range(y.dim() - 1))
            mean, var = y.mean(dim=dims), y.var(dim=dims, unbiased=False)
            decay = 0.9 if bn_decay is None else float(bn_decay)
            with torch.no_grad():
                for name, stat in (("moving_mean", mean), ("moving_variance", var)):
                    p[name].mul_(decay).add_((1 - decay) * stat.detach().to(p[name].device))
        else:
            mean, var = p["moving_mean"].to(x.device), p["moving_variance"].to(x.device)
        y = (y - mean) * (p["gamma"].to(x.device) / torch.sqrt(var + tf_util.BN_EPSILON)) + \
            p["beta"].to(x.device)
    return torch.relu(y) if L.relu else y


def _flat(scopes):
    return [s for sc in scopes for s in ((sc,) if isinstance(sc, str) else sc)]


def _packed_chain(store, layers, scopes):
    """SharedMLP of `layers` (tf_util.TorchLayer: Dense, or conv with batch norm), cached in the
    store under the variables' scopes (an entry of `scopes` may be a tuple: one layer over
    several Dense layers' variables side by side)."""
    shape = tuple((tuple(L.params["weights"].shape), L.relu, "gamma" in L.params) for L in layers)
    key = ("chain", tuple(_flat(scopes)), shape, store.precision)

    def make():
        return tf_util.SharedMLP([
            tf_util.PackedLayer(L.params["weights"], L.params.get("biases"), L.params.get("gamma"),
                                L.params.get("beta"), L.params.get("moving_mean"),
                                L.params.get("moving_variance"), relu=L.relu, device=store.device,
                                precision=store.precision) for L in layers])

    return store.cached(key, _flat(scopes), tf_util.CONV_SUFFIXES + tf_util.DENSE_SUFFIXES, make)


def _packed_wide(store, L, scope):
    """One layer (tf_util.TorchLayer) that the fused kernel refuses, packed for the K-streamed
    kernel (tf_util.WideLayer) and cached as _packed_chain caches: fp32 whatever the store's
    precision is (the kernel has no bf16 form)."""
    key = ("wide", tuple(_flat([scope])), tuple(L.params["weights"].shape), L.relu,
           "gamma" in L.params)

    def make():
        return tf_util.WideLayer(tf_util.PackedLayer(
            L.params["weights"], L.params.get("biases"), L.params.get("gamma"),
            L.params.get("beta"), L.params.get("moving_mean"), L.params.get("moving_variance"),
            relu=L.relu, device=store.device, precision="fp32"))

    return store.cached(key, _flat([scope]), tf_util.CONV_SUFFIXES + tf_util.DENSE_SUFFIXES, make)


def run_layers(store, x, layers, scopes, is_training=False, bn_decay=None):
    """x (..., cin) through `layers` (tf_util.TorchLayer each, with the scope(s) of its variables
    in `scopes`). Inference: ONE fused kernel for the chain (tf_util.SharedMLP) when
    pn2_shared_mlp_plan accepts it, else layer by layer: a layer the fused kernel refuses (its
    input row does not fit the LDS) runs on the K-streamed kernel (tf_util.WideLayer over
    pn2_dense_wide, fp32). is_training on a trainable store: the HIP training layers
    (tf_util.mlp_train; Dense layers have no batch norm), with gradients for x and every
    variable; a layer that the fused kernel refuses, or whose transpose it refuses (the input
    gradient is a layer over W^T), trains in fp32 there, its GEMMs on the K-streamed kernel.
    Otherwise (is_training on a plain store, or an input that requires a gradient) the torch
    composition. With ParamStore(wide_layers="torch") the refused layers run from torch ops
    (_layer_torch) instead, as they did before the K-streamed kernel existed."""
    pu = pointnet_util
    shapes = [tuple(int(s) for s in L.params["weights"].shape) for L in layers]
    wide_hip = store.wide_layers == "hip"
    if is_training or pu._needs_grad(x):
        hip = bool(is_training) and store.is_trainable
        for L, (cin, cout) in zip(layers, shapes):
            if hip and plan_accepts(cin, (cout,)) and plan_accepts(cout, (cin,)):
                x = tf_util.mlp_train(x, [L], bn_decay)
            elif hip and wide_hip and wide_accepts(cin, cout) and wide_accepts(cout, cin):
                x = tf_util.mlp_train(x, [L], bn_decay, precision="fp32")
            else:
                x = _layer_torch(x, L, is_training, bn_decay)
        return x
    if plan_accepts(shapes[0][0], tuple(s[1] for s in shapes)):
        return _packed_chain(store, layers, scopes)(x)
    with torch.no_grad():
        for L, sc, (cin, cout) in zip(layers, scopes, shapes):
            if plan_accepts(cin, (cout,)):
                x = _packed_chain(store, [L], [sc])(x)
            elif wide_hip and wide_accepts(cin, cout):
                x = _packed_wide(store, L, sc)(x)
            else:
                x = _layer_torch(device_tensor(x, "inputs", torch.float32),
                                 _device_layer(store, L, sc), False, None)
    return x


def _device_layer(store, L, scope):
    """L with its variables by value on the store's device, cached like a packed layer (a plain
    store keeps its variables on the host)."""
    key = ("torch", tuple(_flat([scope])), tuple(L.params["weights"].shape), L.relu)

    def make():
        return tf_util.TorchLayer({k: v.detach().to(store.device) for k, v in L.params.items()
                                   if v is not None}, relu=L.relu)

    return store.cached(key, _flat([scope]), tf_util.CONV_SUFFIXES + tf_util.DENSE_SUFFIXES, make)


def _dense_layer(store, scopes, cin, cout, relu=False):
    """One tf_util.TorchLayer over one Dense layer's variables, or over several Dense layers of
    one input side by side ([W_a | W_b | ...]: one GEMM)."""
    if isinstance(scopes, str):
        return tf_util.TorchLayer(store.dense(scopes, cin, cout), relu=relu,
                                  train_precision=store.train_precision)
    ps = [store.dense(s, cin, cout) for s in scopes]
    dev = ps[0]["weights"].device
    return tf_util.TorchLayer({"weights": torch.cat([p["weights"].to(dev) for p in ps], dim=1),
                               "biases": torch.cat([p["biases"].to(dev) for p in ps])},
                              relu=relu, train_precision=store.train_precision)


def _store(params):
    return params if params is not None else tf_util.default_store()


def group_attention(store, scope, x, query, key_dim, num_heads=16, is_training=False):
    """AttentionLayer.call (:29-45) on the store's variables '<scope>/{query,key,value}/
    {kernel,bias}': x (B,M,ns,cin), query (B,M,cq) -> (B,M,num_heads*key_dim). Three Dense layers
    (run_layers), then attention_reduce with key_dim."""
    C = int(key_dim) * int(num_heads)
    q, k, v = (f"{scope}/{n}" for n in ("query", "key", "value"))
    cin, cq = int(x.shape[-1]), int(query.shape[-1])
    Q = run_layers(store, query.contiguous(), [_dense_layer(store, q, cq, C)], [q], is_training)
    K = run_layers(store, x, [_dense_layer(store, k, cin, C)], [k], is_training)
    V = run_layers(store, x, [_dense_layer(store, v, cin, C)], [v], is_training)
    return attention_reduce(Q, K, V, key_dim)


class InnerAttentionLayer:
    """attention_layer.py:48-78: attention among the 5 heads of ONE point (it never looks across
    the group): Dense query | key | value of width 5*key_dim in one GEMM, torch.ops.pn2.head_mix,
    then the Dense `out` to output_dim. Variables '<scope>/{query,key,value,out}/{kernel,bias}'."""
    num_heads = 5

    def __init__(self, output_dim, key_dim, scope="ScannetInnerAttentionLayer", params=None):
        if key_dim % 4 or not 4 <= key_dim <= 256:
            raise NotImplementedError("InnerAttentionLayer runs key_dim % 4 == 0, 4 <= key_dim <= "
                                      f"256 (csrc/attn_net.hip), got {key_dim}")
        self.output_dim, self.key_dim, self.scope, self.params = output_dim, key_dim, scope, params

    def __call__(self, x, is_training=False):
        store, H, kd = _store(self.params), self.num_heads, self.key_dim
        qkv = tuple(f"{self.scope}/{n}" for n in ("query", "key", "value"))
        y = run_layers(store, x, [_dense_layer(store, qkv, int(x.shape[-1]), H * kd)], [qkv],
                       is_training)
        y = call("head_mix", y, H, kd)
        out = f"{self.scope}/out"
        return run_layers(store, y, [_dense_layer(store, out, H * kd, self.output_dim)], [out],
                          is_training)


class FeedForwardLayer:
    """attention_layer.py:81-105: Dense + ReLU three times (width inner_dim), then a Dense to
    input_and_output_dim: one four-layer chain. The reference's dropout has rate 0. Variables
    '<scope>/layer_{1..4}/{kernel,bias}'. relu_out: a ReLU on the result (AttentionNetMLPLayer
    puts one between its blocks), folded into the last layer."""

    def __init__(self, input_and_output_dim, inner_dim, dropout=0,
                 scope="ScannetFeedForwardLayer", params=None):
        if dropout:
            raise NotImplementedError("FeedForwardLayer: the reference only builds it with "
                                      "dropout = 0")
        self.input_and_output_dim, self.inner_dim = input_and_output_dim, inner_dim
        self.dropout, self.scope, self.params = dropout, scope, params

    def __call__(self, x, is_training=False, relu_out=False):
        store = _store(self.params)
        widths = [self.inner_dim] * 3 + [self.input_and_output_dim]
        scopes = [f"{self.scope}/layer_{i}" for i in (1, 2, 3, 4)]
        layers, c = [], int(x.shape[-1])
        for i, (sc, w) in enumerate(zip(scopes, widths)):
            layers.append(_dense_layer(store, sc, c, w, relu=i < 3 or relu_out))
            c = w
        return run_layers(store, x, layers, scopes, is_training)


class InnerAttentionBlock:
    """attention_layer.py:108-125: p = pre_feed_forward(x); p = inner attention(p);
    feed_forward(p) + p. Variables under '<scope>/{pre_feed_forward,inner_attention,
    feed_forward}/'."""

    def __init__(self, out_dim, key_dim, scope="ScannetInnerAttentionBlock", params=None):
        self.out_dim, self.key_dim, self.scope, self.params = out_dim, key_dim, scope, params
        self.attention_layer = InnerAttentionLayer(out_dim, key_dim,
                                                   scope=f"{scope}/inner_attention", params=params)
        self.feed_forward_layer = FeedForwardLayer(out_dim, out_dim,
                                                   scope=f"{scope}/feed_forward", params=params)
        self.pre_feed_forward_layer = FeedForwardLayer(
            out_dim, out_dim, scope=f"{scope}/pre_feed_forward", params=params)

    def __call__(self, x, is_training=False):
        if isinstance(x, (list, tuple)):  # the reference passes a one-element list (:159)
            x, = x
        p = self.pre_feed_forward_layer(x, is_training)
        p = self.attention_layer(p, is_training)
        return self.feed_forward_layer(p, is_training) + p


class _AttentionNetBase:
    """sample_and_group (knn=False, use_xyz=True), the subclass's per-point blocks, then the
    group attention with the group's first neighbour as the query (:166-167, :208-209)."""

    def __init__(self, npoint, out_dim, inner_dimensions, is_training=True, radius=0.1, nsample=32,
                 bn=True, scope=None, params=None):
        if out_dim % 4 or not 4 <= out_dim <= 512:
            raise NotImplementedError(f"{type(self).__name__} runs out_dim % 4 == 0, 4 <= out_dim "
                                      f"<= 512 (key_dim = out_dim), got {out_dim}")
        self.npoint, self.radius, self.nsample = npoint, radius, nsample
        self.out_dim, self.key_dim, self.inner_dimensions = out_dim, out_dim, list(inner_dimensions)
        self.is_training, self.bn = is_training, bn
        self.scope = scope if scope is not None else type(self).__name__
        self.params = params

    def __call__(self, inputs, is_training=None):
        xyz, points = inputs
        training = self.is_training if is_training is None else is_training
        if pointnet_util._is_empty_points(points):
            points = None
        new_xyz, x, idx, _ = pointnet_util.sample_and_group(self.npoint, self.radius, self.nsample,
                                                           xyz, points, False, True)
        x = self.blocks(x, training)
        out = group_attention(_store(self.params), f"{self.scope}/attention", x,
                              x[:, :, 0], self.key_dim, 16, training)
        return [new_xyz, out, idx]


class AttentionNetLayer(_AttentionNetBase):
    """attention_layer.py:128-168. [xyz, points] -> [new_xyz, new_points (B, npoint, 16*out_dim),
    idx]. Variables: '<scope>/block_<i>/...' (InnerAttentionBlock(inner_dimensions[i], out_dim))
    and '<scope>/attention/{query,key,value}/{kernel,bias}'. The last inner dimension feeds the
    attention's Dense layers, so any value works."""

    def __init__(self, npoint, out_dim, inner_dimensions, is_training=True, radius=0.1, nsample=32,
                 bn=True, scope=None, params=None):
        super().__init__(npoint, out_dim, inner_dimensions, is_training, radius, nsample, bn,
                         scope, params)
        self.inner_blocks = [InnerAttentionBlock(d, self.key_dim, scope=f"{self.scope}/block_{i}",
                                                 params=params)
                             for i, d in enumerate(self.inner_dimensions)]

    def blocks(self, x, training):
        for block in self.inner_blocks:
            x = block(x, training)
        return x


class AttentionNetMLPLayer(_AttentionNetBase):
    """attention_layer.py:171-210: feed-forward blocks FeedForwardLayer(d, d) with a ReLU between
    them and none after the last, then the attention. Variables '<scope>/feed_forward_<i>/
    layer_{1..4}/...' and '<scope>/attention/...'."""

    def __init__(self, npoint, out_dim, inner_dimensions, is_training=True, radius=0.1, nsample=32,
                 bn=True, scope=None, params=None):
        super().__init__(npoint, out_dim, inner_dimensions, is_training, radius, nsample, bn,
                         scope, params)
        if not self.inner_dimensions:
            raise InvalidArgumentError("AttentionNetMLPLayer needs at least one inner dimension")
        self.inner_blocks = [FeedForwardLayer(d, d, scope=f"{self.scope}/feed_forward_{i}",
                                              params=params)
                             for i, d in enumerate(self.inner_dimensions)]

    def blocks(self, x, training):
        for i, block in enumerate(self.inner_blocks):
            x = block(x, training, relu_out=i + 1 < len(self.inner_blocks))
        return x
