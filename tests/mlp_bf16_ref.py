"""numpy evaluations of the bf16 matrix-core mode's numerical contract (include/pn2hip.h,
pn2_mlp_pack_bf16) and the inputs that tests/test_mlp_bf16_cpu.py and tests/test_gpu_mlp_bf16.py
share.

A layer is a dict: W (cin, cout) float32, scale / shift (cout) float32 or None (1 / 0), relu,
bf16 (packed by pn2_mlp_pack_bf16 or by pn2_mlp_pack). Three evaluations of a chain:

    E    the contract: a bf16 layer's operands rounded to bf16 (nearest even; the activations
         from the fp32 value the layer before hands over), everything else unrounded, the sums
         and the epilogue in float64
    F    the unrounded layers in float64 (no bf16 anywhere)
    E32  E with the sums and the epilogue in numpy float32: the CPU stand-in for the kernel

The chain bound is  max|got - E| <= max|E - F| / 16  (a tiny fp32 difference may flip a later
bf16 rounding, so the fp32 bar does not apply to chains); the CPU test holds the stand-in to
1/64 of max|E - F| on the same inputs, so a failing GPU test cannot blame them.

Choice of inputs. An activation whose fp32 value lies within fp32 summation noise of a bf16 tie
rounds one way or the other depending on the order of the sum; one such flip moves an output
by about 2^-8 |x| |w|, 0.02 to 0.5 of max|E - F| at these shapes, and numpy's own float32
product shows one in roughly every seventh case. Such inputs test the summation order, not the
contract, so the seeds are chosen without them: a seed is used when every member of a family
of fp32 stand-ins, which differ only in the order of the sums (STANDINS: numpy's product, sums
over chunks of 16 input features front to back and back to front, and the float64 sum rounded
once), stays within 1/64. The seeds are the first ones from 0 that pass, five per chain, one
per other case; nothing a GPU computed enters the choice.
"""
import functools

import numpy as np

STANDINS = ("E32", "E32c", "E32r", "E32d")


def bf16_round(a):
    """float32 -> the nearest bf16 (ties to even), returned as float32."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(a))


def make_layer(rng, cin, cout, bf16=True, relu=True, affine=True):
    """weights U[-1,1) * sqrt(3/cin), scale in [0.5, 1.5], shift in [-0.5, 0.5]."""
    L = {"W": (rng.uniform(-1, 1, (cin, cout)) * np.sqrt(3.0 / cin)).astype(np.float32),
         "scale": None, "shift": None, "relu": relu, "bf16": bf16}
    if affine:
        L["scale"] = rng.uniform(0.5, 1.5, cout).astype(np.float32)
        L["shift"] = rng.uniform(-0.5, 0.5, cout).astype(np.float32)
    return L


def make_chain(rng, cin, widths, flags=None, last_relu=True):
    """flags: per layer True = bf16 (default: all)."""
    layers, c = [], cin
    for i, w in enumerate(widths):
        last = i == len(widths) - 1
        layers.append(make_layer(rng, c, w, bf16=True if flags is None else flags[i],
                                 relu=last_relu if last else True))
        c = w
    return layers


def _epilogue(y, L, dt):
    if L["scale"] is not None:
        y = y * L["scale"].astype(dt) + L["shift"].astype(dt)
    return np.maximum(y, dt(0)) if L["relu"] else y


def layer_eval(x, L, mode):
    """One layer on x (..., cin): mode 'E', 'F' or 'E32'. x is float64 for E / F (the value
    the layer before hands over is its float32 rounding), float32 for E32."""
    W = L["W"]
    if mode == "F":
        return _epilogue(np.asarray(x, np.float64) @ W.astype(np.float64), L, np.float64)
    if mode == "E":
        if L["bf16"]:
            xin = bf16_round(np.asarray(x, np.float64).astype(np.float32)).astype(np.float64)
            return _epilogue(xin @ bf16_round(W).astype(np.float64), L, np.float64)
        return _epilogue(np.asarray(x, np.float64) @ W.astype(np.float64), L, np.float64)
    assert mode in STANDINS
    x = np.asarray(x, np.float32)
    if L["bf16"]:
        x, W = bf16_round(x), bf16_round(W)
    return _epilogue(_matmul32(x, W, mode), L, np.float32)


def _matmul32(x, W, mode):
    """x @ W with float32 sums in the stand-in's order."""
    if mode == "E32":
        return x @ W
    if mode == "E32d":
        return (x.astype(np.float64) @ W.astype(np.float64)).astype(np.float32)
    starts = list(range(0, W.shape[0], 16))
    acc = np.zeros(x.shape[:-1] + (W.shape[1],), np.float32)
    for c in (starts if mode == "E32c" else starts[::-1]):
        acc = acc + x[..., c:c + 16] @ W[c:c + 16]
    return acc


def chain_eval(x, layers, mode):
    y = np.asarray(x, np.float32 if mode in STANDINS else np.float64)
    for L in layers:
        y = layer_eval(y, L, mode)
    return y


def pool_eval(y, pool):
    """Pooling over the nsample axis of y (B, M, ns, C) (pointnet_util.py:130-145)."""
    if pool is None:
        return y
    if pool == "max":
        return y.max(axis=2)
    if pool == "avg":
        return y.sum(axis=2) / y.dtype.type(y.shape[2])
    if pool == "max_and_avg":
        return np.concatenate([y.sum(axis=2) / y.dtype.type(y.shape[2]), y.max(axis=2)], axis=-1)
    raise ValueError(pool)


def attention_eval(X, q, k, v, att_scale, att_shift, add_max, mode):
    """The attention tail on the MLP output X (B, M, ns, C) (attention_layer.py:29-45, :259-261,
    :296-303): the query Dense of each group's first neighbour (q: an fp32 layer), key and value
    Dense (k, v: bf16 or fp32 layers), head h = the flat block [4 ns h, 4 ns (h + 1)) of the
    group's (ns, C) keys / values, softmax((K_h q_h) / 2) V_h, the batch norm, + max over ns of
    X. Everything after the Dense layers is fp32 work in the kernel: float64 here for E / F,
    float32 for E32."""
    dt = np.float32 if mode in STANDINS else np.float64
    B, M, ns, C = X.shape
    Q = layer_eval(X[:, :, 0], q, mode).astype(dt)
    K = layer_eval(X, k, mode).astype(dt).reshape(B, M, C // 4, ns, 4)
    V = layer_eval(X, v, mode).astype(dt).reshape(B, M, C // 4, ns, 4)
    s = np.einsum("bmhjd,bmhd->bmhj", K, Q.reshape(B, M, C // 4, 4)) / dt(2)
    e = np.exp(s - s.max(axis=-1, keepdims=True))
    a = e / e.sum(axis=-1, keepdims=True)
    out = np.einsum("bmhj,bmhjd->bmhd", a, V).reshape(B, M, C)
    out = out * att_scale.astype(dt) + att_shift.astype(dt)
    if add_max:
        out = out + np.asarray(X, dt).max(axis=2)
    return out


def group_rows(xyz, points, new_xyz, idx, xyz_last=False):
    """pn2_group_concat in numpy float32: [xyz[idx] - new_xyz, points[idx]] (or [points, xyz]),
    (B, M, ns, 3 + C). The subtraction is one fp32 operation, as in the kernel."""
    B = xyz.shape[0]
    b = np.arange(B)[:, None, None]
    g = xyz[b, idx] - new_xyz[:, :, None, :]
    if points is None:
        return g
    return np.concatenate([points[b, idx], g] if xyz_last else [g, points[b, idx]], axis=-1)


def fp_rows(dist, nn, p1, p2):
    """pn2_fp_apply in numpy float32: IDW weights of dist (B, n, 3), the interpolation of p2 at
    nn, concat [interp, p1] (pointnet_util.py:218-226), in the kernel's operation order."""
    one = np.float32(1)
    r = one / np.maximum(dist, np.float32(1e-10))
    w = r / ((r[..., 0] + r[..., 1]) + r[..., 2])[..., None]
    b = np.arange(p2.shape[0])[:, None]
    t = [p2[b, nn[..., j]] * w[..., j, None] for j in range(3)]
    interp = (t[0] + t[1]) + t[2]
    return interp if p1 is None else np.concatenate([interp, p1], axis=-1)


def ratios(evaluate):
    """max|S - E| / max|E - F| of every stand-in S; evaluate(mode) -> the case's output."""
    E, F = evaluate("E"), evaluate("F")
    d = np.abs(E - F).max()
    return {m: float(np.abs(evaluate(m).astype(np.float64) - E).max() / d) for m in STANDINS}, d


def first_seeds(count, evaluate_at, limit=64):
    """The first `count` seeds from 0 at which every stand-in stays within 1/64 (see the module
    docstring); evaluate_at(seed) -> evaluate(mode)."""
    seeds = []
    for seed in range(limit):
        if max(ratios(evaluate_at(seed))[0].values()) <= 1 / 64:
            seeds.append(seed)
            if len(seeds) == count:
                return tuple(seeds)
    raise AssertionError(f"fewer than {count} usable seeds below {limit}")


# ---------------------------------------------------------------- shared inputs

SHAPE_ROWS = (1, 33, 100)
SHAPE_CINS = (3, 8, 9, 16, 19, 35)
SHAPE_WIDTHS = ([32], [21], [13, 40], [32, 32, 64])
BIG_SHAPE = (64, 259, [256, 512])  # rows, cin, widths: the weights stay in global memory

# (cin, widths, flags (None = all bf16), last layer has a ReLU)
CHAINS = {
    "sa1": (9, [32, 32, 64], None, True),
    "sa2": (67, [64, 64, 128], None, True),
    "fp4_head": (131, [128, 128, 128, 21], [True, True, True, False], False),
    "two": (3, [32, 64], None, True),
    "sa4": (259, [256, 512], None, True),
    "mixed_bfb": (19, [32, 32, 64], [True, False, True], True),
    "mixed_fb": (19, [32, 64], [False, True], True),
}
CHAIN_ROWS = 96


def chain_case(name, seed):
    cin, widths, flags, last_relu = CHAINS[name]
    rng = np.random.default_rng([seed, cin, len(widths), sum(widths)])
    layers = make_chain(rng, cin, widths, flags, last_relu)
    x = rng.uniform(-1, 1, (CHAIN_ROWS, cin)).astype(np.float32)
    return x, layers


def chain_evaluate(name, seed):
    x, layers = chain_case(name, seed)
    return functools.lru_cache(None)(lambda mode: chain_eval(x, layers, mode))


@functools.lru_cache(None)
def chain_seeds(name):
    """Five seeds per chain."""
    return first_seeds(5, lambda seed: chain_evaluate(name, seed))


GROUP_CASES = [
    # (ns, C, pool, xyz_last)
    (8, 0, "max", False), (8, 6, "avg", False),
    (32, 0, "max", False), (32, 6, "max_and_avg", False), (32, 6, None, False),
    (64, 0, "avg", False), (64, 6, "max", True),
    (128, 0, "max_and_avg", False), (128, 6, "max", False), (128, 6, None, False),
]


def group_evaluate(ns, C, pool, xyz_last, seed):
    xyz, points, new_xyz, idx, layers = group_case(ns, C, seed)
    x = group_rows(xyz, points, new_xyz, idx, xyz_last)
    return functools.lru_cache(None)(lambda mode: pool_eval(chain_eval(x, layers, mode), pool))


@functools.lru_cache(None)
def group_seed(ns, C, pool, xyz_last):
    return first_seeds(1, lambda seed: group_evaluate(ns, C, pool, xyz_last, seed))[0]


def group_case(ns, C, seed=0, B=2, N=256, M=16, widths=(32, 32, 64)):
    rng = np.random.default_rng([seed, ns, C, M])
    xyz = rng.uniform(-1, 1, (B, N, 3)).astype(np.float32)
    points = rng.uniform(-1, 1, (B, N, C)).astype(np.float32) if C else None
    new_xyz = xyz[:, rng.choice(N, M, replace=False)].copy()
    idx = rng.integers(0, N, (B, M, ns)).astype(np.int32)
    layers = make_chain(rng, 3 + C, list(widths))
    return xyz, points, new_xyz, idx, layers


def fp_evaluate(C1, seed):
    dist, nn, p1, p2, layers = fp_case(C1, seed)
    x = fp_rows(dist, nn, p1, p2)
    return functools.lru_cache(None)(lambda mode: chain_eval(x, layers, mode))


@functools.lru_cache(None)
def fp_seed(C1):
    return first_seeds(1, lambda seed: fp_evaluate(C1, seed))[0]


def fp_case(C1, seed=0, B=2, n=100, m=20, C2=32, widths=(64, 32)):
    rng = np.random.default_rng([seed, C1, n, m])
    dist = rng.uniform(1e-3, 1.0, (B, n, 3)).astype(np.float32)
    nn = rng.integers(0, m, (B, n, 3)).astype(np.int32)
    p1 = rng.uniform(-1, 1, (B, n, C1)).astype(np.float32) if C1 else None
    p2 = rng.uniform(-1, 1, (B, m, C2)).astype(np.float32)
    layers = make_chain(rng, C1 + C2, list(widths))
    return dist, nn, p1, p2, layers


ATTN_CASES = [
    # (C_in, widths, ns, B, M, add_max)
    (6, [32, 32, 64], 32, 2, 16, False),
    (6, [32, 32, 64], 32, 2, 16, True),
    (16, [512], 32, 1, 4, False),  # C = 512 = 4 * (4 ns): four K/V column segments
]


def attn_evaluate(C_in, widths, ns, B, M, add_max, seed):
    xyz, points, new_xyz, idx, layers, dense, sc, sh = attn_case(C_in, widths, ns, B, M, seed)
    x = group_rows(xyz, points, new_xyz, idx)
    return functools.lru_cache(None)(lambda mode: attention_eval(
        chain_eval(x, layers, mode), *dense, sc, sh, add_max, mode))


@functools.lru_cache(None)
def attn_seed(C_in, widths, ns, B, M, add_max):
    return first_seeds(1, lambda seed: attn_evaluate(C_in, list(widths), ns, B, M, add_max,
                                                     seed))[0]


def attn_case(C_in, widths, ns, B, M, seed=0, N=256):
    xyz, points, new_xyz, idx, _ = group_case(ns, C_in, seed, B, N, M)
    rng = np.random.default_rng([seed, 77, ns, widths[-1]])
    layers = make_chain(rng, 3 + C_in, list(widths))
    C = widths[-1]
    # Dense layers: a bias (scale None in the pack = 1; the shift is the bias), no ReLU
    dense = []
    for j in range(3):
        L = make_layer(rng, C, C, bf16=j > 0, relu=False, affine=False)
        L["shift"] = rng.uniform(-0.5, 0.5, C).astype(np.float32)
        L["scale"] = np.ones(C, np.float32)
        dense.append(L)
    att_scale = rng.uniform(0.5, 1.5, C).astype(np.float32)
    att_shift = rng.uniform(-0.5, 0.5, C).astype(np.float32)
    return xyz, points, new_xyz, idx, layers, dense, att_scale, att_shift


def exact_chain(rng, rows, cin, widths):
    """Operands that are small integers over 8 and whose every intermediate activation is exactly
    a bf16 value, so the bf16 path, the fp32 path, E, F and E32 all give the same bits: x in
    {-2..2}/8; a layer that feeds another one has at most two non-zero weights (+-1/8 in the
    first layer, +-1 in later ones) per output, a last layer is dense in {-2..2}/8. No scale,
    no shift, ReLU on every layer but the last."""
    x = (rng.integers(-2, 3, (rows, cin)) / 8.0).astype(np.float32)
    layers, c = [], cin
    for i, w in enumerate(widths):
        if i == len(widths) - 1:
            W = rng.integers(-2, 3, (c, w)) / 8.0
        else:
            W = np.zeros((c, w))
            for o in range(w):
                f = rng.choice(c, size=min(2, c), replace=False)
                W[f, o] = rng.choice([-1.0, 1.0], size=len(f)) * (0.125 if i == 0 else 1.0)
        layers.append({"W": W.astype(np.float32), "scale": None, "shift": None,
                       "relu": i < len(widths) - 1, "bf16": True})
        c = w
    return x, layers


def as_fp32(layers):
    return [dict(L, bf16=False) for L in layers]


def packed_size_bf16(cin, cout):
    """The documented size of pn2_mlp_pack_bf16's output in bytes."""
    return ((cout + 31) // 32) * (((cin + 15) // 16) * 1024 + 256)
