"""Shared by tests/test_mlp_train_bf16_cpu.py and tests/test_gpu_mlp_train_bf16.py: the numpy
evaluations of the training layer's bf16 contract (include/pn2hip.h, at pn2_mlp_pack_bf16), the
cases and their inputs, the float64 / float32 formulas of everything the contract leaves fp32
(those of mlp_train_ref, applied to a given y), and the C ABI calls the GPU tests compare bits
with. Not a test module.

Three evaluations of each of the layer's three GEMMs, as in mlp_bf16_ref:

    E    the contract: both operands rounded to bf16 (nearest even), products and sums in float64
    F    the unrounded product in float64
    E32  E with the sums in numpy float32: the CPU stand-in for the kernel and the yardstick of
         support.assert_close (the rounding of given inputs is deterministic, so the project's
         fp32 bar applies unchanged to a single GEMM)
"""
import functools
import importlib

import numpy as np

from conftest import PKG_NAME
from mlp_bf16_ref import bf16_round
from mlp_train_ref import EPS, SLAB

# (rows, cin, cout) of the weight-gradient tests and what each reaches
WGRAD_SHAPES = [
    (1, 3, 5),          # a single row
    (15, 32, 32),       # below one MFMA
    (17, 33, 67),       # a ragged MFMA, ragged tiles
    (65, 40, 72),       # past one block per wave
    (1025, 32, 64),     # two slabs, NJ = 2
    (2050, 64, 160),    # NJ = 4 with a last group of one tile
    (4099, 128, 128),   # several slabs and tiles
]

# the ops' cases: (rows, cin, cout) and, pooled, (groups, ns, cin, cout); ns = 8 is the pooled
# kernels' groups layout, ns = 128 the split one
LAYER_CASES = [(17, 33, 67), (65, 40, 72), (1025, 32, 64), (2050, 64, 160)]
POOL_CASES = [(3, 8, 33, 67), (129, 8, 40, 72), (1, 128, 32, 64), (17, 128, 64, 160)]


def shape_id(shape):
    return "x".join(str(int(v)) for v in shape)


# ------------------------------------------------------------------------------ the GEMMs
def gemm(a, b, mode):
    """a (m, k) @ b (k, n), float32 inputs, by evaluation E, F or E32."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if mode == "F":
        return a.astype(np.float64) @ b.astype(np.float64)
    a, b = bf16_round(a), bf16_round(b)
    if mode == "E":
        return a.astype(np.float64) @ b.astype(np.float64)
    assert mode == "E32"
    return a @ b


def wgrad(x, gy, mode):
    """grad_w (cin, cout) = x^T grad_y over the rows."""
    x, gy = np.asarray(x, np.float32), np.asarray(gy, np.float32)
    return gemm(np.ascontiguousarray(x.reshape(-1, x.shape[-1]).T), gy.reshape(-1, gy.shape[-1]),
                mode)


def forward(x, w, b, mode):
    """y = x W + b; the bias is added unrounded, in the sums' dtype."""
    x = np.asarray(x, np.float32)
    y = gemm(x.reshape(-1, x.shape[-1]), w, mode)
    if b is not None:
        y = y + np.asarray(b, np.float32).astype(y.dtype)
    return y.reshape(x.shape[:-1] + (np.shape(w)[1],))


def grad_x(gy, w, mode):
    """grad_x = grad_y W^T."""
    gy = np.asarray(gy, np.float32)
    out = gemm(gy.reshape(-1, gy.shape[-1]), np.ascontiguousarray(np.asarray(w, np.float32).T),
               mode)
    return out.reshape(gy.shape[:-1] + (np.shape(w)[0],))


# ------------------------------------------------------------------------------ the inputs
def _rng(shape, salt):
    return np.random.default_rng([salt] + [int(v) for v in shape])


@functools.lru_cache(maxsize=None)
def exact_inputs(shape):
    """x of integers in [-4, 4], grad_y of integers in [-4, 4] times 2^-3: every operand is a
    bf16 value and every product and partial sum is exact in fp32."""
    rows, cin, cout = shape
    rng = _rng(shape, 1)
    x = rng.integers(-4, 5, (rows, cin)).astype(np.float32)
    gy = (rng.integers(-4, 5, (rows, cout)) * 0.125).astype(np.float32)
    return x, gy


@functools.lru_cache(maxsize=None)
def random_inputs(shape):
    """x and grad_y uniform in [-1, 1), float32."""
    rows, cin, cout = shape
    rng = _rng(shape, 2)
    return (rng.uniform(-1, 1, (rows, cin)).astype(np.float32),
            rng.uniform(-1, 1, (rows, cout)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def layer_inputs(case, bn):
    """The variables and tensors of one op case (float32 numpy; gamma of both signs)."""
    *lead, cin, cout = case
    rng = _rng(case, 3 + int(bn))
    u = lambda lo, hi, *s: rng.uniform(lo, hi, s).astype(np.float32)  # noqa: E731
    lim = float(np.sqrt(6.0 / (cin + cout)))
    p = {"x": u(-1, 1, *lead, cin), "w": u(-lim, lim, cin, cout), "b": u(-0.1, 0.1, cout),
         "gamma": None, "beta": None, "go": u(-1, 1, lead[0], cout)}
    if bn:
        mag, sign = u(0.5, 1.5, cout), u(-1, 1, cout)
        p["gamma"] = np.where(sign < 0, -mag, mag).astype(np.float32)
        p["beta"] = u(-0.2, 0.2, cout)
    return p


# ------------------------------------------------------------- what stays fp32, from a given y
def act_ref(y, gamma, beta, relu, dt, ns=None):
    """mlp_train_ref.ref_layer's formulas after y, in numpy dtype dt on a given y (..., C):
    (out, mean, var, act); pooled (ns given: y is (groups, ns, C)) out is the max over the ns
    axis of the activation act. mean and var are None without batch norm."""
    y = np.asarray(y).astype(dt)
    flat = y.reshape(-1, y.shape[-1])
    mean = var = None
    z = y
    if gamma is not None:
        mean = flat.mean(axis=0, dtype=dt)
        var = ((flat - mean) ** 2).mean(axis=0, dtype=dt)
        z = (y - mean) * (np.asarray(gamma).astype(dt) / np.sqrt(var + dt(EPS))) + \
            np.asarray(beta).astype(dt)
    if relu:
        z = np.maximum(z, dt(0))
    return (z.max(axis=-2) if ns else z), mean, var, z


# ------------------------------------------------------------------------------ the C ABI
def _L():
    return importlib.import_module(PKG_NAME + "._lib")


def _ws(torch, like, nbytes):
    return torch.empty(max(nbytes // 4, 4), dtype=torch.float32, device=like.device)


def c_wgrad(torch, x, gy, bf16):
    """pn2_mlp_wgrad_bf16 (or pn2_mlp_wgrad) through the C ABI on device tensors: grad_w, poisoned
    with NaN first."""
    L = _L()
    cin, cout = int(x.shape[-1]), int(gy.shape[-1])
    rows = x.numel() // cin
    nbytes = int(L.lib().pn2_mlp_wgrad_workspace_size(rows, cin, cout))
    ws = _ws(torch, x, nbytes)
    gw = torch.full((cin, cout), float("nan"), device=x.device)
    f = L.lib().pn2_mlp_wgrad_bf16 if bf16 else L.lib().pn2_mlp_wgrad
    L.check(f(L.ptr(x), L.ptr(gy), rows, cin, cout, L.ptr(gw), L.ptr(ws), nbytes,
              L.stream_of(x)), "mlp_wgrad")
    return gw


def c_bn_stats(torch, y):
    L = _L()
    C = int(y.shape[-1])
    rows = y.numel() // C
    nbytes = int(L.lib().pn2_bn_workspace_size(rows, C))
    ws = _ws(torch, y, nbytes)
    mean, var = (torch.full((C,), float("nan"), device=y.device) for _ in range(2))
    L.check(L.lib().pn2_bn_stats(L.ptr(y), rows, C, L.ptr(mean), L.ptr(var), L.ptr(ws), nbytes,
                                 L.stream_of(y)), "bn_stats")
    return mean, var


def _bn_ptrs(L, mean, var, gamma, beta):
    bn = gamma is not None
    return (L.ptr(mean) if bn else None, L.ptr(var) if bn else None, L.ptr(gamma) if bn else None,
            L.ptr(beta) if bn else None)


def c_act_fwd(torch, y, mean, var, gamma, beta, relu, pooled):
    """pn2_bn_act_fwd, or pooled pn2_bn_act_pool_fwd over y (groups, ns, C): (out, arg or None)."""
    L = _L()
    C = int(y.shape[-1])
    rows = y.numel() // C
    if pooled:
        ns = int(y.shape[-2])
        out = torch.full((rows // ns, C), float("nan"), device=y.device)
        arg = torch.full((rows // ns, C), -7, dtype=torch.int32, device=y.device)
        L.check(L.lib().pn2_bn_act_pool_fwd(L.ptr(y), rows // ns, ns, C,
                                            *_bn_ptrs(L, mean, var, gamma, beta), EPS, int(relu),
                                            L.ptr(out), L.ptr(arg), L.stream_of(y)),
                "bn_act_pool_fwd")
        return out, arg
    out = torch.full_like(y, float("nan"))
    L.check(L.lib().pn2_bn_act_fwd(L.ptr(y), rows, C, *_bn_ptrs(L, mean, var, gamma, beta), EPS,
                                   int(relu), L.ptr(out), L.stream_of(y)), "bn_act_fwd")
    return out, None


def c_act_bwd(torch, go, arg, y, mean, var, gamma, beta, relu):
    """pn2_bn_act_bwd, or with arg pn2_bn_act_pool_bwd: (grad_y, grad_gamma or None, grad_beta)."""
    L = _L()
    C = int(y.shape[-1])
    rows = y.numel() // C
    bn = gamma is not None
    gy = torch.full_like(y, float("nan"))
    gg = torch.full((C,), float("nan"), device=y.device) if bn else None
    gbeta = torch.full((C,), float("nan"), device=y.device)
    if arg is not None:
        ns = int(y.shape[-2])
        nbytes = int(L.lib().pn2_bn_pool_workspace_size(rows // ns, C))
        ws = _ws(torch, y, nbytes)
        L.check(L.lib().pn2_bn_act_pool_bwd(L.ptr(go), L.ptr(arg), L.ptr(y), rows // ns, ns, C,
                                            *_bn_ptrs(L, mean, var, gamma, beta), EPS, int(relu),
                                            L.ptr(gy), L.ptr(gg) if bn else None, L.ptr(gbeta),
                                            L.ptr(ws), nbytes, L.stream_of(y)), "bn_act_pool_bwd")
    else:
        nbytes = int(L.lib().pn2_bn_workspace_size(rows, C))
        ws = _ws(torch, y, nbytes)
        L.check(L.lib().pn2_bn_act_bwd(L.ptr(go), L.ptr(y), rows, C,
                                       *_bn_ptrs(L, mean, var, gamma, beta), EPS, int(relu),
                                       L.ptr(gy), L.ptr(gg) if bn else None, L.ptr(gbeta),
                                       L.ptr(ws), nbytes, L.stream_of(y)), "bn_act_bwd")
    return gy, gg, gbeta


def wgrad_parts(rows, cin, cout):
    """(nslabs, nparts) of the weight gradient, from its workspace size (the rule of
    tests/test_gpu_mlp_train_scale.py)."""
    ws = int(_L().lib().pn2_mlp_wgrad_workspace_size(rows, cin, cout))
    ntiles = -(-cin // 32) * -(-cout // 32)
    assert ws % (ntiles * 4096) == 0
    return -(-rows // SLAB), ws // (ntiles * 4096)
