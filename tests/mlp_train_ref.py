"""Shared by the GPU tests of the training-mode shared-MLP layer (csrc/mlp_train.hip), plain and
fused with the max pool: the case constants, the parameters of a case and the torch CPU
references by tf_util.mlp_torch's formulas, evaluated in float64 and float32. Not a test module."""
import functools
import importlib

import numpy as np

from conftest import PKG_NAME

EPS = 1e-3
SLAB = 1024   # PN2_WGRAD_SLAB_ROWS and PN2_BN_BLOCK_ROWS (include/pn2hip.h)

# the module tests' cloud and SA / FP modules
B, N, NPOINT, RADIUS, NS = 2, 1024, 128, 0.2, 16
SA_MLP, FP_MLP = [32, 64], [64, 32]


def make_params(torch, rows, cin, cout, bn, seed, bias=None):
    g = torch.Generator().manual_seed(seed)
    u = lambda lo, hi, *s: torch.rand(*s, generator=g, dtype=torch.float64) * (hi - lo) + lo  # noqa: E731
    lim = float(np.sqrt(6.0 / (cin + cout)))
    p = {"x": u(-1, 1, rows, cin), "w": u(-lim, lim, cin, cout),
         "b": u(-0.1, 0.1, cout) if bias is None else bias.double(),
         "gamma": u(0.5, 1.5, cout) if bn else None, "beta": u(-0.2, 0.2, cout) if bn else None,
         "go": u(-1, 1, rows, cout)}
    # the values under test are float32: the references start from exactly those numbers
    return {k: None if v is None else v.float() for k, v in p.items()}


def ref_layer(torch, p, dt, relu, mask=None):
    """One layer by tf_util.mlp_torch's formulas in dtype dt on the CPU. mask: the ReLU as a
    product with a given 0/1 mask. Returns (out, y, mean, var) and the leaves."""
    leaves = {k: None if v is None else v.to(dt).clone().requires_grad_(True)
              for k, v in p.items() if k != "go"}
    y = leaves["x"] @ leaves["w"] + leaves["b"]
    mean = var = None
    z = y
    if leaves["gamma"] is not None:
        mean = y.mean(dim=0)
        var = y.var(dim=0, unbiased=False)
        z = (y - mean) * (leaves["gamma"] / torch.sqrt(var + EPS)) + leaves["beta"]
    if relu:
        z = torch.relu(z) if mask is None else z * mask.to(dt)
    return (z, y, mean, var), leaves


def ref_grads(torch, p, dt, relu, mask):
    (out, _, _, _), leaves = ref_layer(torch, p, dt, relu, mask)
    (out * p["go"].to(dt)).sum().backward()
    return {k: v.grad for k, v in leaves.items() if v is not None}


@functools.lru_cache(maxsize=None)
def run_case(case):
    """Forward + backward of one case on the GPU and its references, computed once."""
    import torch
    import pn2hip
    ops, dev = pn2hip.ops, torch.device("cuda:0")
    rows, cin, cout, bn, relu = case
    p = make_params(torch, rows, cin, cout, bn, seed=rows * 31 + cin)
    d = {k: None if v is None else v.to(dev) for k, v in p.items()}
    out, y, mean, var = ops.mlp_layer_train(d["x"], d["w"], d["b"], d["gamma"], d["beta"], EPS, relu)
    grads = ops.mlp_layer_train_grad(d["go"], d["x"], d["w"], y, mean, var, d["gamma"], d["beta"],
                                     EPS, relu, True)
    torch.cuda.synchronize()
    mask = (out > 0).cpu()
    fwd = {dt: ref_layer(torch, p, dt, relu)[0] for dt in (torch.float64, torch.float32)}
    bwd = {dt: ref_grads(torch, p, dt, relu, mask) for dt in (torch.float64, torch.float32)}
    return p, d, (out, y, mean, var), grads, fwd, bwd


def ids(case):
    return "x".join(str(int(v)) for v in case)


def bn_act_bwd(pkg, torch, go, y, mean, var, gamma, beta, relu):
    """pn2_bn_act_bwd through the C ABI: (grad_y, grad_gamma or None, grad_beta)."""
    L = importlib.import_module(PKG_NAME + "._lib")
    rows, C = int(y.shape[0]), int(y.shape[1])
    bn = gamma is not None
    ws_bytes = int(L.lib().pn2_bn_workspace_size(rows, C))
    ws = torch.empty(max(ws_bytes // 4, 4), dtype=torch.float32, device=y.device)
    gy = torch.full_like(y, float("nan"))
    gg = torch.full((C,), float("nan"), device=y.device) if bn else None
    gbeta = torch.full((C,), float("nan"), device=y.device)
    L.check(L.lib().pn2_bn_act_bwd(L.ptr(go), L.ptr(y), rows, C, L.ptr(mean) if bn else None,
                                   L.ptr(var) if bn else None, L.ptr(gamma), L.ptr(beta), EPS,
                                   int(relu), L.ptr(gy), L.ptr(gg), L.ptr(gbeta), L.ptr(ws),
                                   ws_bytes, L.stream_of(y)), "bn_act_bwd")
    return gy, gg, gbeta


def sa_fp(pkg, store, xyz, feats, is_training):
    pu = pkg.pointnet_util
    new_xyz, sa, idx = pu.pointnet_sa_module(xyz, feats, NPOINT, RADIUS, NS, SA_MLP, None, False,
                                             is_training, None, "sa1", params=store)
    fp = pu.pointnet_fp_module(xyz, new_xyz, feats, sa, FP_MLP, is_training, None, "fp1",
                               params=store)
    return new_xyz, sa, fp


# ------------------------------------------------ the layer fused with the max pool
def pool_make_params(torch, groups, ns, cin, cout, bn, seed):
    """make_params over groups * ns rows, with gamma of either sign and a
    (groups, cout) grad_out."""
    g = torch.Generator().manual_seed(seed)
    u = lambda lo, hi, *s: torch.rand(*s, generator=g, dtype=torch.float64) * (hi - lo) + lo  # noqa: E731
    lim = float(np.sqrt(6.0 / (cin + cout)))
    p = {"x": u(-1, 1, groups, ns, cin), "w": u(-lim, lim, cin, cout), "b": u(-0.1, 0.1, cout),
         "gamma": None, "beta": None}
    if bn:
        mag, sign = u(0.5, 1.5, cout), u(-1, 1, cout)
        p["gamma"] = torch.where(sign < 0, -mag, mag)
        p["beta"] = u(-0.2, 0.2, cout)
    p["go"] = u(-1, 1, groups, cout)
    # the values under test are float32: the references start from exactly those numbers
    return {k: None if v is None else v.float() for k, v in p.items()}


def pool_ref_grads(torch, p, dt, relu, mask, arg):
    """Gradients of sum(go * pooled) in dtype dt on the CPU: tf_util.mlp_torch's formulas, the
    ReLU as a product with `mask` (groups, ns, C), the pool as a gather at `arg` (groups, C)."""
    leaves = {k: None if v is None else v.to(dt).clone().requires_grad_(True)
              for k, v in p.items() if k != "go"}
    y = leaves["x"] @ leaves["w"] + leaves["b"]
    z = y
    if leaves["gamma"] is not None:
        flat = y.reshape(-1, y.shape[-1])
        mean, var = flat.mean(dim=0), flat.var(dim=0, unbiased=False)
        z = (y - mean) * (leaves["gamma"] / torch.sqrt(var + EPS)) + leaves["beta"]
    if relu:
        z = z * mask.to(dt)
    pooled = z.gather(1, arg.long()[:, None, :]).squeeze(1)
    (pooled * p["go"].to(dt)).sum().backward()
    return {k: v.grad for k, v in leaves.items() if v is not None}
