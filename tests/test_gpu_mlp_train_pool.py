"""GPU: the training MLP's last layer fused with the max pool over nsample
(torch.ops.pn2.mlp_layer_train_pool / _grad, pn2_bn_act_pool_fwd / _bwd in csrc/mlp_train.hip)
through torch.ops.pn2, the C ABI and the public tf_util / pointnet_util interfaces.

Forward: exact. y, mean, var, out must have the bits of torch.ops.pn2.mlp_layer_train (tested in
test_gpu_mlp_train.py) followed by a max over the ns axis, and arg must be the first sample
that attains the maximum.

Backward: torch float64 autograd on the CPU over tf_util.mlp_torch's formulas, with the ReLU as
a product with the mask `out_full > 0` and the pool as a gather at `arg`, both taken from the
forward under test (a ReLU or an argmax that flips within rounding is a discrete difference, not
an error; test_gpu_mlp_train.py's docstring). Tolerance, the project's:

    max |gpu - f64|  <=  max(4 * max |fp32 - f64|,  1e-6 * (1 + max |f64|))

where fp32 is the same reference evaluated in float32 on the CPU.

gamma is drawn from +-[0.5, 1.5]: about half the channels have a negative scale, where the
largest activation belongs to the smallest y.
"""
import functools
import importlib

import numpy as np
import pytest

from conftest import PKG_NAME
from mlp_train_ref import B, EPS, FP_MLP, N, NPOINT, NS, RADIUS, SA_MLP, ids
from mlp_train_ref import pool_make_params as make_params
from mlp_train_ref import pool_ref_grads as ref_grads
from support import assert_close, gpu_marks

pytestmark = gpu_marks

PG = 128      # PN2_BN_POOL_BLOCK_GROUPS (include/pn2hip.h): groups per stage-1 partial
T, F = True, False

# (groups, ns, cin, cout, batch norm, relu)
CASES = [
    (64, 32, 9, 64, T, T),
    (5, 1, 16, 32, T, T),
    (33, 3, 9, 33, T, T),
    (2, 1500, 6, 40, T, T),           # group_all-like: a group split across row lanes
    (1, 1, 16, 32, T, T),             # a single row: zero variance
    (17, 7, 67, 96, T, F),
    (40, 16, 12, 21, F, T),
    (40, 16, 12, 21, F, F),
    (70, 5, 20, 200, T, T),
    (PG - 1, 2, 16, 32, T, T),        # one below / above the groups of a stage-1 partial
    (PG + 1, 2, 16, 32, T, T),
    (3, 64, 9, 33, T, T),             # the largest ns of the thread-per-group layout ...
    (3, 65, 9, 33, T, T),             # ... and the smallest of the split layout
    (3, 300, 6, 40, F, T),            # split layout without batch norm, a partial last chunk
]


@pytest.fixture(scope="module")
def env():
    import torch
    pkg = importlib.import_module(PKG_NAME)
    import pn2hip
    return pkg, pn2hip.ops, torch, torch.device("cuda:0")


def first_argmax(out_full, out):
    """(groups, C) lowest j with out_full[g, j, c] == out[g, c], on the CPU (numpy's argmax
    returns the first maximum)."""
    eq = out_full.cpu().numpy() == out.cpu().numpy()[:, None, :]
    assert eq.any(axis=1).all(), "out is not an element of the activation"
    return np.argmax(eq, axis=1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def run_case(case):
    """Forward + backward of one case on the GPU, the unfused layer and the references, once."""
    import torch
    import pn2hip
    ops, dev = pn2hip.ops, torch.device("cuda:0")
    groups, ns, cin, cout, bn, relu = case
    p = make_params(torch, groups, ns, cin, cout, bn, seed=groups * 31 + ns * 7 + cin)
    d = {k: None if v is None else v.to(dev) for k, v in p.items()}
    fused = ops.mlp_layer_train_pool(d["x"], d["w"], d["b"], d["gamma"], d["beta"], EPS, relu)
    out, y, mean, var, arg = fused
    grads = ops.mlp_layer_train_pool_grad(d["go"], arg, d["x"], d["w"], y, mean, var, d["gamma"],
                                          d["beta"], EPS, relu, True)
    plain = ops.mlp_layer_train(d["x"], d["w"], d["b"], d["gamma"], d["beta"], EPS, relu)
    torch.cuda.synchronize()
    mask, arg_cpu = (plain[0] > 0).cpu(), arg.cpu()
    bwd = {dt: ref_grads(torch, p, dt, relu, mask, arg_cpu) for dt in (torch.float64, torch.float32)}
    return p, d, fused, grads, plain, bwd


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_forward_is_exact(env, case):
    pkg, ops, torch, dev = env
    groups, ns, cin, cout, bn, relu = case
    p, _, (out, y, mean, var, arg), _, (out_full, y0, mean0, var0), _ = run_case(case)
    assert y.shape == (groups, ns, cout) and out.shape == arg.shape == (groups, cout)
    assert arg.dtype == torch.int32
    assert torch.equal(y, y0) and torch.equal(mean, mean0) and torch.equal(var, var0)
    assert mean.numel() == (cout if bn else 0)
    assert torch.equal(out, out_full.max(dim=1).values)
    want = first_argmax(out_full, out)
    got = arg.cpu().numpy()
    assert np.array_equal(got, want), f"{(got != want).sum()} of {got.size} arg differ"
    if bn:
        assert 0 < int((p["gamma"] < 0).sum()) < cout, "the case needs gamma of either sign"


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_backward(env, case):
    pkg, ops, torch, dev = env
    bn = case[4]
    p, _, _, (gx, gw, gb, gg, gbeta), _, bwd = run_case(case)
    r64, r32 = bwd[torch.float64], bwd[torch.float32]
    assert_close(gx, r64["x"], r32["x"], "grad_x")
    assert_close(gw, r64["w"], r32["w"], "grad_w")
    assert_close(gb, r64["b"], r32["b"], "grad_b")
    if bn:
        assert (gb == 0).all()  # the batch mean absorbs the bias
        assert_close(gg, r64["gamma"], r32["gamma"], "grad_gamma")
        assert_close(gbeta, r64["beta"], r32["beta"], "grad_beta")
    else:
        assert gg.numel() == 0 and gbeta.numel() == 0


def test_need_grad_x_false_and_autograd(env):
    pkg, ops, torch, dev = env
    _, d, (out, y, mean, var, arg), full, _, _ = run_case(CASES[0])
    part = ops.mlp_layer_train_pool_grad(d["go"], arg, d["x"], d["w"], y, mean, var, d["gamma"],
                                         d["beta"], EPS, True, False)
    assert part[0].numel() == 0
    for i in range(1, 5):
        assert torch.equal(part[i], full[i]), i
    # through autograd: the registered backward is the gradient op
    leaves = {k: d[k].clone().requires_grad_(True) for k in ("x", "w", "b", "gamma", "beta")}
    res = ops.mlp_layer_train_pool(leaves["x"], leaves["w"], leaves["b"], leaves["gamma"],
                                   leaves["beta"], EPS, True)
    assert res[0].requires_grad and not any(t.requires_grad for t in res[1:])
    (res[0] * d["go"]).sum().backward()
    for k, want in zip(("x", "w", "b", "gamma", "beta"), full):
        assert torch.equal(leaves[k].grad, want), k


# ------------------------------------------------------------------- C ABI ----------------

def pool_fwd_c(pkg, torch, y, mean, var, gamma, beta, relu):
    """pn2_bn_act_pool_fwd through the C ABI on y (groups, ns, C), outputs pre-filled."""
    L = importlib.import_module(PKG_NAME + "._lib")
    groups, ns, C = (int(s) for s in y.shape)
    out = torch.full((groups, C), float("nan"), device=y.device)
    arg = torch.full((groups, C), -1, dtype=torch.int32, device=y.device)
    L.check(L.lib().pn2_bn_act_pool_fwd(L.ptr(y), groups, ns, C, L.ptr(mean), L.ptr(var),
                                        L.ptr(gamma), L.ptr(beta), EPS, int(relu), L.ptr(out),
                                        L.ptr(arg), L.stream_of(y)), "bn_act_pool_fwd")
    return out, arg


def pool_bwd_c(pkg, torch, go, arg, y, mean, var, gamma, beta, relu):
    """pn2_bn_act_pool_bwd through the C ABI: (grad_y, grad_gamma or None, grad_beta), outputs
    pre-filled with NaN."""
    L = importlib.import_module(PKG_NAME + "._lib")
    groups, ns, C = (int(s) for s in y.shape)
    bn = gamma is not None
    ws_bytes = int(L.lib().pn2_bn_pool_workspace_size(groups, C))
    ws = torch.full((max(ws_bytes // 4, 4),), float("nan"), device=y.device)
    gy = torch.full_like(y, float("nan"))
    gg = torch.full((C,), float("nan"), device=y.device) if bn else None
    gbeta = torch.full((C,), float("nan"), device=y.device)
    L.check(L.lib().pn2_bn_act_pool_bwd(L.ptr(go), L.ptr(arg), L.ptr(y), groups, ns, C,
                                        L.ptr(mean), L.ptr(var), L.ptr(gamma), L.ptr(beta), EPS,
                                        int(relu), L.ptr(gy), L.ptr(gg), L.ptr(gbeta), L.ptr(ws),
                                        ws_bytes, L.stream_of(y)), "bn_act_pool_bwd")
    return gy, gg, gbeta


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_c_abi_writes_every_output(env, case):
    pkg, ops, torch, dev = env
    groups, ns, cin, cout, bn, relu = case
    _, d, (out, y, mean, var, arg), grads, _, _ = run_case(case)
    stats = (mean, var, d["gamma"], d["beta"]) if bn else (None,) * 4
    o, a = pool_fwd_c(pkg, torch, y, *stats, relu)
    assert torch.isfinite(o).all() and (a >= 0).all() and (a < ns).all()
    assert torch.equal(o, out) and torch.equal(a, arg)
    gy, gg, gbeta = pool_bwd_c(pkg, torch, d["go"], arg, y, *stats, relu)
    assert torch.isfinite(gy).all() and torch.isfinite(gbeta).all()
    if bn:
        assert torch.isfinite(gg).all()
        assert torch.equal(gg, grads[3]) and torch.equal(gbeta, grads[4])
    else:
        assert gg is None and torch.equal(gbeta, grads[2])  # the bias gradient
        # grad_y = dz: grad_out at the winner (where the ReLU passes), exactly 0 elsewhere
        hit = torch.zeros_like(y, dtype=torch.bool).scatter_(1, arg.long()[:, None, :], True)
        live = hit & (y > 0) if relu else hit
        assert torch.equal(gy, torch.where(live, d["go"][:, None, :].expand_as(y),
                                           torch.zeros_like(y)))


@pytest.mark.parametrize("ns", [16, 80])
def test_padding_copies_of_the_first_row_never_win(env, ns):
    """A ball query pads a group of cnt neighbours with copies of its first: rows j >= cnt are
    copies of row 0, so the lowest index that attains the maximum is below cnt. ns = 80 runs the
    layout where a group's samples are split across lanes and combined."""
    pkg, ops, torch, dev = env
    groups, C = 48, 40
    g = torch.Generator().manual_seed(ns)
    y = torch.rand(groups, ns, C, generator=g) * 2 - 1
    cnt = 1 + torch.arange(groups) % ns
    pad = torch.arange(ns)[None, :] >= cnt[:, None]
    y = torch.where(pad[:, :, None], y[:, :1, :], y).to(dev)
    flat = y.reshape(-1, C)
    mean, var = flat.mean(0), flat.var(0, unbiased=False)
    mag = torch.rand(C, generator=g) + 0.5
    gamma = torch.where(torch.arange(C) % 2 == 0, mag, -mag).to(dev)
    beta = (torch.rand(C, generator=g) * 0.4 - 0.2).to(dev)
    for relu in (True, False):
        for stats in ((mean, var, gamma, beta), (None,) * 4):
            out, arg = pool_fwd_c(pkg, torch, y, *stats, relu)
            assert (arg < cnt.to(dev)[:, None]).all(), (relu, stats[0] is not None)
            assert (arg >= 0).all()
    assert cnt.min() == 1 and cnt.max() == min(ns, groups)


def test_dead_channels(env):
    """beta = -100 on some channels: every pre-activation there is negative, so out = 0 and
    arg = 0 (the lowest index of an all-zero group), and nothing flows back through them."""
    pkg, ops, torch, dev = env
    groups, ns, cin, cout = 64, 32, 9, 64
    p = make_params(torch, groups, ns, cin, cout, True, seed=5)
    dead = torch.arange(cout) % 3 == 0
    p["beta"] = torch.where(dead, torch.tensor(-100.0), p["beta"])
    d = {k: v.to(dev) for k, v in p.items()}
    out, y, mean, var, arg = ops.mlp_layer_train_pool(d["x"], d["w"], d["b"], d["gamma"],
                                                      d["beta"], EPS, True)
    dd = dead.to(dev)
    assert (out[:, dd] == 0).all() and (arg[:, dd] == 0).all()
    assert (out[:, ~dd] > 0).any()
    gy, gg, gbeta = pool_bwd_c(pkg, torch, d["go"], arg, y, mean, var, d["gamma"], d["beta"], True)
    assert (gg[dd] == 0).all() and (gbeta[dd] == 0).all() and (gy[:, :, dd] == 0).all()
    assert (gg[~dd] != 0).any() and (gbeta[~dd] != 0).any()
    grads = ops.mlp_layer_train_pool_grad(d["go"], arg, d["x"], d["w"], y, mean, var, d["gamma"],
                                          d["beta"], EPS, True, True)
    assert (grads[3][dd] == 0).all() and (grads[4][dd] == 0).all()


@pytest.mark.parametrize("case", [(300, 32, 64, 128, T, T), (2, 1500, 6, 40, T, T)], ids=ids)
def test_deterministic(env, case):
    pkg, ops, torch, dev = env
    groups, ns, cin, cout, bn, relu = case
    p = make_params(torch, groups, ns, cin, cout, bn, seed=11)
    d = {k: v.to(dev) for k, v in p.items()}

    def run():
        f = ops.mlp_layer_train_pool(d["x"], d["w"], d["b"], d["gamma"], d["beta"], EPS, relu)
        g = ops.mlp_layer_train_pool_grad(d["go"], f[4], d["x"], d["w"], f[1], f[2], f[3],
                                          d["gamma"], d["beta"], EPS, relu, True)
        return list(f) + list(g)

    a, b = run(), run()
    for i, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(u, v), f"output {i} differs between two runs"


def test_empty_input_and_no_samples(env):
    pkg, ops, torch, dev = env
    tu = pkg.tf_util
    w = torch.zeros(9, 32, device=dev)
    x = torch.empty((0, 8, 9), device=dev)
    out, y, mean, var, arg = ops.mlp_layer_train_pool(x, w, None, torch.ones(32, device=dev),
                                                      torch.zeros(32, device=dev), EPS, True)
    assert out.shape == arg.shape == (0, 32) and y.shape == (0, 8, 32)
    assert (mean == 0).all() and (var == 0).all()
    grads = ops.mlp_layer_train_pool_grad(out, arg, x, w, y, mean, var, torch.ones(32, device=dev),
                                          torch.zeros(32, device=dev), EPS, True, True)
    assert grads[0].shape == x.shape and all((g == 0).all() for g in grads[1:])
    with pytest.raises(ValueError):
        ops.mlp_layer_train_pool(torch.empty((4, 0, 9), device=dev), w, None, None, None, EPS, True)
    # mlp_train: no rows, the moving averages stay
    store = tu.ParamStore(seed=1).trainable(dev)
    layers = tu.torch_layers(store, ["e"], 9, [32])
    assert tu.mlp_train(x, layers, None, pool="max").shape == (0, 32)
    assert (store["e/bn/moving_mean"] == 0).all() and (store["e/bn/moving_variance"] == 1).all()
    with pytest.raises(pkg.InvalidArgumentError):
        tu.mlp_train(x, layers, None, pool="avg")


# ------------------------------------------------------------------- modules --------------

VARS = (("w", "weights"), ("b", "biases"), ("gamma", "bn/gamma"), ("beta", "bn/beta"))


@pytest.fixture(scope="module")
def cloud(env):
    pkg, ops, torch, dev = env
    xyz, feats = pkg.synth.batch([0, 1], N, "scannet", with_features=True)
    return torch.from_numpy(xyz).to(dev), torch.from_numpy(feats).to(dev)


@pytest.fixture
def spy(env, monkeypatch):
    """Names of the torch.ops.pn2 ops the mirror modules call, in order."""
    pkg = env[0]
    names, real = [], pkg._torch_ops.call

    def call(name, *args):
        names.append(name)
        return real(name, *args)
    monkeypatch.setattr(pkg._torch_ops, "call", call)
    return names


def layer_values(store, scopes):
    """The float32 values of the layers' variables as (cin, cout) / (cout) CPU tensors."""
    out = []
    for s in scopes:
        w = store[f"{s}/weights"].detach().cpu()
        out.append({k: store[f"{s}/{name}"].detach().cpu().reshape(
            (-1, w.shape[-1]) if k == "w" else (-1,)) for k, name in VARS})
    return out


def branch_forward(ops, torch, G, vals, dev):
    """The branch's layers op by op on the GPU: the ReLU masks of every layer, the pooled
    output and its arg from the fused op on the last."""
    h, masks = G.detach(), []
    for i, v in enumerate(vals):
        a = [v[k].to(dev) for k in ("w", "b", "gamma", "beta")]
        if i == len(vals) - 1:
            out, _, _, _, arg = ops.mlp_layer_train_pool(h, *a, EPS, True)
        h = ops.mlp_layer_train(h, *a, EPS, True)[0]
        masks.append((h > 0).cpu())
    return masks, out, arg.cpu()


def branch_ref(torch, dt, G, vals, masks, arg, go):
    """Gradients of sum(go * max-pooled MLP(G)) in dtype dt on the CPU, from the grouped tensor
    G (B, M, ns, cin) on: (grad_G, [per-layer {w, b, gamma, beta} gradients])."""
    a = G.detach().cpu().to(dt).clone().requires_grad_(True)
    x, leaves = a, []
    for v, m in zip(vals, masks):
        L = {k: t.to(dt).clone().requires_grad_(True) for k, t in v.items()}
        y = x @ L["w"] + L["b"]
        flat = y.reshape(-1, y.shape[-1])
        mean, var = flat.mean(0), flat.var(0, unbiased=False)
        x = ((y - mean) * (L["gamma"] / torch.sqrt(var + EPS)) + L["beta"]) * m.to(dt)
        leaves.append(L)
    pooled = x.gather(2, arg.long()[:, :, None, :]).squeeze(2)
    (pooled * go.cpu().to(dt)).sum().backward()
    return a.grad, [{k: t.grad for k, t in L.items()} for L in leaves]


def scatter_to_points(torch, grad_feat, idx, n):
    """group_point's backward on the CPU: grad_feat (B, M, ns, C) added into (B, n, C) at idx."""
    Bn, C = grad_feat.shape[0], grad_feat.shape[-1]
    out = torch.zeros((Bn, n, C), dtype=grad_feat.dtype)
    for b in range(Bn):
        out[b].index_add_(0, idx[b].reshape(-1).long().cpu(), grad_feat[b].reshape(-1, C))
    return out


def check_branch_grads(env, store, feats_grad, branches, go):
    """branches: [(G, idx, scopes, feature slice of G's channels, slice of go's channels)] of one
    module whose output is the concatenation of the branches' pooled MLPs. Compares every
    variable's gradient and the gradient of `points` with the float64 chain from G on."""
    pkg, ops, torch, dev = env
    n, C = feats_grad.shape[1], feats_grad.shape[2]
    pts = {dt: torch.zeros((feats_grad.shape[0], n, C), dtype=dt)
           for dt in (torch.float64, torch.float32)}
    for G, idx, scopes, fsl, gsl in branches:
        vals = layer_values(store, scopes)
        masks, out, arg = branch_forward(ops, torch, G, vals, dev)
        ref = {dt: branch_ref(torch, dt, G, vals, masks, arg, go[..., gsl])
               for dt in (torch.float64, torch.float32)}
        for i, s in enumerate(scopes):
            for k, name in VARS:
                got = store[f"{s}/{name}"].grad
                assert got is not None, f"{s}/{name}"
                r64, r32 = (ref[dt][1][i][k] for dt in (torch.float64, torch.float32))
                assert_close(got.reshape(r64.shape), r64, r32, f"{s}/{name} grad")
                if k == "b":
                    assert (got == 0).all()
                else:
                    assert got.abs().max() > 0, f"{s}/{name}"
        for dt in pts:
            pts[dt] += scatter_to_points(torch, ref[dt][0][..., fsl], idx, n)
    assert_close(feats_grad, pts[torch.float64], pts[torch.float32], "grad_points")
    assert feats_grad.abs().max() > 0


def same_moving_averages(torch, store, hand):
    assert sorted(store) == sorted(hand)
    keys = [k for k in store if k.endswith(("moving_mean", "moving_variance"))]
    assert keys
    for k in keys:
        assert torch.equal(store[k], hand[k]), k
    return keys


@pytest.mark.parametrize("group_all", [False, True], ids=["grouped", "group_all"])
def test_sa_module_runs_the_fused_layer(env, cloud, spy, group_all):
    pkg, ops, torch, dev = env
    tu, pu = pkg.tf_util, pkg.pointnet_util
    xyz, feats0 = cloud
    C = int(feats0.shape[2])
    feats = feats0.clone().requires_grad_(True)
    store, hand = tu.ParamStore(seed=5).trainable(dev), tu.ParamStore(seed=5).trainable(dev)
    new_xyz, got, idx = pu.pointnet_sa_module(xyz, feats, NPOINT, RADIUS, NS, SA_MLP, None,
                                              group_all, True, 0.7, "sa1", params=store)
    assert spy.count("mlp_layer_train_pool") == 1 and spy.count("mlp_layer_train") == 1
    assert spy.index("mlp_layer_train") < spy.index("mlp_layer_train_pool")
    assert got.shape == (B, 1 if group_all else NPOINT, SA_MLP[-1])

    # bitwise the unfused composition by hand, on a second store with the same initial values
    del spy[:]
    f2 = feats0.clone().requires_grad_(True)
    if group_all:
        nx, G, idx2, gxyz = pu.sample_and_group_all(xyz, f2)
    else:
        nx, G, idx2, gxyz = pu.sample_and_group(NPOINT, RADIUS, NS, xyz, f2)
    scopes = ["sa1/conv0", "sa1/conv1"]
    layers = tu.torch_layers(hand, scopes, C + 3, SA_MLP)
    want = pu._pool_torch(tu.mlp_train(G, layers, 0.7), "max", gxyz)
    assert "mlp_layer_train_pool" not in spy
    assert torch.equal(new_xyz, nx) and torch.equal(idx, idx2) and torch.equal(got, want)
    assert len(same_moving_averages(torch, store, hand)) == 4
    assert not torch.equal(store["sa1/conv1/bn/moving_mean"], torch.zeros_like(
        store["sa1/conv1/bn/moving_mean"]))

    g = torch.Generator().manual_seed(3)
    go = torch.rand(got.shape, generator=g).to(dev) - 0.3
    (got * go).sum().backward()
    # SSG order [xyz, points]: the features are G's channels 3 ..
    check_branch_grads(env, store, feats.grad, [(G, idx, scopes, slice(3, None), slice(None))], go)


def test_sa_module_msg_runs_the_fused_layer_for_every_scale(env, cloud, spy):
    pkg, ops, torch, dev = env
    tu, pu, tg = pkg.tf_util, pkg.pointnet_util, pkg.tf_grouping
    xyz, feats0 = cloud
    C = int(feats0.shape[2])
    feats = feats0.clone().requires_grad_(True)
    radii, nss, mlps = [0.1, RADIUS], [8, NS], [[16, 32], [16, 40]]
    store, hand = tu.ParamStore(seed=6).trainable(dev), tu.ParamStore(seed=6).trainable(dev)
    new_xyz, got = pu.pointnet_sa_module_msg(xyz, feats, NPOINT, radii, nss, mlps, True, None,
                                             "msg", params=store)
    assert spy.count("mlp_layer_train_pool") == 2 and spy.count("mlp_layer_train") == 2
    assert got.shape == (B, NPOINT, 72)

    del spy[:]
    nx, gps = pu.sample_and_group_msg(NPOINT, radii, nss, xyz, feats0.clone().requires_grad_(True))
    wants, branches, c0 = [], [], 0
    for i, gp in enumerate(gps):
        scopes = [f"msg/conv{i}_0", f"msg/conv{i}_1"]
        layers = tu.torch_layers(hand, scopes, C + 3, mlps[i])
        wants.append(tu.mlp_train(gp, layers, None).max(dim=2).values)
        idx, _ = tg.query_ball_point(radii[i], nss[i], xyz, nx)
        # MSG order [points, xyz]: the features are gp's first C channels
        branches.append((gp, idx, scopes, slice(0, C), slice(c0, c0 + mlps[i][-1])))
        c0 += mlps[i][-1]
    assert "mlp_layer_train_pool" not in spy
    assert torch.equal(new_xyz, nx) and torch.equal(got, torch.cat(wants, dim=-1))
    assert len(same_moving_averages(torch, store, hand)) == 8

    g = torch.Generator().manual_seed(4)
    go = torch.rand(got.shape, generator=g).to(dev) - 0.3
    (got * go).sum().backward()
    check_branch_grads(env, store, feats.grad, branches, go)


def test_other_paths_keep_the_unfused_layers(env, cloud, spy):
    """Other pooling modes, plain stores, autograd without is_training and inference do not call
    the fused op."""
    pkg, ops, torch, dev = env
    tu, pu = pkg.tf_util, pkg.pointnet_util
    xyz, feats = cloud

    def sa(store, is_training, pooling="max", points=feats):
        return pu.pointnet_sa_module(xyz, points, NPOINT, RADIUS, NS, SA_MLP, None, False,
                                     is_training, None, "sa1", pooling=pooling, params=store)[1]

    trainable = tu.ParamStore(seed=5).trainable(dev)
    for pooling in ("avg", "weighted_avg", "max_and_avg"):
        out = sa(trainable, True, pooling)
        assert out.shape[-1] == SA_MLP[-1] * (2 if pooling == "max_and_avg" else 1)
    assert spy.count("mlp_layer_train") == 6 and "mlp_layer_train_pool" not in spy
    del spy[:]
    sa(tu.ParamStore(seed=5), True)                                   # a plain store
    sa(trainable, False, points=feats.clone().requires_grad_(True))  # autograd, not training
    with torch.no_grad():
        sa(trainable, False)                                          # inference
    pu.pointnet_sa_module_msg(xyz, feats, NPOINT, [RADIUS], [NS], [[32, 40]], True, None, "msg",
                              params=tu.ParamStore(seed=5))
    assert "mlp_layer_train_pool" not in spy and "mlp_layer_train" not in spy
    sa(trainable, True)
    assert spy.count("mlp_layer_train_pool") == 1


def test_learning_smoke(env, cloud, spy):
    """test_gpu_mlp_train.test_learning_smoke's loop (one SA module, one FP module, a 1x1 head
    with 4 classes, 30 Adam steps on one fixed batch) with the SA module on the fused layer: the
    cross-entropy after the last step is lower than at step 0."""
    pkg, ops, torch, dev = env
    tu, pu = pkg.tf_util, pkg.pointnet_util
    xyz, feats = cloud
    med = feats.median(dim=1, keepdim=True).values  # labels: a function of the point's features
    labels = ((feats[..., 0] > med[..., 0]).long() * 2 + (feats[..., 1] > med[..., 1]).long()).reshape(-1)
    store = tu.ParamStore(seed=9).trainable(dev)

    def loss_of():
        new_xyz, sa, _ = pu.pointnet_sa_module(xyz, feats, NPOINT, RADIUS, NS, SA_MLP, None, False,
                                               True, None, "sa1", params=store)
        fp = pu.pointnet_fp_module(xyz, new_xyz, feats, sa, FP_MLP, True, None, "fp1", params=store)
        logits = tu.conv1d(fp, 4, 1, "fc2", activation_fn=None, is_training=True, params=store)
        return torch.nn.functional.cross_entropy(logits.reshape(-1, 4), labels)

    loss_of()  # creates every variable
    opt = torch.optim.Adam(store.parameters(), lr=1e-2)
    losses = []
    for _ in range(30):
        opt.zero_grad()
        loss = loss_of()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        last = float(loss_of())
    print("cross-entropy: step 0", losses[0], "after 30 steps", last)
    assert spy.count("mlp_layer_train_pool") == 32
    assert np.isfinite(losses).all() and last < losses[0]
