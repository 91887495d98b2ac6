"""GPU: the training-mode attention layer (torch.ops.pn2.attn_kv_train / _grad, bn_train / _grad;
pn2_attn_kv_reduce, pn2_attn_kv_reduce_grad, pn2_attn_dx_scatter in csrc/attn_train.hip,
pn2_col_sum in csrc/mlp_train.hip) through torch.ops.pn2, the C ABI and the public attention_layer interfaces.

Forward: exact. kv must have the bits of torch.ops.pn2.mlp_layer_train on [wk | wv], att the bits
of torch.ops.pn2.attn_reduce on de-interleaved copies of kv, pmax the bits of x.max(-2), arg the
first sample that attains it, bn_train the bits of mlp_layer_train with an identity weight.

Backward: torch autograd on the CPU over the plain formulas (Dense, reshape(G, C/4, ns, 4),
scores / 2, softmax, weighted sum; the pool as a gather at the `arg` of the forward under test),
evaluated in float64 and in float32. Tolerance, the project's (tests/support.py):

    max |gpu - f64|  <=  max(4 * max |fp32 - f64|,  1e-6 * (1 + max |f64|))

Two GPU kernels that are each within that bound of float64 (pn2_attn_kv_reduce_grad and
pn2_attn_reduce_grad, whose reduction orders differ on purpose) are within twice the bound of
each other: that is what their direct comparison asserts.

Grid caps of the new kernels, each with a case just past it: the specialised forward strides
beyond 16384 wave tasks (2 tasks in flight x 8192 waves), the specialised backward beyond 8192,
the generic kernels beyond 16384 (group, head) pairs, pn2_attn_dx_scatter beyond 2^20 (g, c).
"""
import ctypes
import functools
import importlib

import numpy as np
import pytest

from conftest import PKG_NAME
from support import assert_close, gpu_marks, tolerance

pytestmark = gpu_marks

EPS = 1e-3

# (G, ns, C)
CASES = [
    (5, 32, 64),        # a head spans 2 rows
    (3, 32, 128),       # C = 4 ns: a head is a row
    (3, 32, 256),       # 2 heads per row; the 2C = 512 GEMM width
    (2, 32, 512),       # 4 heads per row; the 2C = 1024 GEMM width
    (4, 16, 64),        # the other specialised ns values
    (2, 64, 128),
    (3, 8, 32),
    (2, 128, 16),
    (3, 3, 8),          # generic path, head blocks cross row ends unevenly
    (2, 5, 12),
    (1, 1, 4),          # a single row
    (2, 200, 8),        # group_all-like
    (2100, 32, 64),     # 16800 wave tasks: past the specialised forward's and backward's caps
    (1030, 32, 64),     # 8240 wave tasks: past the specialised backward's cap only
    (2100, 3, 32),      # 16800 (group, head) pairs: past the generic kernels' cap
]


@pytest.fixture(scope="module")
def env():
    import torch
    pkg = importlib.import_module(PKG_NAME)
    import pn2hip
    return pkg, pn2hip.ops, torch, torch.device("cuda:0")


def make_params(torch, G, ns, C, seed):
    """Drawn as test_gpu_mlp_train_pool.make_params draws: x in [-1, 1], glorot weights, biases
    in +-0.1 (non-zero), incoming gradients in [-1, 1]; float32 values."""
    g = torch.Generator().manual_seed(seed)
    u = lambda lo, hi, *s: torch.rand(*s, generator=g, dtype=torch.float64) * (hi - lo) + lo  # noqa: E731
    lim = float(np.sqrt(6.0 / (C + C)))
    p = {"x": u(-1, 1, G, ns, C), "go": u(-1, 1, G, C), "gp": u(-1, 1, G, C)}
    for n in "qkv":
        p["w" + n] = u(-lim, lim, C, C)
        p["b" + n] = u(-0.1, 0.1, C)
    return {k: v.float() for k, v in p.items()}


LEAVES = ("x", "wq", "bq", "wk", "bk", "wv", "bv")


def reduce_ref(torch, q, K, V):
    """attention_layer.py:35-42 with key_dim = output_dim = 4 on q (G, C), K, V (G, ns, C)."""
    G, ns, C = K.shape
    Kh, Vh = K.reshape(G, C // 4, ns, 4), V.reshape(G, C // 4, ns, 4)   # the reshape quirk
    s = (Kh * q.reshape(G, C // 4, 1, 4)).sum(-1) / 2
    a = torch.softmax(s, dim=-1)
    return (a[..., None] * Vh).sum(2).reshape(G, C)


def ref_grads(torch, p, dt, arg):
    """Gradients of sum(go * att) + sum(gp * pmax) in dtype dt on the CPU."""
    L = {k: p[k].to(dt).clone().requires_grad_(True) for k in LEAVES}
    x = L["x"]
    att = reduce_ref(torch, x[:, 0] @ L["wq"] + L["bq"], x @ L["wk"] + L["bk"],
                     x @ L["wv"] + L["bv"])
    pooled = x.gather(1, arg.long()[:, None, :]).squeeze(1)
    ((att * p["go"].to(dt)).sum() + (pooled * p["gp"].to(dt)).sum()).backward()
    return {k: v.grad for k, v in L.items()}


def reduce_ref_grads(torch, q, K, V, go, dt):
    L = [t.detach().cpu().to(dt).clone().requires_grad_(True) for t in (q, K, V)]
    (reduce_ref(torch, *L) * go.detach().cpu().to(dt)).sum().backward()
    return [t.grad for t in L]


def kv_reduce_grad_c(pkg, torch, q, kv, go):
    """pn2_attn_kv_reduce_grad through ctypes, outputs pre-filled with NaN."""
    G, ns, C2 = kv.shape
    gq = torch.full_like(q, float("nan"))
    gkv = torch.full_like(kv, float("nan"))
    pkg._lib.check(pkg.lib().pn2_attn_kv_reduce_grad(
        q.data_ptr(), kv.data_ptr(), go.data_ptr(), G, ns, C2 // 2, gq.data_ptr(),
        gkv.data_ptr(), pkg._lib.stream_of(q)), "attn_kv_reduce_grad")
    return gq, gkv


@functools.lru_cache(maxsize=None)
def run_case(case):
    """Forward + backward of one case on the GPU and the references, once."""
    import torch
    import pn2hip
    pkg = importlib.import_module(PKG_NAME)
    ops, dev = pn2hip.ops, torch.device("cuda:0")
    G, ns, C = case
    p = make_params(torch, G, ns, C, seed=G * 31 + ns * 7 + C)
    d = {k: v.to(dev) for k, v in p.items()}
    w = [d[k] for k in ("wq", "bq", "wk", "bk", "wv", "bv")]
    fwd = ops.attn_kv_train(d["x"], *w, True)
    att, pmax, arg, q, kv = fwd
    grads = ops.attn_kv_train_grad(d["go"], d["gp"], arg, d["x"], d["wq"], d["wk"], d["wv"], q,
                                   kv, True)
    c_grads = kv_reduce_grad_c(pkg, torch, q, kv, d["go"])
    torch.cuda.synchronize()
    bwd = {dt: ref_grads(torch, p, dt, arg.cpu()) for dt in (torch.float64, torch.float32)}
    return p, d, fwd, grads, c_grads, bwd


def ids(case):
    return "x".join(str(int(v)) for v in case)


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_forward_is_exact(env, case):
    pkg, ops, torch, dev = env
    G, ns, C = case
    p, d, (att, pmax, arg, q, kv), _, _, _ = run_case(case)
    assert att.shape == pmax.shape == arg.shape == q.shape == (G, C) and kv.shape == (G, ns, 2 * C)
    assert arg.dtype == torch.int32
    wkv, bkv = torch.cat([d["wk"], d["wv"]], 1), torch.cat([d["bk"], d["bv"]])
    assert torch.equal(kv, ops.mlp_layer_train(d["x"], wkv, bkv, None, None, EPS, False)[0])
    assert torch.equal(q, ops.mlp_layer_train(d["x"][:, 0].contiguous(), d["wq"], d["bq"], None,
                                              None, EPS, False)[0])
    K, V = kv[..., :C].contiguous(), kv[..., C:].contiguous()
    assert torch.equal(att, ops.attn_reduce(q[None], K[None], V[None])[0])
    assert torch.equal(pmax, d["x"].max(-2).values)
    want = np.argmax(p["x"].numpy(), axis=1).astype(np.int32)   # numpy: the first maximum
    got = arg.cpu().numpy()
    assert np.array_equal(got, want), f"{(got != want).sum()} of {got.size} arg differ"
    # without the pool: the same att, q and kv, 0-element pmax and arg
    att2, pmax2, arg2, q2, kv2 = ops.attn_kv_train(
        d["x"], *[d[k] for k in ("wq", "bq", "wk", "bk", "wv", "bv")], False)
    assert torch.equal(att2, att) and torch.equal(q2, q) and torch.equal(kv2, kv)
    assert pmax2.shape == arg2.shape == (0,) and arg2.dtype == torch.int32
    # against float64 too (the fp32 reference sets the bound)
    r = {dt: reduce_ref(torch, q.cpu().to(dt), K.cpu().to(dt), V.cpu().to(dt))
         for dt in (torch.float64, torch.float32)}
    assert_close(att, r[torch.float64], r[torch.float32], "att")


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_reduction_gradient_c_abi(env, case):
    """pn2_attn_kv_reduce_grad writes every element of grad_Q and grad_KV; de-interleaved they
    agree with float64 and with pn2_attn_reduce_grad."""
    pkg, ops, torch, dev = env
    G, ns, C = case
    _, d, (att, pmax, arg, q, kv), _, (gq, gkv), _ = run_case(case)
    assert not torch.isnan(gq).any() and not torch.isnan(gkv).any()
    K, V = kv[..., :C].contiguous(), kv[..., C:].contiguous()
    old = ops.attn_reduce_grad(q[None], K[None], V[None], d["go"][None])
    r64 = reduce_ref_grads(torch, q, K, V, d["go"], torch.float64)
    r32 = reduce_ref_grads(torch, q, K, V, d["go"], torch.float32)
    new = (gq, gkv[..., :C], gkv[..., C:])
    for name, n, o, a, b in zip(("grad_Q", "grad_K", "grad_V"), new, old, r64, r32):
        assert_close(n, a, b, name)
        assert_close(o[0], a, b, name + " (attn_reduce_grad)")
        tol, _ = tolerance(a, b)
        diff = float((n - o[0]).abs().max())
        assert diff <= 2 * tol, f"{name}: the two kernels differ by {diff:.3g} > {2 * tol:.3g}"


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_backward(env, case):
    pkg, ops, torch, dev = env
    _, _, _, grads, _, bwd = run_case(case)
    r64, r32 = bwd[torch.float64], bwd[torch.float32]
    assert len(grads) == 7
    for got, k in zip(grads, LEAVES):
        assert_close(got, r64[k], r32[k], "grad_" + k)
        # (one pseudo-key: the softmax is the constant 1, the query and key gradients vanish)
        if case[1] > 1 or k in ("x", "wv", "bv"):
            assert got.abs().max() > 0, k


def test_need_grad_x_false_and_autograd(env):
    """need_grad_x=False skips grad_x (a 0-element tensor) and leaves the other six gradients'
    bits; the registered autograd returns the op's own gradients, with and without the pool."""
    pkg, ops, torch, dev = env
    case = (5, 32, 64)
    p, d, (att, pmax, arg, q, kv), grads, _, _ = run_case(case)
    no_x = ops.attn_kv_train_grad(d["go"], d["gp"], arg, d["x"], d["wq"], d["wk"], d["wv"], q, kv,
                                  False)
    assert no_x[0].shape == (0,)
    for a, b in zip(no_x[1:], grads[1:]):
        assert torch.equal(a, b)
    for add_max in (True, False):
        L = {k: d[k].clone().requires_grad_(True) for k in LEAVES}
        out = ops.attn_kv_train(*[L[k] for k in LEAVES], add_max)
        assert not (out[2].requires_grad or out[3].requires_grad or out[4].requires_grad)
        loss = (out[0] * d["go"]).sum()
        if add_max:
            loss = loss + (out[1] * d["gp"]).sum()
        loss.backward()
        want = grads if add_max else ops.attn_kv_train_grad(
            d["go"], None, out[2], d["x"], d["wq"], d["wk"], d["wv"], q, kv, True)
        for k, g in zip(LEAVES, want):
            assert torch.equal(L[k].grad, g), (k, add_max)
    # x without a gradient: the variables' gradients only
    L = {k: d[k].clone().requires_grad_(k != "x") for k in LEAVES}
    (ops.attn_kv_train(*[L[k] for k in LEAVES], True)[0] * d["go"]).sum().backward()
    assert L["x"].grad is None and torch.equal(L["wk"].grad, no_x[3])


@pytest.mark.parametrize("case", [(3, 32, 256), (2, 5, 12), (2100, 32, 64)], ids=ids)
def test_deterministic(env, case):
    pkg, ops, torch, dev = env
    _, d, fwd, grads, _, _ = run_case(case)
    w = [d[k] for k in ("wq", "bq", "wk", "bk", "wv", "bv")]
    for _ in range(2):
        again = ops.attn_kv_train(d["x"], *w, True)
        for a, b in zip(again, fwd):
            assert torch.equal(a, b)
        g2 = ops.attn_kv_train_grad(d["go"], d["gp"], again[2], d["x"], d["wq"], d["wk"], d["wv"],
                                    again[3], again[4], True)
        for a, b in zip(g2, grads):
            assert torch.equal(a, b)


def test_empty_input(env):
    pkg, ops, torch, dev = env
    z = lambda *s: torch.zeros(s, device=dev)  # noqa: E731
    att, pmax, arg, q, kv = ops.attn_kv_train(z(0, 5, 8), z(8, 8), z(8), z(8, 8), z(8), z(8, 8),
                                              z(8), True)
    assert att.shape == pmax.shape == arg.shape == (0, 8) and kv.shape == (0, 5, 16)
    grads = ops.attn_kv_train_grad(att, pmax, arg, z(0, 5, 8), z(8, 8), z(8, 8), z(8, 8), q, kv,
                                   True)
    assert grads[0].shape == (0, 5, 8)
    for g in grads[1:]:
        assert (g == 0).all()
    out, mean, var = ops.bn_train(z(0, 8), z(8), z(8), EPS, False)
    assert out.shape == (0, 8) and (mean == 0).all() and (var == 0).all()


# ------------------------------------------------------------------ bn_train ---------------
# (leading shape, C, relu)
BN_CASES = [((5, 7), 4, False), ((37,), 33, True), ((3, 11), 512, False), ((1,), 33, False),
            ((2100,), 4, True)]


@pytest.mark.parametrize("lead,C,relu", BN_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_bn_train(env, lead, C, relu):
    pkg, ops, torch, dev = env
    g = torch.Generator().manual_seed(C * 13 + lead[0])
    u = lambda lo, hi, *s: (torch.rand(*s, generator=g, dtype=torch.float64) * (hi - lo) + lo).float()  # noqa: E731
    x, go = u(-1, 1, *lead, C), u(-1, 1, *lead, C)
    mag, sign = u(0.5, 1.5, C), u(-1, 1, C)
    gamma, beta = torch.where(sign < 0, -mag, mag), u(-0.2, 0.2, C)
    if C > 4:
        assert 0 < int((gamma < 0).sum()) < C
    dx, dgo, dgamma, dbeta = (t.to(dev) for t in (x, go, gamma, beta))
    out, mean, var = ops.bn_train(dx, dgamma, dbeta, EPS, relu)
    out0, y0, mean0, var0 = ops.mlp_layer_train(dx, torch.eye(C, device=dev), None, dgamma, dbeta,
                                                EPS, relu)
    assert torch.equal(y0, dx)     # the identity GEMM returns x exactly
    assert torch.equal(out, out0) and torch.equal(mean, mean0) and torch.equal(var, var0)
    if lead == (1,):
        assert (var == 0).all() and torch.equal(mean, dx[0])
    gx, gg, gb = ops.bn_train_grad(dgo, dx, mean, var, dgamma, dbeta, EPS, relu)
    mask = (out > 0).cpu()

    def ref(dt):
        L = [t.to(dt).clone().requires_grad_(True) for t in (x, gamma, beta)]
        flat = L[0].reshape(-1, C)
        z = (L[0] - flat.mean(0)) * (L[1] / torch.sqrt(flat.var(0, unbiased=False) + EPS)) + L[2]
        if relu:
            z = z * mask.to(dt)
        (z * go.to(dt)).sum().backward()
        return [t.grad for t in L]
    r64, r32 = ref(torch.float64), ref(torch.float32)
    for name, got, a, b in zip(("grad_x", "grad_gamma", "grad_beta"), (gx, gg, gb), r64, r32):
        assert_close(got, a, b, name)
    # autograd returns the op's own gradients
    L = [t.clone().requires_grad_(True) for t in (dx, dgamma, dbeta)]
    (ops.bn_train(*L, EPS, relu)[0] * dgo).sum().backward()
    for t, want in zip(L, (gx, gg, gb)):
        assert torch.equal(t.grad, want)


# ------------------------------------------------------------------ C helpers --------------
@pytest.mark.parametrize("G,ns,C,pool", [(7, 5, 12, True), (7, 5, 12, False), (1, 1, 4, True),
                                         (2100, 2, 512, True)],
                         ids=lambda v: str(v))
def test_dx_scatter_is_exact(env, G, ns, C, pool):
    """In place, float32, the query row first and the pooled gradient second; arg = -1 and
    arg = ns select nothing (and are never dereferenced); arg = 0 adds twice to one element."""
    pkg, ops, torch, dev = env
    rng = np.random.default_rng(G * 7 + C)
    gx = rng.uniform(-1, 1, (G, ns, C)).astype(np.float32)
    gxq = rng.uniform(-1, 1, (G, C)).astype(np.float32)
    gp = rng.uniform(-1, 1, (G, C)).astype(np.float32)
    arg = rng.integers(-1, ns + 1, (G, C)).astype(np.int32)
    arg.reshape(-1)[:4] = [-1, ns, 0, ns - 1]
    assert (arg == -1).any() and (arg == ns).any() and (arg == 0).any()
    want = gx.copy()
    want[:, 0, :] = want[:, 0, :] + gxq
    if pool:
        gi, ci = np.nonzero((arg >= 0) & (arg < ns))
        want[gi, arg[gi, ci], ci] = want[gi, arg[gi, ci], ci] + gp[gi, ci]
    t = {k: torch.from_numpy(v).to(dev) for k, v in dict(gx=gx, gxq=gxq, gp=gp, arg=arg).items()}
    pkg._lib.check(pkg.lib().pn2_attn_dx_scatter(
        t["gx"].data_ptr(), t["gxq"].data_ptr(), t["gp"].data_ptr() if pool else None,
        t["arg"].data_ptr() if pool else None, G, ns, C, pkg._lib.stream_of(t["gx"])), "dx_scatter")
    torch.cuda.synchronize()
    assert np.array_equal(t["gx"].cpu().numpy(), want)


@pytest.mark.parametrize("rows,C", [(1, 4), (37, 33), (1024, 32), (1025, 64), (9000, 130)])
def test_col_sum(env, rows, C):
    """Within the project's tolerance of the float64 sum, equal bits on a second run, and no
    element of the workspace beyond pn2_col_sum_workspace_size touched."""
    pkg, ops, torch, dev = env
    g = torch.Generator().manual_seed(rows + C)
    x = torch.rand(rows, C, generator=g) * 2 - 1
    dx = x.to(dev)
    ws = pkg.lib().pn2_col_sum_workspace_size(rows, C)
    assert ws == -(-rows // 1024) * C * 4
    outs = []
    for _ in range(2):
        work = torch.full((ws // 4 + 8,), 7.0, device=dev)
        out = torch.full((C,), float("nan"), device=dev)
        pkg._lib.check(pkg.lib().pn2_col_sum(dx.data_ptr(), rows, C, out.data_ptr(),
                                             work.data_ptr(), ws, pkg._lib.stream_of(dx)), "col_sum")
        torch.cuda.synchronize()
        assert (work[ws // 4:] == 7.0).all()
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    assert_close(outs[0], x.double().sum(0), x.sum(0), "col_sum")


# ------------------------------------------------------------------ the SA modules ---------
B, N, NPOINT, RADIUS, NS = 2, 512, 64, 0.2, 16
MLP = [32, 64]
DECAY = 0.7


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
    monkeypatch.setattr(pkg.attention_layer, "call", call)
    return names


def hand_module(env, hand, xyz, feats, scope, mlp2, group_all, and_pooling):
    """The module op by op: torch.ops.pn2 calls on the store `hand`, the moving averages updated
    by the rule m <- decay * m + (1 - decay) * batch statistic."""
    pkg, ops, torch, dev = env
    tu, pu = pkg.tf_util, pkg.pointnet_util

    def move(p, mean, var):
        with torch.no_grad():
            p["moving_mean"].mul_(DECAY).add_((1 - DECAY) * mean)
            p["moving_variance"].mul_(DECAY).add_((1 - DECAY) * var)

    def conv_layers(h, scopes, cin, widths):
        for s, w in zip(scopes, widths):
            p = hand.conv(s, cin, w)
            h, _, mean, var = ops.mlp_layer_train(h, p["weights"], p["biases"], p["gamma"],
                                                  p["beta"], EPS, True)
            move(p, mean, var)
            cin = w
        return h

    if group_all:
        nx, G, idx, _ = pu.sample_and_group_all(xyz, feats)
    else:
        nx, G, idx, _ = pu.sample_and_group(NPOINT, RADIUS, NS, xyz, feats)
    C = MLP[-1]
    X = conv_layers(G, [f"{scope}/conv{i}" for i in range(len(MLP))], int(G.shape[-1]), MLP)
    base = f"{scope}/ScannetAttentionLayer"
    d = [hand.dense(f"{base}/{n}", C, C) for n in ("dense", "dense_1", "dense_2")]
    att, pmax = ops.attn_kv_train(X, d[0]["weights"], d[0]["biases"], d[1]["weights"],
                                  d[1]["biases"], d[2]["weights"], d[2]["biases"], and_pooling)[:2]
    p = hand.bn(f"{scope}/{scope}", C)
    out, mean, var = ops.bn_train(att, p["gamma"], p["beta"], EPS, False)
    move(p, mean, var)
    if and_pooling:
        out = out + pmax
    if mlp2:
        out = conv_layers(out, [f"{scope}/conv_post_{i}" for i in range(len(mlp2))], C, mlp2)
    return nx, out, idx, (mean, var)


@pytest.mark.parametrize("and_pooling", [False, True], ids=["attention", "and_pooling"])
@pytest.mark.parametrize("mlp2,group_all", [(None, False), ([48], False), (None, True)],
                         ids=["plain", "mlp2", "group_all"])
def test_sa_attention_modules_train_on_the_hip_layers(env, cloud, spy, mlp2, group_all,
                                                      and_pooling):
    pkg, ops, torch, dev = env
    tu, al = pkg.tf_util, pkg.attention_layer
    xyz, feats0 = cloud
    module = al.pointnet_sa_module_attention_and_pooling if and_pooling else \
        al.pointnet_sa_module_attention
    store, hand = tu.ParamStore(seed=5).trainable(dev), tu.ParamStore(seed=5).trainable(dev)
    feats = feats0.clone().requires_grad_(True)
    new_xyz, got, idx = module(xyz, feats, NPOINT, RADIUS, NS, MLP, mlp2, group_all, True, DECAY,
                               "sa", params=store)
    assert spy.count("attn_kv_train") == 1 and spy.count("bn_train") == 1
    assert spy.count("mlp_layer_train") == len(MLP) + len(mlp2 or [])
    assert "attn_reduce" not in spy
    assert got.shape == (B, 1 if group_all else NPOINT, (mlp2 or MLP)[-1])

    f2 = feats0.clone().requires_grad_(True)
    nx, want, idx2, (mean, var) = hand_module(env, hand, xyz, f2, "sa", mlp2, group_all,
                                              and_pooling)
    assert torch.equal(new_xyz, nx) and torch.equal(idx, idx2) and torch.equal(got, want)

    # variables: the TF names, 2 x 4 conv + 3 x 2 dense + gamma, beta (+ 4 for mlp2)
    assert sorted(store) == sorted(hand)
    assert len(list(store.parameters())) == 16 + (4 if mlp2 else 0)
    for n in ("dense", "dense_1", "dense_2"):
        assert f"sa/ScannetAttentionLayer/{n}/kernel" in store
        assert f"sa/ScannetAttentionLayer/{n}/bias" in store
    moving = [k for k in store if k.endswith(("moving_mean", "moving_variance"))]
    assert len(moving) == 6 + (2 if mlp2 else 0)
    for k in moving:
        assert torch.equal(store[k], hand[k]), k
        assert store[k].device.type == "cuda" and not store[k].requires_grad
    # the rule, spelled out for the batch norm after the attention (initial mean 0, variance 1)
    assert torch.allclose(store["sa/sa/moving_mean"], (1 - DECAY) * mean, rtol=1e-6, atol=1e-9)
    assert torch.allclose(store["sa/sa/moving_variance"], DECAY + (1 - DECAY) * var, rtol=1e-6)
    assert float(var.max()) > 0

    g = torch.Generator().manual_seed(3)
    go = torch.rand(got.shape, generator=g).to(dev) - 0.3
    (got * go).sum().backward()
    (want * go).sum().backward()
    for k in store:
        if k in moving:
            continue
        a, b = store[k].grad, hand[k].grad
        assert a is not None and b is not None, k
        assert torch.equal(a, b), k
        if not k.endswith("biases"):   # a conv bias under batch norm has a zero gradient
            assert a.abs().max() > 0, k
    # the gradient of `points` leaves group_point's backward, which adds with float atomics in
    # no fixed order: the same addends (at most NPOINT * NS = 1024 per point, bit-equal up to
    # there), so two runs differ by at most 1024 * 2^-24 = 6e-5 of the sum of their magnitudes
    top = float(feats.grad.abs().max())
    assert top > 0
    assert float((feats.grad - f2.grad).abs().max()) <= 1e-4 * top

    # one optimiser step, then inference: the trainable store's refreshed packed cache against a
    # plain store of the same values on the fused inference kernel
    opt = torch.optim.Adam(store.parameters(), lr=1e-3)
    before = store["sa/ScannetAttentionLayer/dense_1/kernel"].detach().clone()
    opt.step()
    assert not torch.equal(before, store["sa/ScannetAttentionLayer/dense_1/kernel"].detach())
    del spy[:]
    # (the fused inference kernel keeps a group in one workgroup and takes these widths up to
    # nsample = 32: group_all infers on the cloud's first 32 points)
    n_inf = 32 if group_all else N
    xi, fi = xyz[:, :n_inf].contiguous(), feats0[:, :n_inf].contiguous()
    with torch.no_grad():
        _, inf, _ = module(xi, fi, NPOINT, RADIUS, NS, MLP, mlp2, group_all, False, None, "sa",
                           params=store)
        assert "attn_kv_train" not in spy and "bn_train" not in spy
        plain = tu.ParamStore(store.state_dict())
        assert not plain.is_trainable
        _, inf2, _ = module(xi, fi, NPOINT, RADIUS, NS, MLP, mlp2, group_all, False, None, "sa",
                            params=plain)
    np.testing.assert_allclose(inf.cpu().numpy(), inf2.cpu().numpy(), rtol=1e-4, atol=2e-5)


def test_plain_store_keeps_the_torch_composition(env, cloud, spy):
    """is_training=True on a store that is not trainable runs the differentiable torch
    composition as before: none of the new ops, moving averages on the CPU. Its output is the
    same mathematics as the HIP training path on the same initial values. Bound: fp32 rounding
    (about 1e-6 relative per product) can be amplified by each of the three batch norms by at
    most 1 / sqrt(eps) = 32, reached only where a channel's variance vanishes; 1e-4 + 1e-3 |x|
    leaves two decimal orders over the typical case."""
    pkg, ops, torch, dev = env
    tu, al = pkg.tf_util, pkg.attention_layer
    xyz, feats = cloud
    plain = tu.ParamStore(seed=5)
    args = (xyz, feats, NPOINT, RADIUS, NS, MLP, None, False, True, DECAY, "sa")
    _, got, _ = al.pointnet_sa_module_attention_and_pooling(*args, params=plain)
    assert "attn_reduce" in spy
    for name in ("attn_kv_train", "bn_train", "mlp_layer_train"):
        assert name not in spy
    assert not plain.is_trainable and not list(plain.parameters())
    assert plain["sa/sa/moving_mean"].device.type == "cpu"
    assert float(plain["sa/sa/moving_mean"].abs().max()) > 0
    store = tu.ParamStore(seed=5).trainable(dev)
    _, want, _ = al.pointnet_sa_module_attention_and_pooling(*args, params=store)
    err = float((got.detach() - want.detach()).abs().max())
    print(f"torch composition vs HIP training path: max |diff| {err:.3g}")
    np.testing.assert_allclose(got.detach().cpu().numpy(), want.detach().cpu().numpy(), rtol=1e-3,
                               atol=1e-4)
    np.testing.assert_allclose(plain["sa/sa/moving_variance"].numpy(),
                               store["sa/sa/moving_variance"].cpu().numpy(), rtol=1e-3, atol=1e-5)


def test_knn_grouping_trains_too(env, cloud, spy):
    pkg, ops, torch, dev = env
    tu, al = pkg.tf_util, pkg.attention_layer
    xyz, feats = cloud
    store = tu.ParamStore(seed=8).trainable(dev)
    _, out, _ = al.pointnet_sa_module_attention(xyz, feats, NPOINT, RADIUS, NS, MLP, None, False,
                                                True, None, "sa", knn=True, params=store)
    assert spy.count("attn_kv_train") == 1 and out.shape == (B, NPOINT, MLP[-1])
    out.sum().backward()
    assert store["sa/ScannetAttentionLayer/dense/kernel"].grad.abs().max() > 0
