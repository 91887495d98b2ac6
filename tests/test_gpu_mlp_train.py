"""GPU: the training-mode shared-MLP layer (csrc/mlp_train.hip) through torch.ops.pn2 and the
public tf_util / pointnet_util interfaces.

Reference: torch float64 on the CPU with the formulas of tf_util.mlp_torch(is_training=True)
(conv + bias, batch mean and BIASED variance over the rows, gamma / sqrt(var + 1e-3), ReLU),
and its autograd. Tolerance (the project's, tests/support.py):

    max |gpu - f64|  <=  max(4 * max |fp32 - f64|,  1e-6 * (1 + max |f64|))

where fp32 is the same reference function evaluated in float32 on the CPU.

A ReLU that flips at a pre-activation within rounding of zero is a discrete difference, not an
error, so the backward references multiply by the mask `out_gpu > 0` of the forward output
under test (which the forward tests have validated) instead of applying their own ReLU.
"""
import importlib

import numpy as np
import pytest

from conftest import PKG_NAME
from mlp_train_ref import (B, EPS, FP_MLP, N, NPOINT, NS, RADIUS, SA_MLP, SLAB, bn_act_bwd,
                           ids, make_params, ref_layer, run_case, sa_fp)
from support import assert_close, gpu_marks

pytestmark = gpu_marks

# (rows, cin, cout, batch norm, relu)
CASES = [
    (1000, 3, 32, True, True),
    (33, 9, 64, True, True),
    (77, 259, 256, True, True),
    (64, 768, 256, True, True),
    (4099, 128, 21, False, False),
    (5, 1030, 1024, False, True),
    (1, 16, 32, True, True),          # a single row: zero variance
    (2, 3, 32, True, True),
    (300, 67, 96, True, False),
    (SLAB - 1, 16, 32, True, True),   # one below / above the wgrad slab and the stats block
    (SLAB + 1, 16, 32, True, True),
    (2 * SLAB - 1, 40, 33, True, True),
    (2 * SLAB + 1, 40, 33, False, True),
    (70, 20, 200, True, True),        # 7 output tiles: a last tile group of 3 of 4
]


@pytest.fixture(scope="module")
def env():
    import torch
    pkg = importlib.import_module(PKG_NAME)
    import pn2hip
    return pkg, pn2hip.ops, torch, torch.device("cuda:0")


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_layer_forward(env, case):
    pkg, ops, torch, dev = env
    _, _, (out, y, mean, var), _, fwd, _ = run_case(case)
    r64, r32 = fwd[torch.float64], fwd[torch.float32]
    assert_close(y, r64[1], r32[1], "y")
    assert_close(out, r64[0], r32[0], "out")
    if case[3]:
        assert_close(mean, r64[2], r32[2], "mean")
        assert_close(var, r64[3], r32[3], "var")
        assert (var >= 0).all()
    else:
        assert mean.numel() == 0 and var.numel() == 0


def test_variance_survives_cancellation(env):
    """Channel means of y at +-50 with a spread near 1: E[y^2] - E[y]^2 in fp32 would lose the
    variance (50^2 * 2^-24 ~ 1.5e-4 per term against a tolerance of ~2e-6)."""
    pkg, ops, torch, dev = env
    rows, cin, cout = 4099, 32, 64
    bias = torch.where(torch.arange(cout) % 2 == 0, 50.0, -50.0).float()
    p = make_params(torch, rows, cin, cout, True, seed=7, bias=bias)
    # xavier weights over 32 inputs in [-1, 1]: the spread of y is below 1; scale it to ~1
    p["w"] = (p["w"] * 2.0).float()
    r64 = ref_layer(torch, p, torch.float64, True)[0]
    r32 = ref_layer(torch, p, torch.float32, True)[0]
    assert 45 < r64[2].abs().min() and r64[2].abs().max() < 55
    assert 0.5 < r64[3].min() and r64[3].max() < 2.0
    # the fp32 yardstick itself is meaningful here: finite and not identically exact
    e32 = (r32[3].double() - r64[3]).abs().max().item()
    assert np.isfinite(e32) and e32 > 0
    d = {k: None if v is None else v.to(dev) for k, v in p.items()}
    out, y, mean, var = ops.mlp_layer_train(d["x"], d["w"], d["b"], d["gamma"], d["beta"], EPS, True)
    assert_close(mean, r64[2], r32[2], "mean")
    assert_close(var, r64[3], r32[3], "var")
    assert_close(out, r64[0], r32[0], "out")


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_layer_backward(env, case):
    pkg, ops, torch, dev = env
    _, _, _, (gx, gw, gb, gg, gbeta), _, bwd = run_case(case)
    r64, r32 = bwd[torch.float64], bwd[torch.float32]
    assert_close(gx, r64["x"], r32["x"], "grad_x")
    assert_close(gw, r64["w"], r32["w"], "grad_w")
    assert_close(gb, r64["b"], r32["b"], "grad_b")
    if case[3]:
        assert (gb == 0).all()  # the batch mean absorbs the bias
        assert_close(gg, r64["gamma"], r32["gamma"], "grad_gamma")
        assert_close(gbeta, r64["beta"], r32["beta"], "grad_beta")
    else:
        assert gg.numel() == 0 and gbeta.numel() == 0


@pytest.mark.parametrize("case", [c for c in CASES if c[4]], ids=ids)
def test_backward_mask_is_the_forward_mask(env, case):
    """The backward recomputes the ReLU mask from y; it must equal out > 0 exactly. Without
    batch norm grad_y = dz, so grad_y is exactly 0 wherever out == 0. With batch norm grad_y
    also carries the batch-mean terms (-grad_beta / R - xhat * grad_gamma / R) at every
    element, so the mask is isolated through dz instead: a grad_out that is non-zero only where
    out == 0 must give dz == 0 everywhere, i.e. grad_y, grad_gamma and grad_beta all exactly 0;
    and a grad_out that is non-zero only where out > 0 must lose nothing: grad_beta equals the
    column sums of that grad_out (within the tolerance)."""
    pkg, ops, torch, dev = env
    p, d, (out, y, mean, var), _, _, _ = run_case(case)
    bn = case[3]
    dead = out == 0
    if not bn:
        gy, _, _ = bn_act_bwd(pkg, torch, d["go"], y, None, None, None, None, True)
        assert (gy[dead] == 0).all()
        assert torch.equal(gy[~dead], d["go"][~dead])
        return
    go_dead = torch.where(dead, d["go"], torch.zeros_like(d["go"]))
    gy, gg, gbeta = bn_act_bwd(pkg, torch, go_dead, y, mean, var, d["gamma"], d["beta"], True)
    assert (gy == 0).all() and (gg == 0).all() and (gbeta == 0).all()
    go_live = d["go"] - go_dead
    _, _, gbeta = bn_act_bwd(pkg, torch, go_live, y, mean, var, d["gamma"], d["beta"], True)
    assert_close(gbeta, go_live.cpu().double().sum(0), go_live.cpu().sum(0), "grad_beta (live)")


def test_chain_through_autograd(env):
    """Three layers (1000, 9, [32, 32, 64]) run op by op through autograd."""
    pkg, ops, torch, dev = env
    rows, cin, widths = 1000, 9, [32, 32, 64]
    ps, c = [], cin
    for i, w in enumerate(widths):
        ps.append(make_params(torch, rows, c, w, True, seed=100 + i))
        c = w
    x0, go = ps[0]["x"], ps[-1]["go"]
    leaves = [{k: v.to(dev).requires_grad_(True) for k, v in p.items() if k in ("w", "b", "gamma", "beta")}
              for p in ps]
    xg = x0.to(dev).requires_grad_(True)
    h, masks = xg, []
    for L in leaves:
        h, y, mean, var = ops.mlp_layer_train(h, L["w"], L["b"], L["gamma"], L["beta"], EPS, True)
        assert not y.requires_grad and not mean.requires_grad and not var.requires_grad
        masks.append((h > 0).cpu())
    (h * go.to(dev)).sum().backward()

    def ref(dt):
        rl = [{k: p[k].to(dt).clone().requires_grad_(True) for k in ("w", "b", "gamma", "beta")} for p in ps]
        rx = x0.to(dt).clone().requires_grad_(True)
        a = rx
        for L, m in zip(rl, masks):
            y = a @ L["w"] + L["b"]
            a = ((y - y.mean(0)) * (L["gamma"] / torch.sqrt(y.var(0, unbiased=False) + EPS)) + L["beta"]) * m.to(dt)
        (a * go.to(dt)).sum().backward()
        return a, rx, rl

    a64, x64, l64 = ref(torch.float64)
    a32, x32, l32 = ref(torch.float32)
    assert_close(h, a64, a32, "out")
    assert_close(xg.grad, x64.grad, x32.grad, "grad_x")
    for i, (L, r64, r32) in enumerate(zip(leaves, l64, l32)):
        for k in ("w", "gamma", "beta", "b"):
            assert_close(L[k].grad, r64[k].grad, r32[k].grad, f"layer {i} grad_{k}")


def test_deterministic(env):
    pkg, ops, torch, dev = env
    p = make_params(torch, 4099, 128, 128, True, seed=11)
    d = {k: v.to(dev) for k, v in p.items()}

    def run():
        f = ops.mlp_layer_train(d["x"], d["w"], d["b"], d["gamma"], d["beta"], EPS, True)
        g = ops.mlp_layer_train_grad(d["go"], d["x"], d["w"], f[1], f[2], f[3], d["gamma"],
                                     d["beta"], EPS, True, True)
        return list(f) + list(g)

    a, b = run(), run()
    for i, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(u, v), f"output {i} differs between two runs"


def test_need_grad_x_false(env):
    pkg, ops, torch, dev = env
    _, d, (out, y, mean, var), full, _, _ = run_case(CASES[0])
    part = ops.mlp_layer_train_grad(d["go"], d["x"], d["w"], y, mean, var, d["gamma"], d["beta"],
                                    EPS, True, False)
    assert part[0].numel() == 0
    for i in range(1, 5):
        assert torch.equal(part[i], full[i]), i
    # through autograd: an input that needs no gradient gets none, the variables get theirs
    w = d["w"].clone().requires_grad_(True)
    o = ops.mlp_layer_train(d["x"], w, d["b"], d["gamma"], d["beta"], EPS, True)[0]
    (o * d["go"]).sum().backward()
    assert torch.equal(w.grad, full[1])


# ------------------------------------------------------------------- modules --------------

@pytest.fixture(scope="module")
def cloud(env):
    pkg, ops, torch, dev = env
    xyz, feats = pkg.synth.batch([0, 1], N, "scannet", with_features=True)
    return torch.from_numpy(xyz).to(dev), torch.from_numpy(feats).to(dev)


def test_modules_train_on_a_trainable_store(env, cloud):
    pkg, ops, torch, dev = env
    tu, pu = pkg.tf_util, pkg.pointnet_util
    xyz, feats0 = cloud
    C = int(feats0.shape[2])
    feats = feats0.clone().requires_grad_(True)
    store = tu.ParamStore(seed=5).trainable(dev)
    new_xyz, sa, fp = sa_fp(pkg, store, xyz, feats, True)

    # bitwise equal to the composition by hand, on a second store with the same initial values
    hand = tu.ParamStore(seed=5).trainable(dev)
    f2 = feats0.clone().requires_grad_(True)
    nx, new_points, idx, gxyz = pu.sample_and_group(NPOINT, RADIUS, NS, xyz, f2)
    sa_layers = tu.torch_layers(hand, ["sa1/conv0", "sa1/conv1"], C + 3, SA_MLP)
    sa2 = pu._pool_torch(tu.mlp_train(new_points, sa_layers, None), "max", gxyz)
    fp_in = pu.fp_interpolate(xyz, nx, f2, sa2)
    fp_layers = tu.torch_layers(hand, ["fp1/conv_0", "fp1/conv_1"], C + SA_MLP[-1], FP_MLP)
    fp2 = tu.mlp_train(fp_in, fp_layers, None)
    assert torch.equal(new_xyz, nx) and torch.equal(sa, sa2) and torch.equal(fp, fp2)
    assert sorted(store) == sorted(hand)

    # moving averages: decay * old + (1 - decay) * batch, decay 0.9, old = (0, 1)
    def expect(x, scope, dt):
        w = hand[f"{scope}/weights"].detach().cpu().to(dt).reshape(x.shape[-1], -1)
        y = x.detach().cpu().to(dt).reshape(-1, x.shape[-1]) @ w + hand[f"{scope}/biases"].detach().cpu().to(dt)
        return (0.9 * 0 + 0.1 * y.mean(0)), (0.9 * 1 + 0.1 * y.var(0, unbiased=False))
    for x, scope in ((new_points, "sa1/conv0"), (fp_in, "fp1/conv_0")):
        m64, v64 = expect(x, scope, torch.float64)
        m32, v32 = expect(x, scope, torch.float32)
        assert store[f"{scope}/bn/moving_mean"].device.type == "cuda"
        assert not store[f"{scope}/bn/moving_mean"].requires_grad
        assert_close(store[f"{scope}/bn/moving_mean"], m64, m32, scope + " moving_mean")
        assert_close(store[f"{scope}/bn/moving_variance"], v64, v32, scope + " moving_variance")

    # inference before the step (fills the packed-layer cache)
    with torch.no_grad():
        before = pu.pointnet_sa_module(xyz, feats0, NPOINT, RADIUS, NS, SA_MLP, None, False, False,
                                       None, "sa1", params=store)[1]

    # gradients: every variable and the input features. Under batch norm the bias gradient is
    # identically zero (the batch mean absorbs the bias): exactly 0 there, non-zero elsewhere.
    g = torch.Generator().manual_seed(1)
    (fp * torch.rand(fp.shape, generator=g).to(dev)).sum().backward()
    names = [k for k, v in store.items() if v.requires_grad]
    assert len(names) == 4 * 4 and len(list(store.parameters())) == len(names)
    for k in names:
        gr = store[k].grad
        assert gr is not None and torch.isfinite(gr).all(), k
        if k.endswith("/biases"):
            assert (gr == 0).all(), k
        else:
            assert gr.abs().max() > 0, k
    assert torch.isfinite(feats.grad).all() and feats.grad.abs().max() > 0

    # an optimiser step, then inference: the updated weights are used
    opt = torch.optim.Adam(store.parameters(), lr=1e-2)
    opt.step()
    with torch.no_grad():
        after = pu.pointnet_sa_module(xyz, feats0, NPOINT, RADIUS, NS, SA_MLP, None, False, False,
                                      None, "sa1", params=store)[1]
        layers = tu.torch_layers(store, ["sa1/conv0", "sa1/conv1"], C + 3, SA_MLP)
        ref = pu._pool_torch(tu.mlp_torch(new_points.detach(), layers, False), "max", gxyz)
    assert not torch.equal(after, before)
    torch.testing.assert_close(after, ref, rtol=1e-4, atol=1e-5)
    # checkpoint export: CPU arrays under the TF names, loadable into a plain store
    sd = store.state_dict()
    assert np.array_equal(sd["sa1/conv0/weights"], store["sa1/conv0/weights"].detach().cpu().numpy())
    plain = tu.ParamStore(sd)
    with torch.no_grad():
        again = pu.pointnet_sa_module(xyz, feats0, NPOINT, RADIUS, NS, SA_MLP, None, False, False,
                                      None, "sa1", params=plain)[1]
    torch.testing.assert_close(again, after, rtol=1e-5, atol=1e-6)


def test_plain_store_keeps_the_torch_training_path(env, cloud, monkeypatch):
    pkg, ops, torch, dev = env
    tu, pu = pkg.tf_util, pkg.pointnet_util
    xyz, feats = cloud

    def boom(*a, **k):
        raise AssertionError("mlp_train called on a store that is not trainable")
    monkeypatch.setattr(tu, "mlp_train", boom)
    store = tu.ParamStore(seed=5)
    new_xyz, sa, fp = sa_fp(pkg, store, xyz, feats, True)
    assert not store.is_trainable and all(v.device.type == "cpu" and not v.requires_grad
                                          for v in store.values())
    hand = tu.ParamStore(seed=5)
    C = int(feats.shape[2])
    nx, new_points, idx, gxyz = pu.sample_and_group(NPOINT, RADIUS, NS, xyz, feats)
    layers = tu.torch_layers(hand, ["sa1/conv0", "sa1/conv1"], C + 3, SA_MLP)
    sa2 = pu._pool_torch(tu.mlp_torch(new_points, layers, True, None), "max", gxyz)
    torch.testing.assert_close(sa, sa2, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(store["sa1/conv0/bn/moving_mean"], hand["sa1/conv0/bn/moving_mean"],
                               rtol=1e-5, atol=1e-6)
    with pytest.raises(NotImplementedError, match="trainable"):
        tu.conv2d(new_points, 32, [1, 1], "c", bn=True, is_training=True, params=store)


def test_conv2d_and_conv1d_train(env):
    """tf_util.conv2d / conv1d with is_training=True on a trainable store run mlp_train."""
    pkg, ops, torch, dev = env
    tu = pkg.tf_util
    store = tu.ParamStore(seed=2).trainable(dev)
    x = torch.from_numpy(pkg.synth.features_uniform(3, (2, 50, 4, 9))).to(dev).requires_grad_(True)
    out = tu.conv2d(x, 32, [1, 1], "c2", bn=True, is_training=True, bn_decay=0.5, params=store)
    layers = tu.torch_layers(store, ["c2"], 9, [32], bn=True)
    mm = store["c2/bn/moving_mean"].clone()
    assert torch.equal(out, tu.mlp_train(x, layers, 0.5))
    assert not torch.equal(mm, store["c2/bn/moving_mean"])
    head = tu.conv1d(x[:, :, 0], 4, 1, "fc", activation_fn=None, is_training=True, params=store)
    assert head.shape == (2, 50, 4) and "fc/bn/gamma" not in store
    head.sum().backward()
    assert store["fc/weights"].grad.abs().max() > 0 and store["fc/biases"].grad.abs().max() > 0
    assert x.grad is not None and x.grad.abs().max() > 0


def test_learning_smoke(env, cloud):
    """One SA module, one FP module and a 1x1 head with 4 classes, 30 Adam steps on one fixed
    batch: the cross-entropy after the last step is lower than at step 0."""
    pkg, ops, torch, dev = env
    tu = pkg.tf_util
    xyz, feats = cloud
    med = feats.median(dim=1, keepdim=True).values  # labels: a function of the point's features
    labels = ((feats[..., 0] > med[..., 0]).long() * 2 + (feats[..., 1] > med[..., 1]).long()).reshape(-1)
    store = tu.ParamStore(seed=9).trainable(dev)

    def loss_of():
        _, _, fp = sa_fp(pkg, store, xyz, feats, True)
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
    assert np.isfinite(losses).all() and last < losses[0]


def test_mlp2_and_msg_train_on_a_trainable_store(env, cloud):
    """The mlp2 branch of pointnet_sa_module and pointnet_sa_module_msg run mlp_train on a
    trainable store: bitwise equal to the composition by hand, gradients for their variables."""
    pkg, ops, torch, dev = env
    tu, pu = pkg.tf_util, pkg.pointnet_util
    xyz, feats = cloud
    C = int(feats.shape[2])
    store, hand = tu.ParamStore(seed=4).trainable(dev), tu.ParamStore(seed=4).trainable(dev)

    _, got, _ = pu.pointnet_sa_module(xyz, feats, NPOINT, RADIUS, NS, [32], [48, 24], False, True,
                                      0.8, "sa", params=store)
    _, new_points, _, gxyz = pu.sample_and_group(NPOINT, RADIUS, NS, xyz, feats)
    x = tu.mlp_train(new_points, tu.torch_layers(hand, ["sa/conv0"], C + 3, [32]), 0.8)
    x = pu._pool_torch(x, "max", gxyz)
    want = tu.mlp_train(x, tu.torch_layers(hand, ["sa/conv_post_0", "sa/conv_post_1"], 32,
                                           [48, 24]), 0.8)
    assert got.shape == (B, NPOINT, 24) and torch.equal(got, want)
    assert torch.equal(store["sa/conv_post_1/bn/moving_mean"], hand["sa/conv_post_1/bn/moving_mean"])

    new_xyz, got = pu.pointnet_sa_module_msg(xyz, feats, NPOINT, [RADIUS], [NS], [[32, 40]], True,
                                             None, "msg", params=store)
    nx, (gp,) = pu.sample_and_group_msg(NPOINT, [RADIUS], [NS], xyz, feats)
    layers = tu.torch_layers(hand, ["msg/conv0_0", "msg/conv0_1"], C + 3, [32, 40])
    want = tu.mlp_train(gp, layers, None).max(dim=2).values
    assert torch.equal(new_xyz, nx) and got.shape == (B, NPOINT, 40) and torch.equal(got, want)
    assert sorted(store) == sorted(hand)

    got.sum().backward()
    for k in ("msg/conv0_0/weights", "msg/conv0_1/weights", "msg/conv0_1/bn/gamma",
              "msg/conv0_1/bn/beta"):
        assert torch.isfinite(store[k].grad).all() and store[k].grad.abs().max() > 0, k


def test_empty_input_keeps_the_moving_averages(env):
    pkg, ops, torch, dev = env
    tu = pkg.tf_util
    store = tu.ParamStore(seed=1).trainable(dev)
    x = torch.empty((0, 9), device=dev)
    out, y, mean, var = ops.mlp_layer_train(x, torch.zeros(9, 32, device=dev), None,
                                            torch.ones(32, device=dev), torch.zeros(32, device=dev),
                                            EPS, True)
    assert out.shape == (0, 32) and (mean == 0).all() and (var == 0).all()
    out = tu.conv2d(x, 32, [1, 1], "e", bn=True, is_training=True, params=store)
    assert out.shape == (0, 32)
    assert (store["e/bn/moving_mean"] == 0).all() and (store["e/bn/moving_variance"] == 1).all()
