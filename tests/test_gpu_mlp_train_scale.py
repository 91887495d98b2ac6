"""GPU: the rows kernel (csrc/mlp.hip, source kSrcRows) and the training-mode shared-MLP layer
(csrc/mlp_train.hip) at the row counts real training batches reach, and the gradients of one
SA + one FP module against float64.

tests/test_gpu_mlp.py and tests/test_gpu_mlp_train.py stop at 4,099 rows, where the rows kernel
always launches with R = 1 row tile and tpw = 1 tile per workgroup, every lane of the batch-norm
stage-2 reductions sees at most one block, and every part of the weight gradient holds one
slab. The first real training batch (SA1 at B = 16: 524,288 rows) runs none of that. Here:

  1. pn2_shared_mlp at R = 2, R = 4 and tpw >= 2 with ragged tails; pn2_shared_mlp_plan (the
     launch path's own selection code) proves which launch each shape gets.
  2. mlp_layer_train / mlp_layer_train_grad with more than 8 stats blocks (nblk > 8), and the
     weight gradient with more slabs than parts through both caps (PN2_WGRAD_MAX_PARTS and
     PN2_WGRAD_MAX_WS_BYTES).
  3. group -> training MLP -> max pool -> interpolate -> training MLP, op by op, every
     gradient against the same graph in plain torch float64 on the CPU.

References and tolerance are those of tests/test_gpu_mlp_train.py (its helpers are imported):

    max |gpu - f64|  <=  max(4 * max |fp32 - f64|,  1e-6 * (1 + max |f64|))

with f64 and fp32 the same plain CPU formula in the two dtypes.
"""
import ctypes
import gc
import importlib

import numpy as np
import pytest

from conftest import PKG_NAME
from mlp_ref import fused, make_layers, mlp_f32
from mlp_train_ref import (B, EPS, FP_MLP, N, NPOINT, NS, RADIUS, SA_MLP, SLAB, bn_act_bwd, ids,
                           make_params, ref_grads, ref_layer, run_case)
from support import assert_close, gpu_marks

pytestmark = gpu_marks

WGRAD_MAX_PARTS = 512   # PN2_WGRAD_MAX_PARTS (include/pn2hip.h)
WGRAD_TILE_BYTES = 4096  # one 32 x 32 fp32 partial tile


@pytest.fixture(scope="module")
def env():
    import torch

    from oracle import oracle as O
    O.set_threads(16)
    pkg = importlib.import_module(PKG_NAME)
    import pn2hip
    return pkg, pn2hip.ops, torch, torch.device("cuda:0"), O


def mlp_plan(rows, cin, widths):
    """(R, tpw) of the pn2_shared_mlp launch for these shapes on the current device
    (pn2_shared_mlp_plan: host only; the packed pointers are checked for alignment, never read)."""
    L = importlib.import_module(PKG_NAME + "._lib")
    tab, c = (L.MlpLayer * len(widths))(), cin
    for i, w in enumerate(widths):
        tab[i] = L.MlpLayer(1 << 20, c, w, L.PN2_MLP_RELU)
        c = w
    R, tpw = ctypes.c_int(0), ctypes.c_int(0)
    L.check(L.lib().pn2_shared_mlp_plan(rows, cin, len(widths), tab, ctypes.addressof(R),
                                        ctypes.addressof(tpw)), "shared_mlp_plan")
    return R.value, tpw.value


def wgrad_parts(rows, cin, cout):
    """(nslabs, nparts) of pn2_mlp_wgrad, from its workspace size."""
    L = importlib.import_module(PKG_NAME + "._lib")
    ws = int(L.lib().pn2_mlp_wgrad_workspace_size(rows, cin, cout))
    ntiles = -(-cin // 32) * -(-cout // 32)
    assert ws % (ntiles * WGRAD_TILE_BYTES) == 0
    return -(-rows // SLAB), ws // (ntiles * WGRAD_TILE_BYTES)


# ------------------------------------------------ 1. the rows kernel at R = 2, 4, tpw >= 2 --

# (rows, cin, widths): a workgroup covers R tiles of 32 rows, so every case ends in a partly
# filled workgroup. The plan each row obtained on the MI355X (256 CUs) is in its comment.
ROWS_CASES = [
    (16384 + 33, 9, [32]),       # R = 2, tpw = 1: the last workgroup has 1 full tile + 1 row
    (32768 + 97, 9, [32, 64]),   # R = 4, tpw = 1: the last workgroup has 3 full tiles + 1 row
    (32768 + 1, 67, [96]),       # R = 4, tpw = 1: cin no multiple of 4 or 8, 3 output tiles
    # R = 4, tpw = 2: 4099 workgroup tiles of 128 rows, so the last workgroup runs one tile of
    # its two, and that tile has 5 rows. (tpw = 2 needs >= 4096 such tiles on 256 CUs with two
    # workgroups per CU; 524288 + 128 * 3 + 5 rows give 4100 tiles, an even count that leaves
    # the last workgroup full, so this row has one tile fewer.)
    (524288 + 128 * 2 + 5, 3, [32]),
]


def rows_id(case):
    return f"{case[0]}x{case[1]}-" + "-".join(str(w) for w in case[2])


@pytest.mark.parametrize("case", ROWS_CASES, ids=rows_id)
def test_rows_kernel_multi_tile_vs_f64(env, case):
    pkg, ops, torch, dev, O = env
    rows, cin, widths = case
    R, tpw = mlp_plan(rows, cin, widths)
    nblocks = -(-rows // (32 * R))
    print(f"plan {rows_id(case)}: R {R} tpw {tpw}, {nblocks} tiles of {32 * R} rows, "
          f"last tile {rows - (nblocks - 1) * 32 * R} rows, last workgroup "
          f"{nblocks - (-(-nblocks // tpw) - 1) * tpw} of {tpw} tiles")
    rng = np.random.default_rng(rows * 31 + cin)
    layers = make_layers(rng, cin, widths)
    x = rng.uniform(-1, 1, (rows, cin)).astype(np.float32)
    got = fused(pkg, layers)(torch.from_numpy(x).to(dev)).cpu().numpy()
    assert_close(got, O.mlp_f64(x, layers), mlp_f32(x, layers), "shared_mlp")


def test_rows_cases_reach_every_plan():
    """The table above covers R = 2, R = 4 and tpw >= 2, each with a ragged last workgroup."""
    plans = {case[0]: mlp_plan(*case) for case in ROWS_CASES}
    print("plans (rows: R, tpw):", plans)
    assert {R for R, _ in plans.values()} >= {2, 4}
    assert max(tpw for _, tpw in plans.values()) >= 2
    for rows, (R, tpw) in plans.items():
        assert rows % (32 * R) != 0                      # a partly filled last tile
        if tpw > 1:
            assert -(-rows // (32 * R)) % tpw != 0       # a last workgroup short of tpw tiles


# ------------------------------------------------ 2. the training layer at scale ------------

BIG = (514 * SLAB + 7, 35, 40, True, True)
# (rows, cin, cout, batch norm, relu)
SCALE_CASES = [
    (9 * SLAB + 5, 16, 40, True, True),      # nblk 10: lanes 0, 1 take two blocks; 5-row tail
    (16 * SLAB + 1, 40, 33, True, True),     # nblk 17: a 1-row block on lane 0's third pass
    (32768 + 97, 35, 40, True, False),       # nblk 33
    (32768 + 97, 35, 40, False, True),       # bn_bwd_partial<false> over 33 blocks
    # 515 stats blocks (64 to 65 per stage-2 lane); 515 wgrad slabs over 512 parts: parts 0 to
    # 2 take two slabs, and the second slab of part 2 has 7 rows
    BIG,
]
# R of the forward GEMM (cin -> cout) and of the grad_x GEMM (cout -> cin). The tpw obtained
# on the MI355X is 1, except for BIG: 2 for both GEMMs (4113 tiles of 128 rows, so the last
# workgroup runs one tile of its two, with 7 rows)
EXPECT_R = {SCALE_CASES[0]: (1, 1), SCALE_CASES[1]: (2, 2), SCALE_CASES[2]: (4, 4),
            SCALE_CASES[3]: (4, 4), BIG: (4, 4)}


def check_forward(torch, case, outs, fwd):
    out, y, mean, var = outs
    r64, r32 = fwd[torch.float64], fwd[torch.float32]
    assert_close(y, r64[1], r32[1], "y")
    assert_close(out, r64[0], r32[0], "out")
    if case[3]:
        assert_close(mean, r64[2], r32[2], "mean")
        assert_close(var, r64[3], r32[3], "var")
        assert (var >= 0).all()
    else:
        assert mean.numel() == 0 and var.numel() == 0


def check_backward(torch, case, grads, bwd):
    gx, gw, gb, gg, gbeta = grads
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


@pytest.mark.parametrize("case", SCALE_CASES, ids=ids)
def test_layer_at_scale(env, case):
    pkg, ops, torch, dev, O = env
    rows, cin, cout, bn, relu = case
    assert -(-rows // SLAB) > 8                       # nblk: some stage-2 lane loops twice
    plans = mlp_plan(rows, cin, [cout]), mlp_plan(rows, cout, [cin])
    nslabs, nparts = wgrad_parts(rows, cin, cout)
    print(f"{ids(case)}: forward (R, tpw) {plans[0]}, grad_x (R, tpw) {plans[1]}, "
          f"wgrad {nslabs} slabs in {nparts} parts")
    assert (plans[0][0], plans[1][0]) == EXPECT_R[case]
    if case == BIG:
        assert nparts == WGRAD_MAX_PARTS and nslabs > nparts
        assert min(plans[0][1], plans[1][1]) >= 2
    # not cached (the module-level cache of run_case would keep ~0.5 GB alive)
    p, d, outs, grads, fwd, bwd = run_case.__wrapped__(case)
    try:
        check_forward(torch, case, outs, fwd)
        check_backward(torch, case, grads, bwd)
        if case == BIG:  # bitwise reproducible: a second run equals the first
            f = ops.mlp_layer_train(d["x"], d["w"], d["b"], d["gamma"], d["beta"], EPS, relu)
            g = ops.mlp_layer_train_grad(d["go"], d["x"], d["w"], f[1], f[2], f[3], d["gamma"],
                                         d["beta"], EPS, relu, True)
            for i, (u, v) in enumerate(zip(list(outs) + list(grads), list(f) + list(g))):
                assert torch.equal(u, v), f"output {i} differs between two runs"
    finally:
        del p, d, outs, grads, fwd, bwd
        gc.collect()
        torch.cuda.empty_cache()


def test_wgrad_workspace_capped(env):
    """pn2_mlp_wgrad with the workspace cap binding: 1030 -> 1024 channels allow 15 parts, so
    17 slabs leave parts 0 and 1 with two slabs each (the second slab of part 1 has 1 row)."""
    pkg, ops, torch, dev, O = env
    L = importlib.import_module(PKG_NAME + "._lib")
    rows, cin, cout = 16 * SLAB + 1, 1030, 1024
    nslabs, nparts = wgrad_parts(rows, cin, cout)
    assert (nslabs, nparts) == (17, 15)
    g = torch.Generator().manual_seed(1030)
    x = torch.rand(rows, cin, generator=g) * 2 - 1
    gy = torch.rand(rows, cout, generator=g) * 2 - 1
    xd, gyd = x.to(dev), gy.to(dev)
    ws_bytes = int(L.lib().pn2_mlp_wgrad_workspace_size(rows, cin, cout))
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=dev)
    gw = torch.full((cin, cout), float("nan"), device=dev)
    L.check(L.lib().pn2_mlp_wgrad(L.ptr(xd), L.ptr(gyd), rows, cin, cout, L.ptr(gw), L.ptr(ws),
                                  ws_bytes, L.stream_of(xd)), "mlp_wgrad")
    assert_close(gw, x.double().T @ gy.double(), x.T @ gy, "grad_w")


@pytest.mark.parametrize("rows", [9 * SLAB + 5, 514 * SLAB + 7])
def test_variance_survives_cancellation_at_scale(env, rows):
    """test_variance_survives_cancellation (channel means of y at +-50, spread near 1) with
    two blocks on some stage-2 lanes, and with 64 to 65 blocks on every lane."""
    pkg, ops, torch, dev, O = env
    cin, cout = 32, 32
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


def test_degenerate_channels(env):
    """A zero weight column (y constant there: a variance of ~0 against eps = 1e-3) and a
    channel with gamma = 0 (its grad_y is exactly 0, so it adds exactly 0 to grad_w)."""
    pkg, ops, torch, dev, O = env
    rows, cin, cout = 300, 16, 64
    const, dead = 5, 9
    p = make_params(torch, rows, cin, cout, True, seed=rows * 31 + cin)
    p["w"][:, const] = 0
    p["gamma"][dead] = 0
    d = {k: v.to(dev) for k, v in p.items()}
    out, y, mean, var = ops.mlp_layer_train(d["x"], d["w"], d["b"], d["gamma"], d["beta"], EPS, True)
    grads = ops.mlp_layer_train_grad(d["go"], d["x"], d["w"], y, mean, var, d["gamma"], d["beta"],
                                     EPS, True, True)
    mask = (out > 0).cpu()
    fwd = {dt: ref_layer(torch, p, dt, True)[0] for dt in (torch.float64, torch.float32)}
    bwd = {dt: ref_grads(torch, p, dt, True, mask) for dt in (torch.float64, torch.float32)}
    assert fwd[torch.float64][3][const] < 1e-12 * EPS
    case = (rows, cin, cout, True, True)
    check_forward(torch, case, (out, y, mean, var), fwd)
    check_backward(torch, case, grads, bwd)
    gy, gg, _ = bn_act_bwd(pkg, torch, d["go"], y, mean, var, d["gamma"], d["beta"], True)
    assert (gy[:, dead] == 0).all()
    assert (grads[1][:, dead] == 0).all()
    assert torch.isfinite(grads[3][dead]) and torch.equal(gg, grads[3])


# ------------------------------------------------ 3. module gradients against float64 -------

DECAY = 0.8
SCOPES = ["sa1/conv0", "sa1/conv1", "fp1/conv_0", "fp1/conv_1"]
VARS = ("weights", "biases", "bn/gamma", "bn/beta")


def test_module_gradients_vs_f64(env):
    """One SA module and one FP module on a trainable store, composed by hand op by op
    (test_modules_train_on_a_trainable_store pins the modules as bitwise equal to this
    composition), against the same graph in plain torch on the CPU in float64 and float32. The
    reference takes the discrete choices from the GPU forward (they are validated bit-exactly
    elsewhere, and a flip is not an error): the sampled centres, the ball-query and three_nn
    indices and the IDW weights, each ReLU as a product with the mask out_gpu > 0, and the max
    pool as a gather at the GPU's argmax."""
    pkg, ops, torch, dev, O = env
    tu, pu, ti = pkg.tf_util, pkg.pointnet_util, pkg.tf_interpolate
    xyz_np, feats_np = pkg.synth.batch([0, 1], N, "scannet", with_features=True)
    xyz, feats0 = torch.from_numpy(xyz_np).to(dev), torch.from_numpy(feats_np).to(dev)
    C = int(feats0.shape[2])
    widths = [(C + 3, SA_MLP[0]), (SA_MLP[0], SA_MLP[1]),
              (C + SA_MLP[1], FP_MLP[0]), (FP_MLP[0], FP_MLP[1])]

    # ---- the graph under test
    store = tu.ParamStore(seed=5).trainable(dev)
    for scope, (ci, co) in zip(SCOPES, widths):
        store.conv(scope, ci, co)
    init = {k: v.detach().cpu().clone() for k, v in store.items()}
    feats = feats0.clone().requires_grad_(True)

    def layer(h, scope):
        ci, co = widths[SCOPES.index(scope)]
        v = store.conv(scope, ci, co)
        out, y, mean, var = ops.mlp_layer_train(h, v["weights"], v["biases"], v["gamma"],
                                                v["beta"], EPS, True)
        return out, (out > 0).cpu()

    new_xyz, new_points, idx, _ = pu.sample_and_group(NPOINT, RADIUS, NS, xyz, feats)
    assert new_points.shape == (B, NPOINT, NS, C + 3)
    h, masks = new_points, []
    for scope in SCOPES[:2]:
        h, m = layer(h, scope)
        masks.append(m)
    pooled = h.max(dim=2)
    sa, arg = pooled.values, pooled.indices.cpu()
    fp_in, (dist, nn_idx) = pu.fp_interpolate(xyz, new_xyz, feats, sa, return_nn=True)
    weight = ti.idw_weights(dist)
    h = fp_in
    for scope in SCOPES[2:]:
        h, m = layer(h, scope)
        masks.append(m)
    fp = h
    go = torch.rand(fp.shape, generator=torch.Generator().manual_seed(1)) * 2 - 1
    (fp * go.to(dev)).sum().backward()

    # ---- the reference
    bidx = torch.arange(B).reshape(B, 1, 1)
    idx_c, nn_c = idx.cpu().long(), nn_idx.cpu().long()

    def ref(dt):
        leaves = {k: v.to(dt).clone().requires_grad_(True) for k, v in init.items()
                  if k.endswith(VARS)}
        f = feats0.cpu().to(dt).requires_grad_(True)
        x, nx = xyz.cpu().to(dt), new_xyz.detach().cpu().to(dt)
        stats = []

        def rlayer(a, scope, mask):
            ci, co = widths[SCOPES.index(scope)]
            y = a @ leaves[f"{scope}/weights"].reshape(ci, co) + leaves[f"{scope}/biases"]
            y2 = y.reshape(-1, co)
            mean, var = y2.mean(0), y2.var(0, unbiased=False)
            stats.append((mean.detach(), var.detach()))
            z = (y - mean) * (leaves[f"{scope}/bn/gamma"] / torch.sqrt(var + EPS))
            return (z + leaves[f"{scope}/bn/beta"]) * mask.to(dt)

        a = torch.cat([x[bidx, idx_c] - nx.unsqueeze(2), f[bidx, idx_c]], dim=-1)
        for scope, m in zip(SCOPES[:2], masks[:2]):
            a = rlayer(a, scope, m)
        s = torch.gather(a, 2, arg.unsqueeze(2)).squeeze(2)
        interp = (s[bidx, nn_c] * weight.cpu().to(dt).unsqueeze(-1)).sum(dim=2)
        a = torch.cat([interp, f], dim=-1)
        for scope, m in zip(SCOPES[2:], masks[2:]):
            a = rlayer(a, scope, m)
        (a * go.to(dt)).sum().backward()
        return a.detach(), s.detach(), f.grad, {k: v.grad for k, v in leaves.items()}, stats

    fp64, sa64, gf64, gv64, st64 = ref(torch.float64)
    fp32, sa32, gf32, gv32, st32 = ref(torch.float32)
    assert_close(sa, sa64, sa32, "sa output")
    assert_close(fp, fp64, fp32, "fp output")
    assert_close(feats.grad, gf64, gf32, "grad of the input features")
    assert sorted(gv64) == sorted(f"{s}/{v}" for s in SCOPES for v in VARS)
    for k in sorted(gv64):
        assert store[k].grad is not None, k
        assert_close(store[k].grad, gv64[k], gv32[k], "grad " + k)
        if k.endswith("/biases"):
            assert (store[k].grad == 0).all(), k  # the batch mean absorbs the bias

    # ---- moving averages of the modules: decay * old + (1 - decay) * batch from (0, 1), after
    # one call and after a second call on the same store (same inputs and variables, so the
    # same batch statistics: two steps pin the in-place update rule, not just its first step)
    mod = tu.ParamStore(seed=5).trainable(dev)
    f2 = feats0.clone().requires_grad_(True)
    mm = {dt: [(torch.zeros_like(m), torch.ones_like(v)) for m, v in st]
          for dt, st in ((torch.float64, st64), (torch.float32, st32))}
    for call in (1, 2):
        nx, sa_m, _ = pu.pointnet_sa_module(xyz, f2, NPOINT, RADIUS, NS, SA_MLP, None, False, True,
                                            DECAY, "sa1", params=mod)
        fp_m = pu.pointnet_fp_module(xyz, nx, f2, sa_m, FP_MLP, True, DECAY, "fp1", params=mod)
        assert torch.equal(sa_m, sa) and torch.equal(fp_m, fp)
        for dt, st in ((torch.float64, st64), (torch.float32, st32)):
            mm[dt] = [(DECAY * m0 + (1 - DECAY) * m, DECAY * v0 + (1 - DECAY) * v)
                      for (m0, v0), (m, v) in zip(mm[dt], st)]
        for i, scope in enumerate(SCOPES):
            assert_close(mod[f"{scope}/bn/moving_mean"], mm[torch.float64][i][0],
                         mm[torch.float32][i][0], f"call {call} {scope} moving_mean")
            assert_close(mod[f"{scope}/bn/moving_variance"], mm[torch.float64][i][1],
                         mm[torch.float32][i][1], f"call {call} {scope} moving_variance")
