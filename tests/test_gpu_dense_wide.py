"""GPU: the K-streamed layer kernel (csrc/mlp_wide.hip) through pn2_dense_wide,
torch.ops.pn2.dense_wide, the training ops that fall to it (mlp_layer_train[_pool] and their
gradients at widths the fused kernel refuses) and the attention networks' dispatch
(attention_layer.run_layers, attention_models.fp_module).

Values are held to the project's bar (tests/support.py) against numpy float64,

    max |gpu - f64|  <=  max(4 * max |fp32 - f64|,  1e-6 * (1 + max |f64|))

with fp32 the same formulas in numpy float32; on shapes that pn2_shared_mlp also takes the
result is compared with its bits: both kernels sum each output as one chain over the chunks of 8
input channels on the fp32 matrix cores, the fused kernel with either operand order (its staged
and its register epilogue), this kernel with the weights as the A operand.
"""
import importlib

import pytest

import attn_net_ref as R
import mlp_train_ref as TR
from conftest import PKG_NAME
from dense_wide_ref import (BITS_CASES, call_c, case_id, draw, packed_layer, plan, ref_f32,
                            ref_f64, run_value_case, value_cases)
from mlp_ref import fused
from support import assert_close, gpu_marks, same_bits

pytestmark = gpu_marks


@pytest.fixture(scope="module")
def env():
    import torch
    pkg = importlib.import_module(PKG_NAME)
    import pn2hip
    return pkg, pn2hip.ops, torch, torch.device("cuda:0")


# ------------------------------------------------------------------ (1) values against float64
@pytest.mark.parametrize("case", value_cases(), ids=case_id)
def test_values_vs_f64(env, case):
    cin, _, _, got, r64, r32 = run_value_case(case)
    assert_close(got, r64, r32, f"dense_wide cin={cin}")


# ------------------------------------------------------------- (2) bits against pn2_shared_mlp
@pytest.mark.parametrize("rows,cin,cout", BITS_CASES)
def test_bits_of_shared_mlp(env, rows, cin, cout):
    pkg, ops, torch, dev = env
    x, layers = draw(rows, cin, cout)
    xd = torch.from_numpy(x).to(dev)
    want = fused(pkg, layers)(xd)
    got = call_c(torch, packed_layer(pkg, layers[0]), xd)
    same_bits(got, want, f"dense_wide vs shared_mlp {rows}x{cin}->{cout}")


# -------------------------------------------- (3) reproducibility and entry-point agreement
@pytest.mark.parametrize("case", [c for c in value_cases() if c[1] in (2051, "ks+1", 1280)],
                         ids=case_id)
def test_two_runs_and_the_torch_op_agree(env, case):
    pkg, ops, torch, dev = env
    cin, xd, P, got, _, _ = run_value_case(case)
    assert not torch.isnan(got).any()            # the NaN-filled out came back fully written
    same_bits(call_c(torch, P, xd), got, "second run")
    via_op = ops.dense_wide(xd, P.buf, P.cin, P.cout, P.relu)
    assert via_op.shape == got.shape
    same_bits(via_op, got, "torch op vs C entry point")
    # leading axes are rows
    if xd.shape[0] % 2 == 0:
        same_bits(ops.dense_wide(xd.reshape(2, -1, cin), P.buf, P.cin, P.cout, P.relu)
                  .reshape(got.shape), got, "(2, rows / 2, cin) input")


def test_no_rows(env):
    pkg, ops, torch, dev = env
    _, layers = draw(4, 1280, 33)
    P = packed_layer(pkg, layers[0])
    assert ops.dense_wide(torch.empty(0, 1280, device=dev), P.buf, 1280, 33, True).shape == (0, 33)


# ------------------------------------------------------------------------------ (4) layout
@pytest.mark.parametrize("cout", [256, 33])
def test_offset_buffers_give_the_same_bits(env, cout):
    """x 4 bytes past a 16-byte boundary (per-float loads), out 4 bytes past one (per-float
    stores), cout % 4 != 0 (per-float stores whatever the pointer): the aligned call's bits."""
    pkg, ops, torch, dev = env
    rows, cin = 70, 1280
    x, layers = draw(rows, cin, cout)
    P = packed_layer(pkg, layers[0])
    xd = torch.from_numpy(x).to(dev)
    assert xd.data_ptr() % 16 == 0
    base = call_c(torch, P, xd)
    assert base.data_ptr() % 16 == 0
    xbuf = torch.zeros(rows * cin + 1, device=dev)
    xo = xbuf[1:].view(rows, cin)
    xo.copy_(xd)
    assert xo.data_ptr() % 16 == 4
    for xin, off_out in ((xo, False), (xd, True), (xo, True)):
        obuf = torch.full((rows * cout + 1,), float("nan"), device=dev)
        out = obuf[1:].view(rows, cout) if off_out else obuf[:-1].view(rows, cout)
        assert out.data_ptr() % 16 == (4 if off_out else 0)
        call_c(torch, P, xin, out)
        same_bits(out, base, f"x offset={xin is xo}, out offset={off_out}")
        assert torch.isnan(obuf[:1] if off_out else obuf[-1:]).all()   # nothing past the rows


# ----------------------------------------------------------------------- (5) launch limits
@pytest.mark.parametrize("cin,cout,want", [(1280, 33, (8, 32, 2)), (40, 128, (4, 64, 4))])
def test_more_row_blocks_than_one_wave_of_workgroups(env, cin, cout, want):
    """Two workgroups share a CU, so 2 * CUs + 1 row blocks need a second wave of workgroups;
    the last block holds one valid row. Sampled rows against float64, and every row against the
    same layer run in chunks of 1,000 rows (another launch shape: the bits do not depend on it)."""
    pkg, ops, torch, dev = env
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    # the row tiles of a layer over many rows (the shape does not change past 256 blocks)
    row_tiles = plan(1 << 24, cin, cout)[1]
    rows = 32 * row_tiles * 2 * cus + 1
    assert plan(rows, cin, cout)[1:] == want
    _, layers = draw(8, cin, cout)
    P = packed_layer(pkg, layers[0])
    g = torch.Generator(device=dev).manual_seed(3)
    xd = torch.rand(rows, cin, device=dev, generator=g) * 2 - 1
    got = call_c(torch, P, xd)
    assert not torch.isnan(got).any()
    pick = torch.tensor([0, 31, 32, 255, 256, rows // 2, rows - 258, rows - 2, rows - 1], device=dev)
    xs = xd[pick].cpu().numpy()
    assert_close(got[pick], ref_f64(xs, layers), ref_f32(xs, layers), "sampled rows")
    step = 1000
    assert plan(step, cin, cout)[1:] != want
    for r0 in range(0, rows, step * 16):   # every 16th chunk, and the last
        same_bits(call_c(torch, P, xd[r0:r0 + step]), got[r0:r0 + step], f"rows from {r0}")
    r0 = rows - rows % step
    same_bits(call_c(torch, P, xd[r0:]), got[r0:], "the last chunk")


# ----------------------------------------------------------------------------- (6) training
# (rows, cin, cout, batch norm, relu): a wide forward, a wide input gradient (the layer over
# W^T), and both with odd widths
TRAIN_CASES = [(rows, cin, cout, bn, True) for rows, cin, cout in
               ((64, 1280, 32), (64, 32, 1280), (40, 2051, 33)) for bn in (True, False)]


@pytest.mark.parametrize("case", TRAIN_CASES, ids=TR.ids)
def test_training_layer(env, case):
    pkg, ops, torch, dev = env
    p, d, (out, y, mean, var), grads, fwd, bwd = TR.run_case(case)
    r64, r32 = fwd[torch.float64], fwd[torch.float32]
    assert_close(y, r64[1], r32[1], "y")
    assert_close(out, r64[0], r32[0], "out")
    if case[3]:
        assert_close(mean, r64[2], r32[2], "mean")
        assert_close(var, r64[3], r32[3], "var")
    g64, g32 = bwd[torch.float64], bwd[torch.float32]
    names = ("x", "w", "b") + (("gamma", "beta") if case[3] else ())
    for name, g in zip(names, grads):
        assert_close(g, g64[name], g32[name], "grad_" + name)
    # equal bits twice
    again = ops.mlp_layer_train(d["x"], d["w"], d["b"], d["gamma"], d["beta"], TR.EPS, case[4])
    again_g = ops.mlp_layer_train_grad(d["go"], d["x"], d["w"], again[1], again[2], again[3],
                                       d["gamma"], d["beta"], TR.EPS, case[4], True)
    for i, (a, b) in enumerate(zip(list(again) + list(again_g), [out, y, mean, var] + list(grads))):
        same_bits(a, b, f"second run, output {i}")


@pytest.mark.parametrize("case", TRAIN_CASES, ids=TR.ids)
def test_training_layer_with_the_max_pool(env, case):
    pkg, ops, torch, dev = env
    rows, cin, cout, bn, relu = case
    ns = 8
    p = TR.pool_make_params(torch, rows // ns, ns, cin, cout, bn, seed=rows * 31 + cin)
    d = {k: None if v is None else v.to(dev) for k, v in p.items()}

    def run():
        f = ops.mlp_layer_train_pool(d["x"], d["w"], d["b"], d["gamma"], d["beta"], TR.EPS, relu)
        g = ops.mlp_layer_train_pool_grad(d["go"], f[4], d["x"], d["w"], f[1], f[2], f[3],
                                          d["gamma"], d["beta"], TR.EPS, relu, True)
        return list(f), list(g)

    (out, y, mean, var, arg), grads = run()
    torch.cuda.synchronize()
    flat = {k: (v.reshape(rows, -1) if k == "x" else v) for k, v in p.items()}
    r64 = TR.ref_layer(torch, flat, torch.float64, relu)[0]
    r32 = TR.ref_layer(torch, flat, torch.float32, relu)[0]
    pool = lambda z: z.detach().reshape(rows // ns, ns, cout).max(dim=1).values  # noqa: E731
    assert_close(y.reshape(rows, cout), r64[1], r32[1], "y")
    assert_close(out, pool(r64[0]), pool(r32[0]), "pooled out")
    # the ReLU mask and the pool's argument are discrete: the references take the GPU's
    plain = ops.mlp_layer_train(d["x"], d["w"], d["b"], d["gamma"], d["beta"], TR.EPS, relu)[0]
    mask, arg_cpu = (plain > 0).cpu(), arg.cpu()
    g64 = TR.pool_ref_grads(torch, p, torch.float64, relu, mask, arg_cpu)
    g32 = TR.pool_ref_grads(torch, p, torch.float32, relu, mask, arg_cpu)
    names = ("x", "w", "b") + (("gamma", "beta") if bn else ())
    for name, g in zip(names, grads):
        assert_close(g, g64[name], g32[name], "grad_" + name)
    f2, g2 = run()
    for i, (a, b) in enumerate(zip(f2 + g2, [out, y, mean, var, arg] + grads)):
        same_bits(a, b, f"second run, output {i}")


def test_bf16_training_ops_keep_refusing_a_wide_layer(env):
    pkg, ops, torch, dev = env
    x, w = torch.zeros(8, 1280, device=dev), torch.zeros(1280, 32, device=dev)
    with pytest.raises(ValueError):
        ops.mlp_layer_train_bf16(x, w, None, None, None, TR.EPS, True)


# ----------------------------------------------------------------------------- (7) dispatch
DB, DN, DNPOINT, DNS, DOUT, DRADIUS, DCH = 1, 64, 4, 8, 8, 0.6, 1277


@pytest.fixture
def no_torch_layers(env, monkeypatch):
    """attention_layer._layer_torch raises: whatever runs below runs on the project's kernels."""
    pkg = env[0]

    def refuse(*a, **k):
        raise AssertionError("a layer fell back to torch ops (_layer_torch)")

    monkeypatch.setattr(pkg.attention_layer, "_layer_torch", refuse)


def _pooling_layer(pkg, store):
    return pkg.pooling_attention_layer.PoolingAttentionNetLayer(
        None, [8, 8], npoint=DNPOINT, out_dim=DOUT, nsample=DNS, radius=DRADIUS, scope="L",
        params=store)


def _pooling_inputs(pkg, torch):
    from support import clouds
    xyz = torch.from_numpy(clouds(pkg, "uniform", DB, DN, seed=3))
    g = torch.Generator().manual_seed(11)
    points = torch.rand(DB, DN, DCH, generator=g) * 2 - 1
    go = torch.rand(DB, DNPOINT, 16 * DOUT, generator=g) * 2 - 1
    return xyz, points, go


def _pooling_refs(torch, store, xyz, points, new_xyz, idx, training):
    refs = []
    for dt in (torch.float64, torch.float32):
        w = {k: torch.from_numpy(v).to(dt) for k, v in store.state_dict().items()}
        grouped = R.group(xyz.to(dt), points.to(dt), new_xyz.cpu().to(dt), idx.cpu())
        assert grouped.shape[-1] == 1280
        refs.append(R.pooling_attention_net_layer(w, "L", grouped, new_xyz.cpu().to(dt), DOUT, 2,
                                                  training))
    return refs


def test_pooling_layer_runs_without_torch_layers(env, no_torch_layers):
    """A pooling layer over 1,277 point channels + xyz = a 1,280-wide grouped row, which
    the fused kernel refuses. Forward on a plain store, forward + backward on a trainable one,
    with _layer_torch patched to raise; the forward is held to the float64 evaluation, and so is
    the wide_layers="torch" store's (run without the patch below)."""
    pkg, ops, torch, dev = env
    assert not pkg.attention_layer.plan_accepts(1280, (8,))
    xyz, points, go = _pooling_inputs(pkg, torch)
    store = pkg.tf_util.ParamStore(seed=5, wide_layers="hip")
    new_xyz, out, idx = _pooling_layer(pkg, store)([xyz.to(dev), points.to(dev)], is_training=False)
    assert out.shape == (DB, DNPOINT, 16 * DOUT)
    r64, r32 = _pooling_refs(torch, store, xyz, points, new_xyz, idx, False)
    assert_close(out, r64, r32, "pooling layer, wide_layers='hip'")
    again = _pooling_layer(pkg, store)([xyz.to(dev), points.to(dev)], is_training=False)[1]
    same_bits(again, out, "second call (the cached pack)")
    # training: the HIP training layers, gradients for the points and every variable
    tstore = pkg.tf_util.ParamStore(seed=5, wide_layers="hip").trainable(dev)
    p = points.to(dev).requires_grad_(True)
    new_xyz, tout, idx = _pooling_layer(pkg, tstore)([xyz.to(dev), p], is_training=True)
    before = tstore.state_dict()
    t64, t32 = _pooling_refs(torch, pkg.tf_util.ParamStore(before), xyz, points, new_xyz, idx, True)
    assert_close(tout, t64, t32, "pooling layer, training forward")
    (tout * go.to(dev)).sum().backward()
    assert p.grad is not None and torch.isfinite(p.grad).all() and (p.grad != 0).any()
    for k, v in tstore.items():
        if v.requires_grad:
            assert v.grad is not None and torch.isfinite(v.grad).all(), k
    assert (tstore["L/conv0/weights"].grad != 0).any()


def test_pooling_layer_torch_store_agrees(env):
    pkg, ops, torch, dev = env
    xyz, points, _ = _pooling_inputs(pkg, torch)
    outs = {}
    for mode in ("hip", "torch"):
        store = pkg.tf_util.ParamStore(seed=5, wide_layers=mode)
        new_xyz, outs[mode], idx = _pooling_layer(pkg, store)([xyz.to(dev), points.to(dev)],
                                                              is_training=False)
    r64, r32 = _pooling_refs(torch, store, xyz, points, new_xyz, idx, False)
    assert_close(outs["torch"], r64, r32, "pooling layer, wide_layers='torch'")
    assert_close(outs["hip"], r64, r32, "pooling layer, wide_layers='hip'")


def test_torch_store_still_takes_the_torch_layers(env, no_torch_layers):
    pkg, ops, torch, dev = env
    xyz, points, _ = _pooling_inputs(pkg, torch)
    store = pkg.tf_util.ParamStore(seed=5, wide_layers="torch")
    with pytest.raises(AssertionError, match="_layer_torch"):
        _pooling_layer(pkg, store)([xyz.to(dev), points.to(dev)], is_training=False)


FN, FM, FC1, FC2, FMLP = 96, 24, 512, 1024, (16, 8)


def _fp_inputs(pkg, torch):
    from support import clouds
    xyz1 = torch.from_numpy(clouds(pkg, "uniform", 1, FN, seed=5))
    xyz2 = xyz1[:, :FM].contiguous()
    g = torch.Generator().manual_seed(13)
    p1 = torch.rand(1, FN, FC1, generator=g) * 2 - 1
    p2 = torch.rand(1, FM, FC2, generator=g) * 2 - 1
    go = torch.rand(1, FN, FMLP[-1], generator=g) * 2 - 1
    return xyz1, xyz2, p1, p2, go


def _fp_refs(pkg, torch, store, x, training):
    refs = []
    for dt in (torch.float64, torch.float32):
        w = {k: torch.from_numpy(v).to(dt) for k, v in store.state_dict().items()}
        y = x.cpu().to(dt)
        for i in range(len(FMLP)):
            y = R.conv_bn_relu(w, f"fa/conv_{i}", y, training)
        refs.append(y)
    return refs


def test_fp_module_runs_without_torch_layers(env, no_torch_layers):
    """attention_models.fp_module with C1 + C2 = 1,536 (fa_layer1 of the AttentionNet models)."""
    pkg, ops, torch, dev = env
    xyz1, xyz2, p1, p2, go = (t.to(dev) for t in _fp_inputs(pkg, torch))
    fp = pkg.attention_models.fp_module
    x = pkg.pointnet_util.fp_interpolate(xyz1, xyz2, p1, p2)
    assert x.shape[-1] == 1536
    outs = {}
    store = pkg.tf_util.ParamStore(seed=6, wide_layers="hip")
    out = fp(store, xyz1, xyz2, p1, p2, list(FMLP), False, None, "fa")
    r64, r32 = _fp_refs(pkg, torch, store, x, False)
    assert_close(out, r64, r32, "fp_module, wide_layers='hip'")
    outs["hip"] = out
    tstore = pkg.tf_util.ParamStore(seed=6, wide_layers="hip").trainable(dev)
    with torch.no_grad():   # creates the variables
        fp(tstore, xyz1, xyz2, p1, p2, list(FMLP), False, None, "fa")
    before = pkg.tf_util.ParamStore(tstore.state_dict())
    q1, q2 = p1.clone().requires_grad_(True), p2.clone().requires_grad_(True)
    tout = fp(tstore, xyz1, xyz2, q1, q2, list(FMLP), True, None, "fa")
    t64, t32 = _fp_refs(pkg, torch, before, x, True)
    assert_close(tout, t64, t32, "fp_module, training forward")
    (tout * go).sum().backward()
    for name, t in (("points1", q1), ("points2", q2), ("weights", tstore["fa/conv_0/weights"])):
        assert t.grad is not None and torch.isfinite(t.grad).all() and (t.grad != 0).any(), name


def test_fp_module_torch_store_agrees(env):
    pkg, ops, torch, dev = env
    xyz1, xyz2, p1, p2, _ = (t.to(dev) for t in _fp_inputs(pkg, torch))
    x = pkg.pointnet_util.fp_interpolate(xyz1, xyz2, p1, p2)
    for mode in ("torch", "hip"):
        store = pkg.tf_util.ParamStore(seed=6, wide_layers=mode)
        out = pkg.attention_models.fp_module(store, xyz1, xyz2, p1, p2, list(FMLP), False, None,
                                             "fa")
        r64, r32 = _fp_refs(pkg, torch, store, x, False)
        assert_close(out, r64, r32, f"fp_module, wide_layers='{mode}'")
