"""GPU: the training layer's opt-in bf16 matrix-core mode: pn2_mlp_wgrad_bf16 (csrc/mlp_train.hip),
torch.ops.pn2.mlp_layer_train_bf16 / _pool_bf16 and their grad ops, and tf_util's
train_precision through the modules and a short training run.

The contract is written at pn2_mlp_pack_bf16 in include/pn2hip.h; its numpy evaluations E (the
contract, float64 sums), F (no rounding) and E32 (E with float32 sums) and the cases are in
tests/mlp_train_bf16_ref.py, whose own sanity tests/test_mlp_train_bf16_cpu.py checks. The
rounding of given inputs is deterministic, so one GEMM is held to the project's fp32 bar
(support.assert_close) with E as the reference and E32 as the yardstick. Everything the contract
leaves fp32 is compared twice: against the float64 formulas on the device's own y, and bit for
bit against the fp32 layer's entry points called on that y through the C ABI.

  1. layout, exact: integer inputs, the float64 product and pn2_mlp_wgrad bit for bit
  2. rounding mode: ties, near-ties and carries through an identity operand
  3. pn2_mlp_wgrad_bf16 against the contract on random inputs
  4. more slabs than parts, through both caps
  5. the four ops, forward and backward
  6. determinism, and the digests of tests/golden/train_bits_bf16.json
  7. train_precision through the modules and pointnet2_sem_seg
  8. descent: 30 steps at each precision

The JSON names the commit the digests were recorded on top of (the parent of the commit that
added the kernels: the digests belong to that commit's tree). They are regenerated only by
running this file as a script on the GPU:

    python tests/test_gpu_mlp_train_bf16.py --record --commit <hash> [--out FILE]
"""
import hashlib
import importlib
import json
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlp_train_bf16_ref as R  # noqa: E402
from conftest import PKG_NAME  # noqa: E402
from mlp_bf16_ref import bf16_round  # noqa: E402
from mlp_train_ref import EPS, SLAB  # noqa: E402
from support import assert_close, gpu_marks, same_bits  # noqa: E402

pytestmark = gpu_marks

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "train_bits_bf16.json")
T, F = True, False


@pytest.fixture(scope="module")
def env():
    import torch
    pkg = importlib.import_module(PKG_NAME)
    import pn2hip
    return pkg, pn2hip.ops, torch, torch.device("cuda:0")


def to_dev(torch, dev, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ------------------------------------------------------------------ 1. layout, exact --------
@pytest.mark.parametrize("shape", R.WGRAD_SHAPES, ids=R.shape_id)
def test_wgrad_layout_exact(env, shape):
    pkg, ops, torch, dev = env
    x, gy = R.exact_inputs(shape)
    want = R.wgrad(x, gy, "F") + 0.0   # a sum of -0.0 products is +0.0 on accumulators from +0.0
    xd, gyd = to_dev(torch, dev, x), to_dev(torch, dev, gy)
    got = R.c_wgrad(torch, xd, gyd, bf16=True)
    assert np.array_equal(got.cpu().numpy().astype(np.float64), want)
    same_bits(got, want.astype(np.float32), "grad_w vs the float64 product")
    same_bits(got, R.c_wgrad(torch, xd, gyd, bf16=False), "grad_w vs pn2_mlp_wgrad")


# ------------------------------------------------------------------ 2. rounding mode --------
def rounding_probes():
    """1,024 float32 values: exact ties (even and odd kept mantissa), near-ties either side,
    values that carry into the exponent, either sign, several exponents."""
    vals = []
    for e in (-3, 0, 5):
        for keep in (0x00, 0x01, 0x3E, 0x7F):          # the 7 kept mantissa bits
            for low in (0x8000, 0x7FFF, 0x8001, 0x0001, 0xFFFF, 0x0000, 0xC000, 0x4000):
                bits = ((127 + e) << 23) | (keep << 16) | low
                vals += [bits, bits | 0x80000000]
    v = np.array(vals, np.uint32).view(np.float32)
    return np.resize(v, 32 * 32).reshape(32, 32)


def test_wgrad_rounds_to_nearest_even(env):
    pkg, ops, torch, dev = env
    probes = rounding_probes()
    want = bf16_round(probes)
    assert (want != probes).any() and (np.abs(want) > np.abs(probes)).any()
    eye = to_dev(torch, dev, np.eye(32, dtype=np.float32))
    pd = to_dev(torch, dev, probes)
    same_bits(R.c_wgrad(torch, eye, pd, bf16=True), want, "x = I: grad_w = bf16(grad_y)")
    same_bits(R.c_wgrad(torch, pd, eye, bf16=True), np.ascontiguousarray(want.T),
              "grad_y = I: grad_w = bf16(x)^T")


# ------------------------------------------------------------------ 3. against the contract -
@pytest.mark.parametrize("shape", R.WGRAD_SHAPES, ids=R.shape_id)
def test_wgrad_vs_contract(env, shape):
    pkg, ops, torch, dev = env
    x, gy = R.random_inputs(shape)
    got = R.c_wgrad(torch, to_dev(torch, dev, x), to_dev(torch, dev, gy), bf16=True)
    assert_close(got, R.wgrad(x, gy, "E"), R.wgrad(x, gy, "E32"), "grad_w")


# ------------------------------------------------------------------ 4. more slabs than parts
# tests/test_gpu_mlp_train_scale.py's shapes for the fp32 kernel: 515 slabs over
# PN2_WGRAD_MAX_PARTS = 512 parts, and 17 slabs over the 15 parts PN2_WGRAD_MAX_WS_BYTES allows
@pytest.mark.parametrize("shape,parts", [((514 * SLAB + 7, 35, 40), (515, 512)),
                                         ((16 * SLAB + 1, 1030, 1024), (17, 15))],
                         ids=["max_parts", "max_ws_bytes"])
def test_wgrad_more_slabs_than_parts(env, shape, parts):
    pkg, ops, torch, dev = env
    assert R.wgrad_parts(*shape) == parts and parts[0] > parts[1]
    rng = np.random.default_rng(shape[1])
    x = rng.uniform(-1, 1, shape[:2]).astype(np.float32)
    gy = rng.uniform(-1, 1, (shape[0], shape[2])).astype(np.float32)
    got = R.c_wgrad(torch, to_dev(torch, dev, x), to_dev(torch, dev, gy), bf16=True)
    assert_close(got, R.wgrad(x, gy, "E"), R.wgrad(x, gy, "E32"), "grad_w")


# ------------------------------------------------------------------ 5. the ops --------------
def check_forward(torch, x, w, b, gamma, beta, relu, pooled, res, what):
    """One recorded or direct forward call of a _bf16 op: y against the contract; out, mean, var
    (pooled: out, arg) against the float64 formulas on the device's y, and bit for bit against
    the fp32 layer's activation entry points on that y."""
    out, y, mean, var, *arg = res
    bn = gamma is not None
    cpu = lambda t: None if t is None else t.detach().cpu().numpy()  # noqa: E731
    xn, wn, bnp, gn, btn = cpu(x), cpu(w), cpu(b), cpu(gamma), cpu(beta)
    wn = wn.reshape(wn.shape[-2], wn.shape[-1])
    assert_close(y, R.forward(xn, wn, bnp, "E"), R.forward(xn, wn, bnp, "E32"), what + " y")
    ns = int(x.shape[-2]) if pooled else None
    yn = cpu(y).reshape((-1, ns, y.shape[-1]) if pooled else (-1, y.shape[-1]))
    o64, m64, v64, z64 = R.act_ref(yn, gn, btn, relu, np.float64, ns)
    o32, m32, v32, _ = R.act_ref(yn, gn, btn, relu, np.float32, ns)
    assert_close(out.reshape(o64.shape), o64, o32, what + " out")
    if bn:
        assert_close(mean, m64, m32, what + " mean")
        assert_close(var, v64, v32, what + " var")
    else:
        assert mean.numel() == 0 and var.numel() == 0
    yd = y.detach().reshape(yn.shape).contiguous()
    if bn:
        mean_c, var_c = R.c_bn_stats(torch, yd)
        same_bits(mean, mean_c, what + " mean vs pn2_bn_stats")
        same_bits(var, var_c, what + " var vs pn2_bn_stats")
    out_c, arg_c = R.c_act_fwd(torch, yd, mean if bn else None, var if bn else None,
                               gamma.detach() if bn else None, beta.detach() if bn else None,
                               relu, pooled)
    same_bits(out.detach().reshape(out_c.shape), out_c, what + " out vs the fp32 entry point")
    if pooled:
        a = cpu(arg[0]).reshape(o64.shape)
        assert a.dtype == np.int32 and a.min() >= 0 and a.max() < ns
        same_bits(a, arg_c, what + " arg vs pn2_bn_act_pool_fwd")
        at_arg = np.take_along_axis(z64, a[:, None, :].astype(np.int64), 1)[:, 0, :]
        assert_close(at_arg, o64, o32, what + " activation at arg")


def run_layer(ops, torch, dev, case, bn, relu, need_grad_x=True):
    """Forward and backward of one case through the _bf16 ops: (device inputs, forward results,
    gradients)."""
    pooled = len(case) == 4
    d = {k: to_dev(torch, dev, v) for k, v in R.layer_inputs(case, bn).items()}
    fwd = ops.mlp_layer_train_pool_bf16 if pooled else ops.mlp_layer_train_bf16
    res = fwd(d["x"], d["w"], d["b"], d["gamma"], d["beta"], EPS, relu)
    stats = (res[2], res[3]) if bn else (None, None)
    tail = (d["x"], d["w"], res[1], *stats, d["gamma"], d["beta"], EPS, relu, need_grad_x)
    grads = (ops.mlp_layer_train_pool_bf16_grad(d["go"], res[4], *tail) if pooled
             else ops.mlp_layer_train_bf16_grad(d["go"], *tail))
    return d, res, grads, tail


OP_CASES = [(case, bn, relu) for case in R.LAYER_CASES + R.POOL_CASES
            for bn, relu in ((T, T), (F, F))]


def op_id(c):
    return R.shape_id(c[0]) + "-" + "".join("FT"[f] for f in c[1:])


@pytest.mark.parametrize("case,bn,relu", OP_CASES, ids=map(op_id, OP_CASES))
def test_ops_forward(env, case, bn, relu):
    pkg, ops, torch, dev = env
    d, res, _, _ = run_layer(ops, torch, dev, case, bn, relu)
    check_forward(torch, d["x"], d["w"], d["b"], d["gamma"], d["beta"], relu, len(case) == 4, res,
                  op_id((case, bn, relu)))


@pytest.mark.parametrize("case,bn,relu", OP_CASES, ids=map(op_id, OP_CASES))
def test_ops_backward(env, case, bn, relu):
    """grad_gamma, grad_beta and grad_b: the bits of the fp32 grad op on the same y, mean, var.
    grad_x and grad_w: the contract evaluated on the grad_y that pn2_bn_act_bwd / _pool_bwd
    return through the C ABI for the same inputs (without batch norm and ReLU, unpooled, that
    grad_y is grad_out exactly)."""
    pkg, ops, torch, dev = env
    pooled = len(case) == 4
    d, res, grads, tail = run_layer(ops, torch, dev, case, bn, relu)
    want32 = (ops.mlp_layer_train_pool_grad(d["go"], res[4], *tail) if pooled
              else ops.mlp_layer_train_grad(d["go"], *tail))
    for name, got, want in zip(("grad_b", "grad_gamma", "grad_beta"), grads[2:], want32[2:]):
        same_bits(got, want, name + " vs the fp32 grad op")
    stats = (res[2], res[3]) if bn else (None, None)
    gy, gg, gbeta = R.c_act_bwd(torch, d["go"], res[4] if pooled else None, res[1], *stats,
                                d["gamma"], d["beta"], relu)
    if not (bn or relu or pooled):
        same_bits(gy, d["go"], "grad_y = grad_out")
    if bn:
        same_bits(grads[3], gg, "grad_gamma vs the C ABI")
        same_bits(grads[4], gbeta, "grad_beta vs the C ABI")
    x, w, gyn = (t.cpu().numpy() for t in (d["x"], d["w"], gy))
    assert_close(grads[1], R.wgrad(x, gyn, "E"), R.wgrad(x, gyn, "E32"), "grad_w")
    assert_close(grads[0], R.grad_x(gyn, w, "E"), R.grad_x(gyn, w, "E32"), "grad_x")


@pytest.mark.parametrize("case", [R.LAYER_CASES[2], R.POOL_CASES[1]], ids=R.shape_id)
def test_ops_backward_without_grad_x(env, case):
    pkg, ops, torch, dev = env
    _, _, full, _ = run_layer(ops, torch, dev, case, T, T)
    _, _, grads, _ = run_layer(ops, torch, dev, case, T, T, need_grad_x=False)
    assert grads[0].shape == (0,)
    for name, a, b in zip(("grad_w", "grad_b", "grad_gamma", "grad_beta"), grads[1:], full[1:]):
        same_bits(a, b, name + " with and without grad_x")


def test_ops_zero_rows(env):
    pkg, ops, torch, dev = env
    z = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
    out, y, mean, var = ops.mlp_layer_train_bf16(z(0, 9), z(9, 32), z(32), z(32), z(32), EPS, True)
    assert out.shape == y.shape == (0, 32) and not mean.any() and not var.any()
    g = ops.mlp_layer_train_bf16_grad(z(0, 32), z(0, 9), z(9, 32), y, mean, var, z(32), z(32),
                                      EPS, True, True)
    assert g[0].shape == (0, 9) and all(not t.any() for t in g[1:])


# ------------------------------------------------------------------ 6. determinism ----------
BITS_CASES = [(case, bn, relu) for case in (R.LAYER_CASES[1], R.LAYER_CASES[3], R.POOL_CASES[1],
                                            R.POOL_CASES[3]) for bn, relu in ((T, T), (F, F))]
NAMES = ("out", "y", "mean", "var")
GRADS = ("grad_x", "grad_w", "grad_b", "grad_gamma", "grad_beta")


def outputs(ops, torch, dev, c):
    _, res, grads, _ = run_layer(ops, torch, dev, *c)
    names = NAMES + (("arg",) if len(c[0]) == 4 else ())
    return dict(zip(names + GRADS, tuple(res) + tuple(grads)))


def digests(outs):
    return {k: hashlib.sha256(np.ascontiguousarray(v.cpu().numpy()).tobytes()).hexdigest()
            for k, v in outs.items()}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_covers_the_cases(golden):
    assert len(golden["commit"]) == 40
    assert sorted(golden["digests"]) == sorted(map(op_id, BITS_CASES))


@pytest.mark.parametrize("c", BITS_CASES, ids=map(op_id, BITS_CASES))
def test_ops_bits(env, golden, c):
    """Two runs give equal bits, and they are the recorded ones."""
    pkg, ops, torch, dev = env
    first, second = outputs(ops, torch, dev, c), outputs(ops, torch, dev, c)
    for k in first:
        assert torch.equal(first[k], second[k]), f"{op_id(c)}: {k} differs between two runs"
    got, want = digests(first), golden["digests"][op_id(c)]
    assert sorted(got) == sorted(want)
    changed = [k for k in got if got[k] != want[k]]
    assert not changed, f"{op_id(c)}: bits differ from the recorded ones in {changed}"


# ------------------------------------------------------------------ 7. Python level ---------
SPIED = ("_torch_ops", "attention_layer", "tf_sampling", "tf_grouping", "tf_interpolate")


@pytest.fixture
def spy(env, monkeypatch):
    """(name, args, outputs) of every torch.ops.pn2 op the mirror modules call, in order (the
    recording spy of tests/test_gpu_model_train.py)."""
    pkg = env[0]
    entries, real = [], pkg._torch_ops.call

    def call(name, *args):
        out = real(name, *args)
        entries.append((name, args, out))
        return out
    for mod in SPIED:
        assert getattr(getattr(pkg, mod), "call") is real, mod
        monkeypatch.setattr(getattr(pkg, mod), "call", call)
    return entries


def layer_calls(entries):
    return [e for e in entries if e[0].startswith("mlp_layer_train")]


def test_modules_follow_train_precision(env, spy):
    pkg, ops, torch, dev = env
    pu, tu = pkg.pointnet_util, pkg.tf_util
    xyz_np, feats_np = pkg.synth.batch([0, 1], 2048, "scannet", with_features=True)
    xyz, feats = torch.from_numpy(xyz_np).to(dev), torch.from_numpy(feats_np).to(dev)
    store = tu.ParamStore(seed=3, train_precision="bf16").trainable(dev)
    new_xyz, sa, _ = pu.pointnet_sa_module(xyz, feats, 128, 0.2, 16, [32, 64], [32], False, True,
                                           None, "s1", params=store)
    pu.pointnet_sa_module(xyz, feats, None, None, None, [32, 64], None, True, True, None, "s2",
                          params=store)
    pu.pointnet_sa_module_msg(xyz, feats, 128, [0.1, 0.2], [8, 16], [[16, 32], [32, 48]], True,
                              None, "m1", params=store)
    pu.pointnet_fp_module(xyz, new_xyz, feats, sa, [64, 32], True, None, "f1", params=store)
    n_modules = len(layer_calls(spy))
    assert n_modules == 3 + 2 + 4 + 2
    pkg.pointnet2_sem_seg.model_body(xyz, None, True, 21, None, store, seed=1)
    torch.cuda.synchronize()
    calls = layer_calls(spy)
    names = [e[0] for e in calls]
    print("layer ops:", names)
    assert len(calls) == n_modules + 4 * 3 + (2 + 2 + 2 + 3) + 2
    # every MLP layer but fc2 ran a _bf16 op; fc2 (the last call, 21 logits) the fp32 one
    assert all(n.endswith("_bf16") for n in names[:-1])
    assert names[-1] == "mlp_layer_train" and calls[-1][1][1].shape[-1] == 21
    pooled = [n for n in names if n == "mlp_layer_train_pool_bf16"]
    assert len(pooled) == 1 + 1 + 2 + 4      # one per SSG module and per MSG scale
    for i, (name, args, res) in enumerate(calls[:-1]):
        x, w, b, gamma, beta, eps, relu = args
        assert eps == EPS
        with torch.no_grad():
            check_forward(torch, x, w, b, gamma, beta, relu, name.endswith("_pool_bf16"), res,
                          f"call {i} {name} {tuple(x.shape)}->{w.shape[-1]}")


def test_store_set_back_to_fp32_gives_the_fp32_bits(env, spy):
    pkg, ops, torch, dev = env
    pu, tu = pkg.pointnet_util, pkg.tf_util
    xyz_np, feats_np = pkg.synth.batch([0, 1], 1024, "scannet", with_features=True)
    xyz, feats0 = torch.from_numpy(xyz_np).to(dev), torch.from_numpy(feats_np).to(dev)

    def run(store):
        feats = feats0.clone().requires_grad_(True)
        for p in store.parameters():
            p.grad = None
        new_xyz, sa, _ = pu.pointnet_sa_module(xyz, feats, 128, 0.2, 16, [32, 64], None, False,
                                               True, None, "t1", params=store)
        fp = pu.pointnet_fp_module(xyz, new_xyz, feats, sa, [64, 32], True, None, "f1",
                                   params=store)
        fp.sum().backward()
        grads = {k: v.grad.clone() for k, v in store.items() if v.grad is not None}
        return fp.detach(), feats.grad, grads

    opted = tu.ParamStore(seed=9).trainable(dev).set_train_precision("bf16")
    fp16, _, _ = run(opted)
    assert all(n.endswith("_bf16") for n in (e[0] for e in layer_calls(spy)))
    del spy[:]
    opted.set_train_precision("fp32")
    fp_a, gf_a, gv_a = run(opted)
    assert not any(e[0].endswith("_bf16") for e in layer_calls(spy))
    fp_b, gf_b, gv_b = run(tu.ParamStore(seed=9).trainable(dev))
    assert not torch.equal(fp16, fp_b)            # the opt-in did change the arithmetic
    same_bits(fp_a, fp_b, "output")
    same_bits(gf_a, gf_b, "grad of the features")
    assert sorted(gv_a) == sorted(gv_b) and len(gv_a) == 16
    for k in gv_a:
        same_bits(gv_a[k], gv_b[k], "grad " + k)
    # an inference-only opt-in still trains in fp32
    fp_c, _, _ = run(tu.ParamStore(seed=9, precision="bf16").trainable(dev))
    same_bits(fp_c, fp_b, "output of a store with only precision=bf16")


# ------------------------------------------------------------------ 8. descent --------------
def test_bf16_training_descends_like_fp32(env):
    """30 train_steps of pointnet2_sem_seg on one fixed batch (B = 2, N = 2,048, labels by
    height, a fixed dropout seed) at each precision from equal initial values. Both losses stay
    finite, and the bf16 run's drop from its first loss is at least half the fp32 run's. Half is
    a floor, not a measurement: the per-operand relative error is 2^-8, so only a wrong gradient
    (a sign, a transposed tile, lost rows) comes near it."""
    pkg, ops, torch, dev = env
    B, N, C, steps = 2, 2048, 21, 30
    xyz_np = pkg.synth.batch([0, 1], N, "scannet")[0]
    z = xyz_np[..., 2]
    lab = 1 + np.clip((z - z.min()) / (z.max() - z.min() + 1e-9) * 5, 0, 4).astype(np.int32)
    rng = np.random.default_rng(8)
    lab[rng.random((B, N)) < 0.2] = 0                   # unannotated points: weight 0
    smpw_np = (rng.uniform(0.5, 2.0, (B, N)) * (lab > 0)).astype(np.float32)
    xyz, labels, smpw = (torch.from_numpy(a).to(dev) for a in (xyz_np, lab, smpw_np))
    curves = {}
    for prec in ("fp32", "bf16"):
        store = pkg.tf_util.ParamStore(seed=4, train_precision=prec).trainable(dev)
        opt, metrics = pkg.train.AdamOptimizer(store), pkg.train.SegMetrics(C, dev)
        losses = [pkg.train.train_step(store, opt, metrics, xyz, labels, smpw, C, bn_decay=0.5,
                                       seed=1)[0] for _ in range(steps)]
        curves[prec] = torch.stack(losses).cpu().numpy().astype(np.float64)
        print(prec, "loss:", " ".join(f"{v:.4f}" for v in curves[prec]))
    for prec, c in curves.items():
        assert np.isfinite(c).all(), prec
    drop = {p: c[0] - c[-1] for p, c in curves.items()}
    print(f"drop fp32 {drop['fp32']:.4f} bf16 {drop['bf16']:.4f}")
    assert drop["fp32"] > 0, "the fp32 run itself does not descend: the test shows nothing"
    assert drop["bf16"] >= 0.5 * drop["fp32"]


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", action="store_true", required=True)
    ap.add_argument("--commit", required=True, help="the commit whose build is being recorded")
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args()
    import torch
    import pn2hip
    recorded = {op_id(c): digests(outputs(pn2hip.ops, torch, torch.device("cuda:0"), c))
                for c in BITS_CASES}
    with open(a.out, "w") as f:
        json.dump({"commit": a.commit, "digests": recorded}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded", len(recorded), "cases at", a.commit, "->", a.out)
