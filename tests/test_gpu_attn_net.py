"""GPU: the attention networks' reductions (csrc/attn_net.hip: pn2_attn_reduce_kd / _grad,
pn2_head_mix / _grad) through torch.ops.pn2 and the C ABI, and the layers and models built on them
(attention_layer.AttentionNetLayer, AttentionNetMLPLayer, pooling_attention_layer, attention_models,
pooling_attention_model).

References: tests/attn_net_ref.py evaluated on the CPU in float64 and in float32; the acceptance
rule is the project's (tests/support.py):

    max |gpu - f64|  <=  max(4 * max |fp32 - f64|,  1e-6 * (1 + max |f64|))

Outputs of C-ABI calls are pre-filled with NaN, so an element that is not written fails.

Grid caps, each with a case one step past it: the reduction kernels stride beyond
4 * PN2_ATTN_NET_MAX_BLOCKS = 16384 (group, head) wave tasks, the head-mixing kernels beyond 16384
wave tasks of 64 / (key_dim / 4) rows.
"""
import functools
import importlib

import numpy as np
import pytest

import attn_net_ref as R
from conftest import PKG_NAME
from support import assert_close, gpu_marks, same_bits

pytestmark = gpu_marks

# (G, ns, H, kd[, scale])
REDUCE_CASES = [
    (3, 32, 16, 8), (3, 32, 16, 16), (2, 32, 16, 32), (2, 32, 16, 64),   # the net layers
    (2, 32, 16, 128), (1, 32, 16, 256), (1, 32, 16, 512),                # the pooling model
    (2, 32, 4, 4),           # key_dim 4: pn2_attn_reduce itself
    (2, 16, 16, 8), (2, 64, 2, 64), (2, 128, 1, 256),
    (3, 5, 3, 8), (2, 33, 1, 20),   # rows that do not fill the last wave load
    (2, 1, 2, 16),           # a single key
    (2, 200, 2, 32),         # group_all-like
    (3, 7, 5, 12),           # kd / 4 is no power of two
    (2, 5, 2, 260),          # the same with two float4 per lane (kd / 4 = 65 > a wave)
    (3, 32, 4, 16, 30.0),    # scores in the hundreds: the max subtraction matters
    (4100, 2, 4, 8),         # 16400 (group, head) tasks: past the grid cap
]
# (rows, H, kd)
MIX_CASES = [(1, 5, 8), (70, 5, 8), (65, 5, 16), (3, 5, 32), (5, 5, 64), (7, 1, 4), (9, 8, 4),
             (5, 3, 12),
             (32 * 16384 + 40, 2, 8)]   # 16386 wave tasks of 32 rows: past the grid cap


def ids(case):
    return "x".join(str(v) for v in case)


@pytest.fixture(scope="module")
def env():
    import torch
    pkg = importlib.import_module(PKG_NAME)
    import pn2hip
    return pkg, pn2hip.ops, torch, torch.device("cuda:0")


def draw(torch, seed, *shapes, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return [((torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1) * scale).float()
            for s in shapes]


def ref_with_grads(torch, fn, inputs, go, dt):
    """(out, grads of sum(go * out)) of fn on CPU copies of `inputs` in dtype dt."""
    L = [t.to(dt).clone().requires_grad_(True) for t in inputs]
    out = fn(*L)
    (out * go.to(dt)).sum().backward()
    return out.detach(), [t.grad for t in L]


@functools.lru_cache(maxsize=None)
def run_reduce(case):
    import torch
    import pn2hip
    pkg = importlib.import_module(PKG_NAME)
    ops, dev = pn2hip.ops, torch.device("cuda:0")
    G, ns, H, kd = case[:4]
    scale = case[4] if len(case) > 4 else 1.0
    C = H * kd
    Q, K, V, go = draw(torch, 7 * G + ns + 3 * H + kd, (1, G, C), (1, G, ns, C), (1, G, ns, C),
                       (1, G, C), scale=scale)
    go = go / scale
    d = [t.to(dev) for t in (Q, K, V, go)]
    runs = []
    for _ in range(2):
        out = ops.attn_reduce_kd(*d[:3], kd)
        runs.append((out,) + tuple(ops.attn_reduce_kd_grad(*d, kd)))
    # the C ABI on NaN-filled outputs
    nan = lambda t: torch.full_like(t, float("nan"))  # noqa: E731
    c_out, c_gq, c_gk, c_gv = nan(d[0]), nan(d[0]), nan(d[1]), nan(d[2])
    L, lib = pkg._lib, pkg.lib()
    s = L.stream_of(d[0])
    L.check(lib.pn2_attn_reduce_kd(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), 1, G, ns, C,
                                   kd, c_out.data_ptr(), s), "attn_reduce_kd")
    L.check(lib.pn2_attn_reduce_kd_grad(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(),
                                        d[3].data_ptr(), 1, G, ns, C, kd, c_gq.data_ptr(),
                                        c_gk.data_ptr(), c_gv.data_ptr(), s), "attn_reduce_kd_grad")
    torch.cuda.synchronize()
    fn = lambda q, k, v: R.attn_reduce(q, k, v, kd)  # noqa: E731
    refs = {dt: ref_with_grads(torch, fn, (Q, K, V), go, dt)
            for dt in (torch.float64, torch.float32)}
    return d, runs, (c_out, c_gq, c_gk, c_gv), refs


@pytest.mark.parametrize("case", REDUCE_CASES, ids=ids)
def test_reduce_forward_and_backward(env, case):
    pkg, ops, torch, dev = env
    d, runs, c, refs = run_reduce(case)
    (o64, g64), (o32, g32) = refs[torch.float64], refs[torch.float32]
    assert_close(runs[0][0], o64, o32, "out")
    for name, got, a, b in zip(("grad_Q", "grad_K", "grad_V"), runs[0][1:], g64, g32):
        assert_close(got, a, b, name)


@pytest.mark.parametrize("case", REDUCE_CASES, ids=ids)
def test_reduce_is_reproducible_and_c_abi_agrees(env, case):
    pkg, ops, torch, dev = env
    d, runs, c, _ = run_reduce(case)
    for name, first, second, cabi in zip(("out", "grad_Q", "grad_K", "grad_V"), *runs, c):
        same_bits(first, second, f"{name}: second run")
        same_bits(first, cabi, f"{name}: C ABI")   # (a NaN left in a C-ABI output fails here)


def test_key_dim_4_is_attn_reduce(env):
    pkg, ops, torch, dev = env
    d, runs, c, _ = run_reduce((2, 32, 4, 4))
    same_bits(runs[0][0], ops.attn_reduce(*d[:3]), "out")
    for name, got, old in zip(("grad_Q", "grad_K", "grad_V"), runs[0][1:],
                              ops.attn_reduce_grad(*d)):
        same_bits(got, old, name)
    out = pkg.attention_layer.attention_reduce(*d[:3])   # the default keeps today's call
    same_bits(out, runs[0][0], "attention_reduce")


def test_reduce_autograd(env):
    """attention_reduce(Q, K, V, key_dim) differentiates through pn2_attn_reduce_kd_grad."""
    pkg, ops, torch, dev = env
    d, runs, _, _ = run_reduce((3, 32, 16, 8))
    leaves = [t.clone().requires_grad_(True) for t in d[:3]]
    out = pkg.attention_layer.attention_reduce(*leaves, key_dim=8)
    (out * d[3]).sum().backward()
    same_bits(out, runs[0][0], "out")
    for name, leaf, want in zip(("grad_Q", "grad_K", "grad_V"), leaves, runs[0][1:]):
        same_bits(leaf.grad, want, name)


@functools.lru_cache(maxsize=None)
def run_mix(case):
    import torch
    import pn2hip
    pkg = importlib.import_module(PKG_NAME)
    ops, dev = pn2hip.ops, torch.device("cuda:0")
    rows, H, kd = case
    qkv, go = draw(torch, rows % 1000 + 5 * H + kd, (rows, 3 * H * kd), (rows, H * kd))
    qkv = qkv * 2   # scores of a few units
    d = [qkv.to(dev), go.to(dev)]
    runs = [(ops.head_mix(d[0], H, kd), ops.head_mix_grad(d[0], d[1], H, kd)) for _ in range(2)]
    c_out, c_g = torch.full_like(d[1], float("nan")), torch.full_like(d[0], float("nan"))
    L, lib = pkg._lib, pkg.lib()
    s = L.stream_of(d[0])
    L.check(lib.pn2_head_mix(d[0].data_ptr(), rows, H, kd, c_out.data_ptr(), s), "head_mix")
    L.check(lib.pn2_head_mix_grad(d[0].data_ptr(), d[1].data_ptr(), rows, H, kd, c_g.data_ptr(),
                                  s), "head_mix_grad")
    torch.cuda.synchronize()
    fn = lambda x: R.head_mix(x, H, kd)  # noqa: E731
    refs = {dt: ref_with_grads(torch, fn, (qkv,), go, dt) for dt in (torch.float64, torch.float32)}
    return d, runs, (c_out, c_g), refs


@pytest.mark.parametrize("case", MIX_CASES, ids=ids)
def test_head_mix(env, case):
    pkg, ops, torch, dev = env
    d, runs, c, refs = run_mix(case)
    (o64, g64), (o32, g32) = refs[torch.float64], refs[torch.float32]
    assert_close(runs[0][0], o64, o32, "out")
    assert_close(runs[0][1], g64[0], g32[0], "grad_qkv")
    for name, first, second, cabi in zip(("out", "grad_qkv"), *runs, c):
        same_bits(first, second, f"{name}: second run")
        same_bits(first, cabi, f"{name}: C ABI")


def test_head_mix_autograd_and_leading_axes(env):
    pkg, ops, torch, dev = env
    d, runs, _, _ = run_mix((70, 5, 8))
    x = d[0].reshape(2, 5, 7, -1).clone().requires_grad_(True)
    out = ops.head_mix(x, 5, 8)
    assert out.shape == (2, 5, 7, 40)
    (out * d[1].reshape(out.shape)).sum().backward()
    same_bits(out.reshape(70, 40), runs[0][0], "out")
    same_bits(x.grad.reshape(70, -1), runs[0][1], "grad_qkv")


# ------------------------------------------------------------------------------- the layers
LAYER_KINDS = ("net", "mlp", "pooling")
B, N, NPOINT, NSAMPLE, OUT_DIM, RADIUS, CIN = 2, 128, 16, 8, 8, 0.35, 5


def make_layer(pkg, kind, store):
    A = pkg.attention_layer
    kw = dict(npoint=NPOINT, out_dim=OUT_DIM, radius=RADIUS, nsample=NSAMPLE, scope="L",
              params=store)
    if kind == "net":
        return A.AttentionNetLayer(inner_dimensions=[8], **kw)
    if kind == "mlp":
        return A.AttentionNetMLPLayer(inner_dimensions=[8, 8], **kw)
    return pkg.pooling_attention_layer.PoolingAttentionNetLayer(None, [8, 8, 8], **kw)


def layer_ref(kind, w, grouped, new_xyz, training):
    if kind == "net":
        return R.attention_net_layer(w, "L", grouped, OUT_DIM, 1)
    if kind == "mlp":
        return R.attention_net_mlp_layer(w, "L", grouped, OUT_DIM, 2)
    return R.pooling_attention_net_layer(w, "L", grouped, new_xyz, OUT_DIM, 3, training)


def layer_inputs(pkg, torch):
    from support import clouds
    xyz = torch.from_numpy(clouds(pkg, "uniform", B, N, seed=3))
    points, go = draw(torch, 11, (B, N, CIN), (B, NPOINT, 16 * OUT_DIM))
    return xyz, points, go


@functools.lru_cache(maxsize=None)
def run_layer(kind, training):
    """The layer on the GPU (inference on a plain store, or training on a trainable one with the
    gradients of sum(go * out)), and the restatement on the layer's own new_xyz and idx in
    float64 and float32 with autograd for every variable and for `points`."""
    import torch
    pkg = importlib.import_module(PKG_NAME)
    dev = torch.device("cuda:0")
    xyz, points, go = layer_inputs(pkg, torch)
    store = pkg.tf_util.ParamStore(seed=5)
    if training:
        store = store.trainable(dev)
    layer = make_layer(pkg, kind, store)
    p = points.to(dev).requires_grad_(training)
    new_xyz, out, idx = layer([xyz.to(dev), p], is_training=training)
    got = {}
    if training:
        (out * go.to(dev)).sum().backward()
        got = {k: v.grad for k, v in store.items() if v.requires_grad}
        got["points"] = p.grad
    torch.cuda.synchronize()
    # distinct points per group: the radius must not leave the groups to their first neighbour
    distinct = np.mean([len(set(g.tolist())) for g in idx.cpu().numpy().reshape(-1, NSAMPLE)])
    refs = {}
    for dt in (torch.float64, torch.float32):
        w = {k: torch.from_numpy(v).to(dt).requires_grad_(training)
             for k, v in store.state_dict().items()}
        pts = points.to(dt).requires_grad_(training)
        grouped = R.group(xyz.to(dt), pts, new_xyz.cpu().to(dt), idx.cpu())
        ref = layer_ref(kind, w, grouped, new_xyz.cpu().to(dt), training)
        grads = {}
        if training:
            (ref * go.to(dt)).sum().backward()
            grads = {k: v.grad for k, v in w.items()}
            grads["points"] = pts.grad
        refs[dt] = (ref.detach(), grads)
    return out.detach(), got, refs, distinct, (new_xyz, idx)


@pytest.mark.parametrize("kind", LAYER_KINDS)
def test_layer_forward(env, kind):
    pkg, ops, torch, dev = env
    for training in (False, True):
        out, _, refs, distinct, (new_xyz, idx) = run_layer(kind, training)
        assert distinct >= 3, f"groups hold {distinct:.1f} distinct points on average"
        assert out.shape == (B, NPOINT, 16 * OUT_DIM) and new_xyz.shape == (B, NPOINT, 3)
        assert idx.shape == (B, NPOINT, NSAMPLE) and idx.dtype == torch.int32
        assert_close(out, refs[torch.float64][0], refs[torch.float32][0],
                     f"{kind} out (is_training={training})")


@pytest.mark.parametrize("kind", LAYER_KINDS)
def test_layer_gradients(env, kind):
    """On a trainable store with is_training=True: a gradient for every variable and for
    `points`, against float64 autograd of the restatement (the pooling layer's batch norm on the
    batch statistics)."""
    pkg, ops, torch, dev = env
    _, got, refs, _, _ = run_layer(kind, True)
    g64, g32 = refs[torch.float64][1], refs[torch.float32][1]
    trainable = {k for k in g64 if not k.endswith(("moving_mean", "moving_variance"))}
    assert set(got) == trainable, sorted(set(got) ^ trainable)
    for k in sorted(trainable):
        assert got[k] is not None, f"{k}: no gradient"
        assert_close(got[k], g64[k], g32[k], "grad " + k)


# ------------------------------------------------------------------------------- the models
MODELS = ("AttentionNetModel", "AttentionNetFeatureModel", "AttentionNetMLPModel",
          "PoolingAttentionNetModel")
MB, MN, NUM_CLASS, MODEL_NPOINTS, MODEL_RADIUS = 2, 256, 21, (64, 16, 8, 4), 0.3


def make_model(pkg, name, store, is_training):
    mod = pkg.pooling_attention_model if name.startswith("Pooling") else pkg.attention_models
    return getattr(mod, name)(is_training, None, NUM_CLASS, params=store, npoints=MODEL_NPOINTS,
                              radius=MODEL_RADIUS, seed=9)


def model_inputs(pkg, torch, name, dev):
    from support import clouds
    xyz = torch.from_numpy(clouds(pkg, "uniform", MB, MN, seed=1)).to(dev)
    feats, = draw(torch, 2, (MB, MN, 6))
    g = torch.Generator().manual_seed(4)
    labels = torch.randint(0, NUM_CLASS, (MB, MN), generator=g, dtype=torch.int32).to(dev)
    smpw = (labels > 0).float() * 1.5
    return xyz, (feats.to(dev) if "Feature" in name else None), labels, smpw


@pytest.mark.parametrize("name", MODELS)
def test_model_forward(env, name):
    pkg, ops, torch, dev = env
    store = pkg.tf_util.ParamStore(seed=2)
    model = make_model(pkg, name, store, False)
    xyz, feats, _, _ = model_inputs(pkg, torch, name, dev)
    inputs = xyz if feats is None else (xyz, feats)
    logits = model(inputs)
    again = model(inputs)
    assert logits.shape == (MB, MN, NUM_CLASS) and logits.dtype == torch.float32
    assert torch.isfinite(logits).all()
    same_bits(logits, again, "second call")
    end = model.get_end_points(inputs)
    assert end["feats"].shape == (MB, MN, 128) and end["l0_xyz"] is xyz


@pytest.mark.parametrize("name", MODELS)
def test_model_takes_a_training_step(env, name):
    """One train_step_with on a trainable store: every variable has a finite gradient, and
    AdamOptimizer has moved it. A bias in front of a batch norm is the one exception to `moved`:
    its gradient is zero by construction (the batch mean removes it), and the HIP training layer
    returns that zero exactly, so Adam leaves it where it was.

    The step is taken with Adam's epsilon at 1e-30, not TF's default 1e-8. These networks have no
    normalisation between their Dense layers, so at initialisation the activations shrink from
    level to level and the softmax of the deep layers is all but uniform: the query and key
    kernels of l3 and l4 receive gradients of 1e-16 to 1e-29 here (measured; their biases 1e-10 to
    1e-18). Against epsilon = 1e-8 such a gradient moves an fp32 variable by less than its last
    bit; with 1e-30 every non-zero gradient shows as a move, which is what this test is about."""
    pkg, ops, torch, dev = env
    store = pkg.tf_util.ParamStore(seed=2).trainable(dev)
    model = make_model(pkg, name, store, True)
    xyz, feats, labels, smpw = model_inputs(pkg, torch, name, dev)
    with torch.no_grad():   # creates every variable
        model.body(xyz, feats, False, NUM_CLASS, None, store)
    before = store.state_dict()
    opt = pkg.train.AdamOptimizer(store, epsilon=1e-30)
    metrics = pkg.train.SegMetrics(NUM_CLASS)
    loss, _ = pkg.train.train_step_with(model.body, store, opt, metrics, xyz, labels, smpw,
                                        NUM_CLASS, features=feats, seed=9)
    assert torch.isfinite(loss) and sorted(store) == sorted(before)
    leaves = dict(opt.named_parameters())
    assert leaves and all(not k.endswith(("moving_mean", "moving_variance")) for k in leaves)
    for k, p in leaves.items():
        assert p.grad is not None, f"{k}: no gradient"
        assert torch.isfinite(p.grad).all(), f"{k}: non-finite gradient"
        under_bn = k.endswith("/biases") and k[:-len("biases")] + "bn/gamma" in store
        if not under_bn:
            assert not np.array_equal(p.detach().cpu().numpy(), before[k]), f"{k} did not move"
