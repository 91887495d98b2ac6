"""CPU: the attention networks' reductions (csrc/attn_net.hip: torch.ops.pn2.attn_reduce_kd /
_grad, head_mix / _grad) and the layers above them: schemas, Meta shapes, argument errors, the C
entry points' checks (PN2_EINVAL before any launch), the restatements of tests/attn_net_ref.py
against the oracle, and that the layers and models construct. No kernel runs here;
tests/test_gpu_attn_net.py runs them on the MI355X."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import attn_net_ref as R

E = -22
ENTRY_POINTS = ("pn2_attn_reduce_kd", "pn2_attn_reduce_kd_grad", "pn2_head_mix",
                "pn2_head_mix_grad")
OPS = ("attn_reduce_kd", "attn_reduce_kd_grad", "head_mix", "head_mix_grad")


@pytest.fixture(scope="module")
def ops():
    import pn2hip
    return pn2hip.ops


def m(*s, dt=torch.float32):
    return torch.empty(s, device="meta", dtype=dt)


def test_schemas(ops):
    assert str(ops.attn_reduce_kd._schemas[""]) == (
        "pn2::attn_reduce_kd(Tensor Q, Tensor K, Tensor V, int key_dim) -> Tensor")
    assert str(ops.attn_reduce_kd_grad._schemas[""]) == (
        "pn2::attn_reduce_kd_grad(Tensor Q, Tensor K, Tensor V, Tensor grad_out, int key_dim) -> "
        "(Tensor, Tensor, Tensor)")
    assert str(ops.head_mix._schemas[""]) == (
        "pn2::head_mix(Tensor qkv, int heads, int key_dim) -> Tensor")
    assert str(ops.head_mix_grad._schemas[""]) == (
        "pn2::head_mix_grad(Tensor qkv, Tensor grad_out, int heads, int key_dim) -> Tensor")
    assert ops.ATTN_NET_NAMES == OPS
    for name in OPS:
        assert name in ops.__all__ and name not in ops.NAMES + ops.HOST_NAMES
        has = lambda key: torch._C._dispatch_has_kernel_for_dispatch_key(f"pn2::{name}", key)  # noqa: E731
        assert has("CUDA") and has("Meta") and not has("CPU")
    for name in ("attn_reduce_kd", "head_mix"):
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f"pn2::{name}", "Autograd")


def test_meta_shapes_dtypes_and_strides(ops):
    Q, K = m(2, 7, 128), m(2, 7, 32, 128)
    out = ops.attn_reduce_kd(Q, K, K, 8)
    assert out.shape == (2, 7, 128) and out.dtype == torch.float32 and out.is_contiguous()
    gq, gk, gv = ops.attn_reduce_kd_grad(Q, K, K, out, 8)
    assert gq.shape == Q.shape and gk.shape == gv.shape == K.shape
    assert all(g.dtype == torch.float32 and g.is_contiguous() for g in (gq, gk, gv))
    # a strided input is taken as its contiguous copy; key_dim = C is one head; no groups
    assert ops.attn_reduce_kd(m(2, 7, 256)[..., ::2], K, K, 16).stride() == (7 * 128, 128, 1)
    assert ops.attn_reduce_kd(m(1, 3, 512), m(1, 3, 5, 512), m(1, 3, 5, 512), 512).shape == (1, 3, 512)
    assert ops.attn_reduce_kd(m(0, 3, 16), m(0, 3, 5, 16), m(0, 3, 5, 16), 8).shape == (0, 3, 16)
    qkv = m(2, 16, 8, 120)
    out = ops.head_mix(qkv, 5, 8)
    assert out.shape == (2, 16, 8, 40) and out.dtype == torch.float32 and out.is_contiguous()
    g = ops.head_mix_grad(qkv, out, 5, 8)
    assert g.shape == qkv.shape and g.dtype == torch.float32 and g.is_contiguous()
    assert ops.head_mix(m(12), 1, 4).shape == (4,)
    assert ops.head_mix(m(0, 24), 2, 4).shape == (0, 8)


def test_autograd_on_meta_tensors(ops):
    g = lambda *s: torch.empty(s, device="meta", requires_grad=True)  # noqa: E731
    Q, K, V = g(2, 3, 32), g(2, 3, 5, 32), g(2, 3, 5, 32)
    ops.attn_reduce_kd(Q, K, V, 16).sum().backward()
    assert Q.grad.shape == Q.shape and K.grad.shape == K.shape and V.grad.shape == V.shape
    qkv = g(6, 4, 48)
    ops.head_mix(qkv, 2, 8).sum().backward()
    assert qkv.grad.shape == qkv.shape


@pytest.mark.parametrize("call", [
    lambda o: o.attn_reduce_kd(m(2, 3, 24), m(2, 3, 5, 24), m(2, 3, 5, 24), 6),       # kd % 4
    lambda o: o.attn_reduce_kd(m(2, 3, 24), m(2, 3, 5, 24), m(2, 3, 5, 24), 0),       # kd < 4
    lambda o: o.attn_reduce_kd(m(2, 3, 24), m(2, 3, 5, 24), m(2, 3, 5, 24), 16),      # C % kd
    lambda o: o.attn_reduce_kd(m(2, 3, 1032), m(2, 3, 5, 1032), m(2, 3, 5, 1032), 516),  # kd > 512
    lambda o: o.attn_reduce_kd(m(2, 3, 16), m(2, 3, 0, 16), m(2, 3, 0, 16), 8),       # ns = 0
    lambda o: o.attn_reduce_kd(m(2, 3, 16), m(2, 4, 5, 16), m(2, 4, 5, 16), 8),       # M differs
    lambda o: o.attn_reduce_kd(m(2, 3, 16), m(2, 3, 5, 16), m(2, 3, 6, 16), 8),       # V != K
    lambda o: o.attn_reduce_kd(m(6, 16), m(6, 5, 16), m(6, 5, 16), 8),                # ranks
    lambda o: o.attn_reduce_kd_grad(m(2, 3, 16), m(2, 3, 5, 16), m(2, 3, 5, 16), m(2, 3, 8), 8),
    lambda o: o.attn_reduce_kd_grad(m(2, 3, 16), m(2, 3, 5, 16), m(2, 3, 5, 16), m(2, 3, 16), 12),
    lambda o: o.head_mix(m(4, 120), 9, 4),                                            # heads > 8
    lambda o: o.head_mix(m(4, 120), 0, 8),                                            # heads < 1
    lambda o: o.head_mix(m(4, 90), 5, 6),                                             # kd % 4
    lambda o: o.head_mix(m(4, 3 * 260), 1, 260),                                      # kd > 256
    lambda o: o.head_mix(m(4, 100), 5, 8),                                            # width
    lambda o: o.head_mix_grad(m(4, 120), m(4, 120), 5, 8),                            # grad width
    lambda o: o.head_mix_grad(m(4, 120), m(3, 40), 5, 8),                             # grad rows
])
def test_argument_errors(ops, call):
    with pytest.raises(ValueError):
        call(ops)


def test_no_cpu_kernel(ops):
    z = torch.zeros
    with pytest.raises(NotImplementedError):
        ops.attn_reduce_kd(z(1, 2, 16), z(1, 2, 3, 16), z(1, 2, 3, 16), 8)
    with pytest.raises(NotImplementedError):
        ops.attn_reduce_kd_grad(z(1, 2, 16), z(1, 2, 3, 16), z(1, 2, 3, 16), z(1, 2, 16), 8)
    with pytest.raises(NotImplementedError):
        ops.head_mix(z(4, 120), 5, 8)
    with pytest.raises(NotImplementedError):
        ops.head_mix_grad(z(4, 120), z(4, 40), 5, 8)


def test_entry_points_are_declared_exported_and_bound(pn2):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "pn2hip.h")).read(),
                  flags=re.S)
    exported = subprocess.run(["nm", "-D", "--defined-only", pn2.LIB_PATH], capture_output=True,
                              text=True, check=True).stdout
    for name in ENTRY_POINTS:
        assert re.search(rf"\b{name}\s*\(", text), f"{name} not declared in pn2hip.h"
        assert re.search(rf"\bT {name}$", exported, re.M), f"{name} not exported"
        assert name in pn2._lib.SIGNATURES
        assert getattr(pn2.lib(), name) is not None
    assert pn2._lib.PN2_HEAD_MIX_MAX_HEADS == 8 and pn2._lib.PN2_ATTN_NET_MAX_BLOCKS == 4096


def test_reduction_entry_points_check_arguments_without_launching(pn2):
    lib = pn2.lib()
    fake = 1 << 20  # 16-byte aligned, never dereferenced by the checks

    def fwd(**kw):
        names = ("Q", "K", "V", "B", "M", "ns", "C", "key_dim", "out", "stream")
        args = dict(zip(names, (fake, fake, fake, 2, 5, 32, 128, 8, fake, None)))
        args.update(kw)
        return lib.pn2_attn_reduce_kd(*[args[n] for n in names])

    def bwd(**kw):
        names = ("Q", "K", "V", "grad_out", "B", "M", "ns", "C", "key_dim", "grad_Q", "grad_K",
                 "grad_V", "stream")
        args = dict(zip(names, (fake, fake, fake, fake, 2, 5, 32, 128, 8, fake, fake, fake, None)))
        args.update(kw)
        return lib.pn2_attn_reduce_kd_grad(*[args[n] for n in names])

    for fn, bufs in ((fwd, ("Q", "K", "V", "out")),
                     (bwd, ("Q", "K", "V", "grad_out", "grad_Q", "grad_K", "grad_V"))):
        for name in bufs:
            assert fn(**{name: None}) == E, name            # null
            assert fn(**{name: fake + 4}) == E, name        # not 16-byte aligned
            assert fn(**{name: fake + 8}) == E, name
        for kw in (dict(key_dim=6), dict(key_dim=0), dict(key_dim=-8), dict(key_dim=2),
                   dict(key_dim=516, C=1032), dict(key_dim=1024, C=1024),   # kd > 512
                   dict(C=100), dict(C=132, key_dim=16),                     # C % kd
                   dict(ns=0), dict(ns=-1), dict(B=-1), dict(M=-1), dict(C=-8)):
            assert fn(**kw) == E, kw
        assert fn(B=1 << 16, M=1 << 16) == E                # groups are indexed in 31 bits
        # key_dim 4 is pn2_attn_reduce / _grad: their checks
        assert fn(key_dim=4, C=6) == E and fn(key_dim=4, ns=0) == E
        assert fn(key_dim=4, **{bufs[0]: fake + 4}) == E
        # no groups: a no-op that returns 0, whatever the buffers; the shape is checked first
        assert fn(B=0) == 0 and fn(M=0) == 0 and fn(M=0, key_dim=4, C=16) == 0
        assert fn(B=0, **{n: None for n in bufs}) == 0
        assert fn(B=0, key_dim=6) == E and fn(B=0, C=100) == E


def test_head_mix_entry_points_check_arguments_without_launching(pn2):
    lib = pn2.lib()
    fake = 1 << 20

    def fwd(**kw):
        names = ("qkv", "rows", "heads", "key_dim", "out", "stream")
        args = dict(zip(names, (fake, 100, 5, 8, fake, None)))
        args.update(kw)
        return lib.pn2_head_mix(*[args[n] for n in names])

    def bwd(**kw):
        names = ("qkv", "grad_out", "rows", "heads", "key_dim", "grad_qkv", "stream")
        args = dict(zip(names, (fake, fake, 100, 5, 8, fake, None)))
        args.update(kw)
        return lib.pn2_head_mix_grad(*[args[n] for n in names])

    for fn, bufs in ((fwd, ("qkv", "out")), (bwd, ("qkv", "grad_out", "grad_qkv"))):
        for name in bufs:
            assert fn(**{name: None}) == E, name
            assert fn(**{name: fake + 4}) == E, name
        for kw in (dict(heads=9), dict(heads=0), dict(heads=-1), dict(key_dim=6), dict(key_dim=0),
                   dict(key_dim=260), dict(key_dim=512), dict(rows=-1)):
            assert fn(**kw) == E, kw
        assert fn(rows=0) == 0 and fn(rows=0, **{n: None for n in bufs}) == 0
        assert fn(rows=0, heads=9) == E


def test_restated_reduction_at_key_dim_4_is_the_oracle(orc):
    rng = np.random.default_rng(5)
    B, M, ns, C = 2, 5, 7, 24
    Q = rng.standard_normal((B, M, C)).astype(np.float32)
    K = rng.standard_normal((B, M, ns, C)).astype(np.float32)
    V = rng.standard_normal((B, M, ns, C)).astype(np.float32)
    want = orc.attn_reduce(Q, K, V)
    got = R.attn_reduce(*(torch.from_numpy(a) for a in (Q, K, V)), 4).numpy()
    assert np.abs(got - want).max() <= 1e-6


def test_restated_head_mix_is_per_head_softmax_attention():
    """Against the formula written out with loops, in float64."""
    g = torch.Generator().manual_seed(1)
    rows, H, kd = 3, 5, 8
    qkv = torch.rand(rows, 3 * H * kd, generator=g, dtype=torch.float64) * 4 - 2
    got = R.head_mix(qkv, H, kd)
    for r in range(rows):
        q, k, v = qkv[r].reshape(3, H, kd)
        for i in range(H):
            s = torch.stack([q[i] @ k[j] for j in range(H)]) / kd ** 0.5
            a = torch.exp(s - s.max())
            a = a / a.sum()
            want = sum(a[j] * v[j] for j in range(H))
            assert torch.allclose(got[r, i * kd:(i + 1) * kd], want, rtol=0, atol=1e-12)


def test_layers_and_models_construct(pn2):
    A = pn2.attention_layer
    layer = A.AttentionLayer(8, 8)
    assert layer.key_net.out_features == 128 and layer.num_heads == 16
    assert A.AttentionLayer(64, 64, in_dim=64, query_dim=3).query_net.in_features == 3
    assert A.AttentionLayer(4, 4, 8).key_net.out_features == 32   # the SA modules' use
    store = pn2.tf_util.ParamStore(seed=1)
    net = A.AttentionNetLayer(npoint=16, out_dim=8, inner_dimensions=[8], params=store)
    assert net.key_dim == 8 and len(net.inner_blocks) == 1 and net.nsample == 32
    assert isinstance(net.inner_blocks[0].attention_layer, A.InnerAttentionLayer)
    assert net.inner_blocks[0].attention_layer.num_heads == 5
    mlp = A.AttentionNetMLPLayer(npoint=16, out_dim=16, inner_dimensions=[16] * 4, scope="l1")
    assert [b.scope for b in mlp.inner_blocks] == [f"l1/feed_forward_{i}" for i in range(4)]
    pool = pn2.pooling_attention_layer.PoolingAttentionNetLayer(None, [32, 32, 64], npoint=1024,
                                                                out_dim=64)
    assert pool.key_dim == 64 and pool.mlp == [32, 32, 64]
    for mod, names in ((pn2.attention_models, ("AttentionNetModel", "AttentionNetFeatureModel",
                                               "AttentionNetMLPModel")),
                       (pn2.pooling_attention_model, ("PoolingAttentionNetModel",))):
        for name in names:
            model = getattr(mod, name)(False, None, 21, params=store)
            assert [layer.npoint for layer in model.layers] == [1024, 256, 64, 16]
            assert [layer.scope for layer in model.layers] == ["l1", "l2", "l3", "l4"]
            assert callable(model.get_end_points) and callable(model.body)
    import pn2hip
    assert pn2hip.attention_models is pn2.attention_models
    assert pn2hip.pooling_attention_model.PoolingAttentionNetModel is \
        pn2.pooling_attention_model.PoolingAttentionNetModel


def test_layers_refuse_what_the_kernels_do_not_run(pn2):
    A = pn2.attention_layer
    with pytest.raises(NotImplementedError, match="output_dim == key_dim"):
        A.AttentionLayer(8, 4)
    with pytest.raises(NotImplementedError):
        A.AttentionLayer(6, 6)
    with pytest.raises(NotImplementedError):
        A.AttentionNetLayer(npoint=16, out_dim=6, inner_dimensions=[8])
    with pytest.raises(NotImplementedError):
        A.FeedForwardLayer(8, 8, dropout=0.5)
    z = torch.zeros
    with pytest.raises(ValueError):
        A.attention_reduce(z(1, 2, 24), z(1, 2, 3, 24), z(1, 2, 3, 24), key_dim=16)
    with pytest.raises(RuntimeError, match="MI355X only"):   # the default call is today's
        A.attention_reduce(z(1, 2, 24), z(1, 2, 3, 24), z(1, 2, 3, 24))
    with pytest.raises(RuntimeError, match="MI355X only"):
        A.attention_reduce(z(1, 2, 24), z(1, 2, 3, 24), z(1, 2, 3, 24), key_dim=8)


def test_plan_accepts_names_the_layers_that_fall_back(pn2):
    """The widths DESIGN.md lists: the attention networks' Dense chains run fused; the pooling
    model's 2051- and 4099-wide inputs and the wide feature-propagation inputs do not."""
    ok = pn2.attention_layer.plan_accepts
    for c in (8, 16, 32, 64):
        assert ok(c, (c,) * 4) and ok(c, (15 * c,)) and ok(5 * c, (c,)) and ok(c, (16 * c,))
    assert ok(1027, (64, 64, 128)) and ok(512, (8192,)) and ok(131, (16, 16, 16, 16))
    for cin, widths in ((2051, (128, 128, 256)), (4099, (256, 256, 512)), (12288, (256, 256)),
                        (2304, (256, 256)), (1280, (256, 128)), (1536, (256, 256)), (8192, (512,))):
        assert not ok(cin, widths), (cin, widths)
    assert not ok(8, (8,) * 7)   # longer than one fused chain
