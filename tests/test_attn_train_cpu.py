"""CPU: the training-mode attention layer (csrc/attn_train.hip, torch.ops.pn2.attn_kv_train /
attn_kv_train_grad) and the stand-alone batch-statistics batch norm (bn_train / bn_train_grad):
schemas, Meta shapes, no CPU kernel, the exported entry points and their argument checks, which
return PN2_EINVAL before any launch. No kernel runs here; tests/test_gpu_attn_train.py runs them
on the MI355X."""
import os
import re
import subprocess

import pytest
import torch

E = -22
NEW_ENTRY_POINTS = ("pn2_attn_kv_reduce", "pn2_attn_kv_reduce_grad", "pn2_attn_dx_scatter",
                    "pn2_col_sum_workspace_size", "pn2_col_sum")
NEW_OPS = ("attn_kv_train", "attn_kv_train_grad", "bn_train", "bn_train_grad")


@pytest.fixture(scope="module")
def ops():
    import pn2hip
    return pn2hip.ops


def test_schemas(ops):
    assert str(ops.attn_kv_train._schemas[""]) == (
        "pn2::attn_kv_train(Tensor x, Tensor wq, Tensor bq, Tensor wk, Tensor bk, Tensor wv, "
        "Tensor bv, bool add_max) -> (Tensor att, Tensor pmax, Tensor arg, Tensor q, Tensor kv)")
    assert str(ops.attn_kv_train_grad._schemas[""]) == (
        "pn2::attn_kv_train_grad(Tensor grad_att, Tensor? grad_pmax, Tensor arg, Tensor x, "
        "Tensor wq, Tensor wk, Tensor wv, Tensor q, Tensor kv, bool need_grad_x) -> "
        "(Tensor grad_x, Tensor grad_wq, Tensor grad_bq, Tensor grad_wk, Tensor grad_bk, "
        "Tensor grad_wv, Tensor grad_bv)")
    assert str(ops.bn_train._schemas[""]) == (
        "pn2::bn_train(Tensor x, Tensor gamma, Tensor beta, float eps, bool relu) -> "
        "(Tensor out, Tensor mean, Tensor var)")
    assert str(ops.bn_train_grad._schemas[""]) == (
        "pn2::bn_train_grad(Tensor grad_out, Tensor x, Tensor mean, Tensor var, Tensor gamma, "
        "Tensor beta, float eps, bool relu) -> (Tensor grad_x, Tensor grad_gamma, "
        "Tensor grad_beta)")
    for name in NEW_OPS:
        assert name in ops.NAMES
        has = lambda key: torch._C._dispatch_has_kernel_for_dispatch_key(f"pn2::{name}", key)  # noqa: E731
        assert has("CUDA") and has("Meta") and not has("CPU")
    for name in ("attn_kv_train", "bn_train"):
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f"pn2::{name}", "Autograd")


def test_meta_shapes(ops):
    m = lambda *s, dt=torch.float32: torch.empty(s, device="meta", dtype=dt)  # noqa: E731
    x, w, b = m(2, 64, 16, 32), m(32, 32), m(32)
    att, pmax, arg, q, kv = ops.attn_kv_train(x, w, b, w, b, w, b, True)
    assert att.shape == pmax.shape == arg.shape == q.shape == (2, 64, 32)
    assert kv.shape == (2, 64, 16, 64)
    assert att.dtype == pmax.dtype == q.dtype == kv.dtype == torch.float32
    assert arg.dtype == torch.int32
    grads = ops.attn_kv_train_grad(att, pmax, arg, x, w, w, w, q, kv, True)
    assert len(grads) == 7 and grads[0].shape == x.shape
    assert [tuple(g.shape) for g in grads[1:]] == [(32, 32), (32,)] * 3
    # without the pool: 0-element pmax and arg, and no grad_pmax
    att, pmax, arg, q, kv = ops.attn_kv_train(x, w, b, w, b, w, b, False)
    assert att.shape == (2, 64, 32) and pmax.shape == arg.shape == (0,)
    assert pmax.dtype == torch.float32 and arg.dtype == torch.int32
    grads = ops.attn_kv_train_grad(att, None, arg, x, w, w, w, q, kv, False)
    assert grads[0].shape == (0,) and grads[1].shape == (32, 32)
    # the smallest input: one group of one row; no groups
    att, pmax, arg, q, kv = ops.attn_kv_train(m(1, 4), m(4, 4), m(4), m(4, 4), m(4), m(4, 4),
                                              m(4), True)
    assert att.shape == pmax.shape == arg.shape == q.shape == (4,) and kv.shape == (1, 8)
    att, _, _, _, kv = ops.attn_kv_train(m(0, 5, 8), m(8, 8), m(8), m(8, 8), m(8), m(8, 8), m(8),
                                         False)
    assert att.shape == (0, 8) and kv.shape == (0, 5, 16)

    out, mean, var = ops.bn_train(m(3, 7, 33), m(33), m(33), 1e-3, False)
    assert out.shape == (3, 7, 33) and mean.shape == var.shape == (33,)
    gx, gg, gb = ops.bn_train_grad(out, m(3, 7, 33), mean, var, m(33), m(33), 1e-3, False)
    assert gx.shape == (3, 7, 33) and gg.shape == gb.shape == (33,)
    out, mean, var = ops.bn_train(m(4), m(4), m(4), 1e-3, True)
    assert out.shape == mean.shape == (4,)


@pytest.mark.parametrize("add_max", [True, False])
def test_autograd_on_meta_tensors(ops, add_max):
    """The registered autograd runs end to end on fake tensors: arg, q and kv carry no gradient,
    x and the six variables get one of their own shape."""
    m = lambda *s: torch.empty(s, device="meta", requires_grad=True)  # noqa: E731
    x = m(2, 10, 5, 8)
    ws = [m(8, 8), m(8), m(8, 8), m(8), m(8, 8), m(8)]
    att, pmax, arg, q, kv = ops.attn_kv_train(x, *ws, add_max)
    assert att.requires_grad and not (arg.requires_grad or q.requires_grad or kv.requires_grad)
    gamma, beta = m(8), m(8)
    out, mean, var = ops.bn_train(att, gamma, beta, 1e-3, False)
    assert out.requires_grad and not (mean.requires_grad or var.requires_grad)
    (out + pmax if add_max else out).sum().backward()
    for t in [x, gamma, beta] + ws:
        assert t.grad is not None and t.grad.shape == t.shape
    # an input that needs no gradient
    ws[0].grad = None
    ops.attn_kv_train(x.detach(), *ws, add_max)[0].sum().backward()
    assert ws[0].grad.shape == (8, 8)


@pytest.mark.parametrize("call", [
    lambda o, m: o.attn_kv_train(m(3, 5, 6), m(6, 6), m(6), m(6, 6), m(6), m(6, 6), m(6), True),  # C % 4
    lambda o, m: o.attn_kv_train(m(8), m(8, 8), m(8), m(8, 8), m(8), m(8, 8), m(8), True),        # 1-D x
    lambda o, m: o.attn_kv_train(m(3, 0, 8), m(8, 8), m(8), m(8, 8), m(8), m(8, 8), m(8), True),  # ns = 0
    lambda o, m: o.attn_kv_train(m(3, 5, 8), m(8, 8), m(8), m(8, 4), m(8), m(8, 8), m(8), True),  # wk
    lambda o, m: o.attn_kv_train(m(3, 5, 8), m(8, 8), m(8), m(8, 8), m(8), m(8, 8), m(7), True),  # bv
    # the gradient op: grad_att not (..., C), kv not (..., ns, 2C), grad_pmax / arg not (..., C)
    lambda o, m: o.attn_kv_train_grad(m(3, 5, 8), None, m(0), m(3, 5, 8), m(8, 8), m(8, 8),
                                      m(8, 8), m(3, 8), m(3, 5, 16), True),
    lambda o, m: o.attn_kv_train_grad(m(3, 8), None, m(0), m(3, 5, 8), m(8, 8), m(8, 8),
                                      m(8, 8), m(3, 8), m(3, 5, 8), True),
    lambda o, m: o.attn_kv_train_grad(m(3, 8), m(3, 8), m(3, 7), m(3, 5, 8), m(8, 8), m(8, 8),
                                      m(8, 8), m(3, 8), m(3, 5, 16), True),
    lambda o, m: o.bn_train(m(3, 8), m(7), m(8), 1e-3, False),
    lambda o, m: o.bn_train_grad(m(3, 7), m(3, 8), m(8), m(8), m(8), m(8), 1e-3, False),
    lambda o, m: o.bn_train_grad(m(3, 8), m(3, 8), m(7), m(8), m(8), m(8), 1e-3, False),
])
def test_shape_errors(ops, call):
    m = lambda *s: torch.empty(s, device="meta")  # noqa: E731
    with pytest.raises(ValueError):
        call(ops, m)


def test_no_cpu_kernel(ops):
    z = torch.zeros
    with pytest.raises(NotImplementedError):
        ops.attn_kv_train(z(3, 5, 8), z(8, 8), z(8), z(8, 8), z(8), z(8, 8), z(8), True)
    with pytest.raises(NotImplementedError):
        ops.attn_kv_train_grad(z(3, 8), None, z(0, dtype=torch.int32), z(3, 5, 8), z(8, 8),
                               z(8, 8), z(8, 8), z(3, 8), z(3, 5, 16), True)
    with pytest.raises(NotImplementedError):
        ops.bn_train(z(3, 8), z(8), z(8), 1e-3, False)
    with pytest.raises(NotImplementedError):
        ops.bn_train_grad(z(3, 8), z(3, 8), z(8), z(8), z(8), z(8), 1e-3, False)


def test_mirror_refuses_cpu_tensors(pn2):
    """The public interfaces name the device, as every other mirror function does."""
    store = pn2.tf_util.ParamStore(seed=1)
    with pytest.raises(RuntimeError, match="MI355X only"):
        pn2.tf_util.bn_train(torch.zeros(3, 8), store.bn("a/a", 8))
    with pytest.raises(RuntimeError, match="MI355X only"):
        pn2.attention_layer.attention_train(torch.zeros(2, 3, 5, 8), store, "a", 8)


def test_entry_points_are_declared_exported_and_bound(pn2):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "pn2hip.h")).read(),
                  flags=re.S)
    exported = subprocess.run(["nm", "-D", "--defined-only", pn2.LIB_PATH], capture_output=True,
                              text=True, check=True).stdout
    _lib = __import__("importlib").import_module(pn2.__name__ + "._lib")
    for name in NEW_ENTRY_POINTS:
        assert re.search(rf"\b{name}\s*\(", text), f"{name} not declared in pn2hip.h"
        assert re.search(rf"\bT {name}$", exported, re.M), f"{name} not exported"
        assert name in _lib.SIGNATURES
        assert getattr(pn2.lib(), name) is not None


def test_reduction_entry_points_check_arguments_without_launching(pn2):
    lib = pn2.lib()
    fake = 1 << 20  # 16-byte aligned, never dereferenced by the checks

    def fwd(**kw):
        names = ("Q", "KV", "G", "ns", "C", "out", "stream")
        args = dict(zip(names, (fake, fake, 10, 32, 64, fake, None)))
        args.update(kw)
        return lib.pn2_attn_kv_reduce(*[args[n] for n in names])

    def bwd(**kw):
        names = ("Q", "KV", "grad_out", "G", "ns", "C", "grad_Q", "grad_KV", "stream")
        args = dict(zip(names, (fake, fake, fake, 10, 32, 64, fake, fake, None)))
        args.update(kw)
        return lib.pn2_attn_kv_reduce_grad(*[args[n] for n in names])

    for fn, bufs in ((fwd, ("Q", "KV", "out")),
                     (bwd, ("Q", "KV", "grad_out", "grad_Q", "grad_KV"))):
        for name in bufs:
            assert fn(**{name: None}) == E, name            # null
            assert fn(**{name: fake + 4}) == E, name        # not 16-byte aligned
            assert fn(**{name: fake + 8}) == E, name
        for kw in (dict(C=6), dict(C=62), dict(C=-4), dict(ns=0), dict(ns=-1), dict(G=-1)):
            assert fn(**kw) == E, kw
        assert fn(G=1 << 31) == E                           # groups are indexed in 31 bits
        assert fn(ns=1 << 20, C=1 << 10) == E               # ns * C >= 2^30: 32-bit row offsets
        # no groups: a no-op that returns 0, whatever the buffers
        assert fn(G=0) == 0
        assert fn(G=0, **{n: None for n in bufs}) == 0
        assert fn(G=0, C=6) == E                            # the shape is checked first


def test_helper_entry_points_check_arguments_without_launching(pn2):
    lib = pn2.lib()
    fake = 1 << 20

    def scatter(**kw):
        names = ("grad_x", "grad_xq", "grad_pmax", "arg", "G", "ns", "C", "stream")
        args = dict(zip(names, (fake, fake, fake, fake, 10, 32, 64, None)))
        args.update(kw)
        return lib.pn2_attn_dx_scatter(*[args[n] for n in names])

    for name in ("grad_x", "grad_xq"):
        assert scatter(**{name: None}) == E, name
    assert scatter(grad_pmax=None) == E and scatter(arg=None) == E   # NULL together only
    for kw in (dict(ns=0), dict(ns=-3), dict(G=-1), dict(C=-1)):
        assert scatter(**kw) == E, kw
    assert scatter(G=1 << 31) == E and scatter(G=1 << 27, ns=16) == E  # G * ns > 2^31 - 1
    assert scatter(G=0) == 0
    assert scatter(G=0, grad_x=None, grad_xq=None, grad_pmax=None, arg=None) == 0

    # one fp32 partial per channel and block of PN2_BN_BLOCK_ROWS (1024) rows
    assert lib.pn2_col_sum_workspace_size(1024, 32) == 32 * 4
    assert lib.pn2_col_sum_workspace_size(1025, 33) == 2 * 33 * 4
    assert lib.pn2_col_sum_workspace_size(1, 1) == 4
    for rows, C in ((0, 32), (-3, 32), (10, 0), (10, -1)):
        assert lib.pn2_col_sum_workspace_size(rows, C) == 0, (rows, C)
    ws = lib.pn2_col_sum_workspace_size(5000, 64)

    def col_sum(**kw):
        names = ("x", "rows", "C", "out", "ws", "ws_bytes", "stream")
        args = dict(zip(names, (fake, 5000, 64, fake, fake, ws, None)))
        args.update(kw)
        return lib.pn2_col_sum(*[args[n] for n in names])

    for name in ("x", "out", "ws"):
        assert col_sum(**{name: None}) == E, name
    for kw in (dict(rows=0), dict(rows=-1), dict(C=0), dict(C=-2), dict(rows=1 << 31, ws_bytes=1 << 40),
               dict(ws_bytes=ws - 1)):
        assert col_sum(**kw) == E, kw
