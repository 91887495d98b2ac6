"""CPU: the training MLP's last layer fused with the max pool over nsample (csrc/mlp_train.hip,
torch.ops.pn2.mlp_layer_train_pool / mlp_layer_train_pool_grad): schemas, Meta shapes, no CPU
kernel, and the argument checks of the C entry points, which return PN2_EINVAL before any
launch. No kernel runs here; tests/test_gpu_mlp_train_pool.py runs them on the MI355X."""
import pytest
import torch

E = -22
POOL_GROUPS = 128  # PN2_BN_POOL_BLOCK_GROUPS (include/pn2hip.h)


@pytest.fixture(scope="module")
def ops():
    import pn2hip
    return pn2hip.ops


def test_schemas(ops):
    assert str(ops.mlp_layer_train_pool._schemas[""]) == (
        "pn2::mlp_layer_train_pool(Tensor x, Tensor weight, Tensor? bias, Tensor? gamma, "
        "Tensor? beta, float eps, bool relu) -> (Tensor out, Tensor y, Tensor mean, Tensor var, "
        "Tensor arg)")
    assert str(ops.mlp_layer_train_pool_grad._schemas[""]) == (
        "pn2::mlp_layer_train_pool_grad(Tensor grad_out, Tensor arg, Tensor x, Tensor weight, "
        "Tensor y, Tensor? mean, Tensor? var, Tensor? gamma, Tensor? beta, float eps, bool relu, "
        "bool need_grad_x) -> (Tensor grad_x, Tensor grad_w, Tensor grad_b, Tensor grad_gamma, "
        "Tensor grad_beta)")
    for name in ("mlp_layer_train_pool", "mlp_layer_train_pool_grad"):
        assert name in ops.NAMES
        has = lambda key: torch._C._dispatch_has_kernel_for_dispatch_key(f"pn2::{name}", key)  # noqa: E731
        assert has("CUDA") and has("Meta") and not has("CPU")
    assert torch._C._dispatch_has_kernel_for_dispatch_key("pn2::mlp_layer_train_pool", "Autograd")


def test_header_constant():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "pn2hip.h")).read()
    assert int(re.search(r"#define PN2_BN_POOL_BLOCK_GROUPS (\d+)", text).group(1)) == POOL_GROUPS


def test_meta_shapes(ops):
    m = lambda *s, dt=torch.float32: torch.empty(s, device="meta", dtype=dt)  # noqa: E731
    x, w = m(2, 64, 16, 9), m(9, 32)
    out, y, mean, var, arg = ops.mlp_layer_train_pool(x, w, m(32), m(32), m(32), 1e-3, True)
    assert out.shape == arg.shape == (2, 64, 32) and y.shape == (2, 64, 16, 32)
    assert out.dtype == y.dtype == torch.float32 and arg.dtype == torch.int32
    assert mean.shape == var.shape == (32,)
    gx, gw, gb, gg, gbeta = ops.mlp_layer_train_pool_grad(out, arg, x, w, y, mean, var, m(32),
                                                          m(32), 1e-3, True, True)
    assert gx.shape == x.shape and gw.shape == (9, 32)
    assert gb.shape == gg.shape == gbeta.shape == (32,)
    # no batch norm: mean and var are (0,), and so are their gradients' slots
    out, y, mean, var, arg = ops.mlp_layer_train_pool(x, w, m(32), None, None, 1e-3, False)
    assert out.shape == arg.shape == (2, 64, 32) and mean.shape == var.shape == (0,)
    for mv in ((mean, var), (None, None)):
        gx, gw, gb, gg, gbeta = ops.mlp_layer_train_pool_grad(out, arg, x, w, y, mv[0], mv[1],
                                                              None, None, 1e-3, True, False)
        assert gx.shape == (0,) and gw.shape == (9, 32) and gb.shape == (32,)
        assert gg.shape == gbeta.shape == (0,)
    # the smallest input: (ns, cin), one group
    out, y, _, _, arg = ops.mlp_layer_train_pool(m(7, 9), w, None, None, None, 1e-3, True)
    assert out.shape == arg.shape == (32,) and y.shape == (7, 32)
    # no groups
    out, y, _, _, arg = ops.mlp_layer_train_pool(m(0, 7, 9), w, None, None, None, 1e-3, True)
    assert out.shape == arg.shape == (0, 32) and y.shape == (0, 7, 32)


@pytest.mark.parametrize("bn", [True, False])
def test_autograd_on_meta_tensors(ops, bn):
    """The registered autograd runs end to end on fake tensors: y, mean, var and arg carry no
    gradient, every differentiable input gets one of its own shape, absent inputs none."""
    m = lambda *s: torch.empty(s, device="meta", requires_grad=True)  # noqa: E731
    x, w, b = m(2, 10, 5, 9), m(9, 32), m(32)
    gamma, beta = (m(32), m(32)) if bn else (None, None)
    out, y, mean, var, arg = ops.mlp_layer_train_pool(x, w, b, gamma, beta, 1e-3, True)
    assert out.requires_grad and out.shape == (2, 10, 32)
    assert not (y.requires_grad or mean.requires_grad or var.requires_grad or arg.requires_grad)
    out.sum().backward()
    for t in (x, w, b) + ((gamma, beta) if bn else ()):
        assert t.grad is not None and t.grad.shape == t.shape
    # no bias, and an input that needs no gradient
    w.grad = None
    ops.mlp_layer_train_pool(x.detach(), w, None, gamma, beta, 1e-3, False)[0].sum().backward()
    assert w.grad.shape == w.shape


@pytest.mark.parametrize("call", [
    lambda o, m: o.mlp_layer_train_pool(m(10, 4, 8), m(9, 32), None, None, None, 1e-3, True),   # cin
    lambda o, m: o.mlp_layer_train_pool(m(10, 4, 9), m(9, 32), None, m(32), None, 1e-3, True),  # no beta
    lambda o, m: o.mlp_layer_train_pool(m(9), m(9, 32), None, None, None, 1e-3, True),          # 1-D x
    lambda o, m: o.mlp_layer_train_pool(m(10, 0, 9), m(9, 32), None, None, None, 1e-3, True),   # ns = 0
    lambda o, m: o.mlp_layer_train_pool(m(10, 4, 9), m(9, 32), m(31), None, None, 1e-3, True),  # bias
    # the gradient op: grad_out / arg not (..., cout), y not (..., ns, cout), gamma without mean
    lambda o, m: o.mlp_layer_train_pool_grad(m(10, 4, 32), m(10, 32), m(10, 4, 9), m(9, 32),
                                             m(10, 4, 32), None, None, None, None, 1e-3, True, True),
    lambda o, m: o.mlp_layer_train_pool_grad(m(10, 32), m(10, 31), m(10, 4, 9), m(9, 32),
                                             m(10, 4, 32), None, None, None, None, 1e-3, True, True),
    lambda o, m: o.mlp_layer_train_pool_grad(m(10, 32), m(10, 32), m(10, 4, 9), m(9, 32),
                                             m(10, 5, 32), None, None, None, None, 1e-3, True, True),
    lambda o, m: o.mlp_layer_train_pool_grad(m(10, 32), m(10, 32), m(10, 4, 9), m(9, 32),
                                             m(10, 4, 32), None, None, m(32), m(32), 1e-3, True, True),
])
def test_shape_errors(ops, call):
    m = lambda *s: torch.empty(s, device="meta")  # noqa: E731
    with pytest.raises(ValueError):
        call(ops, m)


def test_no_cpu_kernel(ops):
    z = torch.zeros
    with pytest.raises(NotImplementedError):
        ops.mlp_layer_train_pool(z(10, 4, 9), z(9, 32), None, None, None, 1e-3, True)
    with pytest.raises(NotImplementedError):
        ops.mlp_layer_train_pool_grad(z(10, 32), z(10, 32, dtype=torch.int32), z(10, 4, 9),
                                      z(9, 32), z(10, 4, 32), None, None, None, None, 1e-3, True,
                                      True)


def test_pool_entry_points_check_arguments_without_launching(pn2):
    lib = pn2.lib()
    fake = 1 << 20  # never dereferenced by the checks
    # two floats (sum dz, sum dz * xhat) per channel and block of PN2_BN_POOL_BLOCK_GROUPS groups
    assert lib.pn2_bn_pool_workspace_size(POOL_GROUPS, 32) == 2 * 32 * 4
    assert lib.pn2_bn_pool_workspace_size(POOL_GROUPS + 1, 33) == 2 * 2 * 33 * 4
    assert lib.pn2_bn_pool_workspace_size(1, 1) == 2 * 4
    for groups, C in ((0, 32), (-3, 32), (10, 0), (10, -1), (0, 0)):
        assert lib.pn2_bn_pool_workspace_size(groups, C) == 0, (groups, C)

    ok = (fake, 100, 16, 32, fake, fake, fake, fake, 1e-3, 1, fake, fake, None)

    def fwd(**kw):
        names = ("y", "groups", "ns", "C", "mean", "var", "gamma", "beta", "eps", "relu", "out",
                 "arg", "stream")
        args = dict(zip(names, ok))
        args.update(kw)
        return lib.pn2_bn_act_pool_fwd(*[args[n] for n in names])

    for name in ("y", "out", "arg"):
        assert fwd(**{name: None}) == E, name
    for kw in (dict(groups=0), dict(groups=-5), dict(ns=0), dict(ns=-1), dict(C=0), dict(C=-2)):
        assert fwd(**kw) == E, kw
    assert fwd(groups=1 << 27, ns=16) == E              # groups * ns = 2^31 > 0x7fffffff
    assert fwd(groups=1 << 31, ns=1) == E
    assert fwd(groups=1 << 62, ns=4) == E               # a product that overflows 64 bits
    for missing in ("mean", "var", "gamma", "beta"):   # the four together or none
        assert fwd(**{missing: None}) == E, missing
    assert fwd(mean=None, gamma=None) == E
    assert fwd(eps=-1.0) == E

    ws = lib.pn2_bn_pool_workspace_size(100, 32)
    okb = (fake, fake, fake, 100, 16, 32, fake, fake, fake, fake, 1e-3, 1, fake, fake, fake, fake,
           ws, None)

    def bwd(**kw):
        names = ("grad_out", "arg", "y", "groups", "ns", "C", "mean", "var", "gamma", "beta", "eps",
                 "relu", "grad_y", "grad_gamma", "grad_beta", "ws", "ws_bytes", "stream")
        args = dict(zip(names, okb))
        args.update(kw)
        return lib.pn2_bn_act_pool_bwd(*[args[n] for n in names])

    for name in ("grad_out", "arg", "y", "grad_y", "grad_beta", "ws"):
        assert bwd(**{name: None}) == E, name
    for kw in (dict(groups=0), dict(groups=-5), dict(ns=0), dict(ns=-1), dict(C=0), dict(C=-2)):
        assert bwd(**kw) == E, kw
    assert bwd(groups=1 << 27, ns=16, ws_bytes=1 << 40) == E
    assert bwd(groups=1 << 31, ns=1, ws_bytes=1 << 40) == E
    assert bwd(ws_bytes=ws - 1) == E
    for missing in ("mean", "var", "gamma", "beta"):
        assert bwd(**{missing: None}) == E, missing
    assert bwd(grad_gamma=None) == E                    # batch norm without its gamma gradient
    assert bwd(mean=None, var=None, gamma=None, beta=None) == E  # grad_gamma without batch norm
    assert bwd(eps=-1.0) == E


def test_mlp_train_rejects_other_pooling(pn2):
    tu = pn2.tf_util
    store = tu.ParamStore(seed=1)
    layers = tu.torch_layers(store, ["a/conv0"], 9, [32])
    for pool in ("avg", "weighted_avg", "max_and_avg", "MAX", True):
        with pytest.raises(pn2.InvalidArgumentError):
            tu.mlp_train(torch.zeros(2, 4, 8, 9), layers, None, pool=pool)
    with pytest.raises(pn2.InvalidArgumentError):
        tu.mlp_train(torch.zeros(2, 4, 8, 9), [], None, pool="max")
