"""CPU: the training-mode shared-MLP layer (csrc/mlp_train.hip, torch.ops.pn2.mlp_layer_train /
mlp_layer_train_grad): schemas, Meta shapes, no CPU kernel, and the argument checks of the C
entry points, which return PN2_EINVAL before any launch. No kernel runs here;
tests/test_gpu_mlp_train.py runs them on the MI355X."""
import pytest
import torch

E = -22


@pytest.fixture(scope="module")
def ops():
    import pn2hip
    return pn2hip.ops


def test_schemas(ops):
    assert str(ops.mlp_layer_train._schemas[""]) == (
        "pn2::mlp_layer_train(Tensor x, Tensor weight, Tensor? bias, Tensor? gamma, Tensor? beta, "
        "float eps, bool relu) -> (Tensor out, Tensor y, Tensor mean, Tensor var)")
    assert str(ops.mlp_layer_train_grad._schemas[""]) == (
        "pn2::mlp_layer_train_grad(Tensor grad_out, Tensor x, Tensor weight, Tensor y, "
        "Tensor? mean, Tensor? var, Tensor? gamma, Tensor? beta, float eps, bool relu, "
        "bool need_grad_x) -> (Tensor grad_x, Tensor grad_w, Tensor grad_b, Tensor grad_gamma, "
        "Tensor grad_beta)")
    for name in ("mlp_layer_train", "mlp_layer_train_grad"):
        assert name in ops.NAMES
        has = lambda key: torch._C._dispatch_has_kernel_for_dispatch_key(f"pn2::{name}", key)  # noqa: E731
        assert has("CUDA") and has("Meta") and not has("CPU")
    assert torch._C._dispatch_has_kernel_for_dispatch_key("pn2::mlp_layer_train", "Autograd")


def test_meta_shapes(ops):
    m = lambda *s: torch.empty(s, device="meta")  # noqa: E731
    x, w = m(2, 64, 16, 9), m(9, 32)
    out, y, mean, var = ops.mlp_layer_train(x, w, m(32), m(32), m(32), 1e-3, True)
    assert out.shape == y.shape == (2, 64, 16, 32)
    assert mean.shape == var.shape == (32,)
    out, y, mean, var = ops.mlp_layer_train(x, w, m(32), None, None, 1e-3, False)
    assert out.shape == (2, 64, 16, 32) and mean.shape == var.shape == (0,)
    gx, gw, gb, gg, gbeta = ops.mlp_layer_train_grad(out, x, w, y, m(32), m(32), m(32), m(32),
                                                     1e-3, True, True)
    assert gx.shape == x.shape and gw.shape == (9, 32)
    assert gb.shape == gg.shape == gbeta.shape == (32,)
    gx, gw, gb, gg, gbeta = ops.mlp_layer_train_grad(out, x, w, y, None, None, None, None, 1e-3,
                                                     True, False)
    assert gx.shape == (0,) and gw.shape == (9, 32) and gb.shape == (32,)
    assert gg.shape == gbeta.shape == (0,)


@pytest.mark.parametrize("bn", [True, False])
def test_autograd_on_meta_tensors(ops, bn):
    """The registered autograd runs end to end on fake tensors: y, mean and var carry no
    gradient, every differentiable input gets one of its own shape, absent inputs none."""
    m = lambda *s: torch.empty(s, device="meta", requires_grad=True)  # noqa: E731
    x, w, b = m(2, 10, 9), m(9, 32), m(32)
    gamma, beta = (m(32), m(32)) if bn else (None, None)
    out, y, mean, var = ops.mlp_layer_train(x, w, b, gamma, beta, 1e-3, True)
    assert out.requires_grad and not (y.requires_grad or mean.requires_grad or var.requires_grad)
    out.sum().backward()
    for t in (x, w, b) + ((gamma, beta) if bn else ()):
        assert t.grad is not None and t.grad.shape == t.shape
    # no bias, and an input that needs no gradient
    w.grad = None
    ops.mlp_layer_train(x.detach(), w, None, gamma, beta, 1e-3, False)[0].sum().backward()
    assert w.grad.shape == w.shape


@pytest.mark.parametrize("call", [
    lambda o, m: o.mlp_layer_train(m(10, 8), m(9, 32), None, None, None, 1e-3, True),   # cin
    lambda o, m: o.mlp_layer_train(m(10, 9), m(9, 32), m(31), None, None, 1e-3, True),  # bias
    lambda o, m: o.mlp_layer_train(m(10, 9), m(9, 32), None, m(32), None, 1e-3, True),  # no beta
    lambda o, m: o.mlp_layer_train(m(10, 9), m(1, 1, 9, 32), None, None, None, 1e-3, True),
])
def test_shape_errors(ops, call):
    m = lambda *s: torch.empty(s, device="meta")  # noqa: E731
    with pytest.raises(ValueError):
        call(ops, m)


def test_no_cpu_kernel(ops):
    with pytest.raises(NotImplementedError):
        ops.mlp_layer_train(torch.zeros(10, 9), torch.zeros(9, 32), None, None, None, 1e-3, True)
    with pytest.raises(NotImplementedError):
        ops.mlp_layer_train_grad(torch.zeros(10, 32), torch.zeros(10, 9), torch.zeros(9, 32),
                                 torch.zeros(10, 32), None, None, None, None, 1e-3, True, True)


def test_bn_entry_points_check_arguments_without_launching(pn2):
    lib = pn2.lib()
    fake = 1 << 20  # never dereferenced by the checks
    # two (mean, M2) floats per channel and block of PN2_BN_BLOCK_ROWS = 1024 rows
    assert lib.pn2_bn_workspace_size(1024, 32) == 2 * 32 * 4
    assert lib.pn2_bn_workspace_size(1025, 33) == 2 * 2 * 33 * 4
    assert lib.pn2_bn_workspace_size(0, 32) == 0 and lib.pn2_bn_workspace_size(10, 0) == 0
    ws = lib.pn2_bn_workspace_size(100, 32)
    assert lib.pn2_bn_stats(None, 100, 32, fake, fake, fake, ws, None) == E       # y
    assert lib.pn2_bn_stats(fake, 100, 32, None, fake, fake, ws, None) == E       # mean
    assert lib.pn2_bn_stats(fake, 100, 32, fake, None, fake, ws, None) == E       # var
    assert lib.pn2_bn_stats(fake, 100, 32, fake, fake, None, ws, None) == E       # workspace
    assert lib.pn2_bn_stats(fake, 100, 32, fake, fake, fake, ws - 1, None) == E   # too small
    assert lib.pn2_bn_stats(fake, 0, 32, fake, fake, fake, ws, None) == E         # rows
    assert lib.pn2_bn_stats(fake, -5, 32, fake, fake, fake, ws, None) == E
    assert lib.pn2_bn_stats(fake, 100, 0, fake, fake, fake, ws, None) == E        # C
    assert lib.pn2_bn_stats(fake, 1 << 31, 32, fake, fake, fake, 1 << 40, None) == E  # rows cap

    assert lib.pn2_bn_act_fwd(None, 100, 32, fake, fake, fake, fake, 1e-3, 1, fake, None) == E
    assert lib.pn2_bn_act_fwd(fake, 100, 32, fake, fake, fake, fake, 1e-3, 1, None, None) == E
    assert lib.pn2_bn_act_fwd(fake, 0, 32, fake, fake, fake, fake, 1e-3, 1, fake, None) == E
    assert lib.pn2_bn_act_fwd(fake, 100, -1, fake, fake, fake, fake, 1e-3, 1, fake, None) == E
    # mean, var, gamma, beta: all four or none
    assert lib.pn2_bn_act_fwd(fake, 100, 32, fake, fake, fake, None, 1e-3, 1, fake, None) == E
    assert lib.pn2_bn_act_fwd(fake, 100, 32, None, fake, None, None, 1e-3, 1, fake, None) == E
    assert lib.pn2_bn_act_fwd(fake, 100, 32, fake, fake, fake, fake, -1.0, 1, fake, None) == E

    ok = (fake, fake, 100, 32, fake, fake, fake, fake, 1e-3, 1, fake, fake, fake, fake, ws, None)

    def bwd(**kw):
        names = ("grad_out", "y", "rows", "C", "mean", "var", "gamma", "beta", "eps", "relu",
                 "grad_y", "grad_gamma", "grad_beta", "ws", "ws_bytes", "stream")
        args = dict(zip(names, ok))
        args.update(kw)
        return lib.pn2_bn_act_bwd(*[args[n] for n in names])

    for name in ("grad_out", "y", "grad_y", "grad_beta", "ws"):
        assert bwd(**{name: None}) == E, name
    assert bwd(rows=0) == E and bwd(C=0) == E
    assert bwd(ws_bytes=ws - 1) == E
    assert bwd(beta=None) == E                          # three of the four
    assert bwd(grad_gamma=None) == E                    # batch norm without its gamma gradient
    assert bwd(mean=None, var=None, gamma=None, beta=None) == E  # grad_gamma without batch norm


def test_wgrad_entry_point_checks_arguments_without_launching(pn2):
    lib = pn2.lib()
    fake = 1 << 20
    tile = 32 * 32 * 4
    # one partial tile per 1024-row slab and 32x32 output tile ...
    assert lib.pn2_mlp_wgrad_workspace_size(1000, 3, 32) == tile
    assert lib.pn2_mlp_wgrad_workspace_size(1025, 33, 64) == 2 * (2 * 2) * tile
    # ... at most 512 parts, and no more than 64 MiB
    assert lib.pn2_mlp_wgrad_workspace_size(1 << 20, 32, 32) == 512 * tile
    big = lib.pn2_mlp_wgrad_workspace_size(1 << 20, 1030, 1024)
    assert 0 < big <= 64 << 20 and big % (33 * 32 * tile) == 0
    assert lib.pn2_mlp_wgrad_workspace_size(0, 3, 32) == 0
    ws = lib.pn2_mlp_wgrad_workspace_size(100, 9, 32)
    assert lib.pn2_mlp_wgrad(None, fake, 100, 9, 32, fake, fake, ws, None) == E
    assert lib.pn2_mlp_wgrad(fake, None, 100, 9, 32, fake, fake, ws, None) == E
    assert lib.pn2_mlp_wgrad(fake, fake, 100, 9, 32, None, fake, ws, None) == E
    assert lib.pn2_mlp_wgrad(fake, fake, 100, 9, 32, fake, None, ws, None) == E
    assert lib.pn2_mlp_wgrad(fake, fake, 100, 9, 32, fake, fake, ws - 1, None) == E
    assert lib.pn2_mlp_wgrad(fake, fake, 0, 9, 32, fake, fake, ws, None) == E
    assert lib.pn2_mlp_wgrad(fake, fake, 100, 0, 32, fake, fake, ws, None) == E
    assert lib.pn2_mlp_wgrad(fake, fake, 100, 9, -3, fake, fake, ws, None) == E


def test_trainable_store_on_cpu(pn2):
    """ParamStore.trainable(): leaves with gradients for the variables, plain tensors for the
    moving statistics, for existing and later variables; parameters() and state_dict()."""
    tu = pn2.tf_util
    store = tu.ParamStore(seed=3)
    before = {k: v.clone() for k, v in store.conv("a/conv0", 9, 32).items()}
    assert not store.is_trainable and not any(v.requires_grad for v in store.values())
    assert store.trainable("cpu") is store and store.is_trainable
    store.conv("a/conv1", 32, 64)
    store.dense("a/q", 64, 64)
    for name, t in store.items():
        assert t.is_leaf and t.requires_grad == (not name.endswith(("moving_mean",
                                                                    "moving_variance"))), name
    params = list(store.parameters())
    assert len(params) == 4 + 4 + 2
    assert all(any(p is t for t in store.values()) for p in params)
    sd = store.state_dict()
    assert sorted(sd) == sorted(store)
    assert sd["a/conv0/weights"].shape == (1, 1, 9, 32)
    assert (sd["a/conv0/weights"].reshape(9, 32) == before["weights"].numpy()).all()
    # a checkpoint round trip gives an equal, plain store
    again = tu.ParamStore(sd)
    assert not again.is_trainable
    assert all(torch.equal(again[k], store[k].detach()) for k in store)
    # the packed-layer cache follows in-place changes of a trainable store's variables
    s0 = store.stamp(["a/conv0"], tu.CONV_SUFFIXES)
    with torch.no_grad():
        store["a/conv0/weights"].add_(1.0)
    assert store.stamp(["a/conv0"], tu.CONV_SUFFIXES) != s0
    assert tu.ParamStore().stamp(["a/conv0"], tu.CONV_SUFFIXES) is None


def test_conv2d_training_needs_a_trainable_store(pn2):
    tu = pn2.tf_util
    with pytest.raises(NotImplementedError, match=r"ParamStore\.trainable\(\)"):
        tu.conv2d(torch.zeros(1, 4, 1, 9), 32, [1, 1], "c", bn=True, is_training=True,
                  params=tu.ParamStore())
    with pytest.raises(NotImplementedError, match=r"ParamStore\.trainable\(\)"):
        tu.conv1d(torch.zeros(1, 4, 9), 32, 1, "c", bn=True, is_training=True,
                  params=tu.ParamStore())
