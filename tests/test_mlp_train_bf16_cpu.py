"""CPU: the training layer's opt-in bf16 matrix-core mode (csrc/mlp_train.hip pn2_mlp_wgrad_bf16,
torch.ops.pn2.mlp_layer_train_bf16 and its three namesakes, tf_util.ParamStore's
train_precision): schemas, Meta results, no CPU kernel, the names' tuple, the argument checks of
the C entry point that return before any launch, the Python setting, and the numpy reference's
own sanity on the inputs tests/test_gpu_mlp_train_bf16.py uses. No kernel runs here."""
import numpy as np
import pytest
import torch

import mlp_train_bf16_ref as R

E = -22
FWD = ("mlp_layer_train", "mlp_layer_train_pool")
PAIRS = [(n, n + "_bf16") for n in FWD] + [(n + "_grad", n + "_bf16_grad") for n in FWD]


@pytest.fixture(scope="module")
def ops():
    import pn2hip
    return pn2hip.ops


def test_schemas_are_the_fp32_ops(ops):
    """Each _bf16 op has its fp32 namesake's schema but for the name, kernels under CUDA and Meta
    and none under CPU, and the two forward ops carry autograd."""
    for fp32, bf16 in PAIRS:
        want = str(getattr(ops, fp32)._schemas[""]).replace(f"pn2::{fp32}(", f"pn2::{bf16}(")
        assert str(getattr(ops, bf16)._schemas[""]) == want
        has = lambda key: torch._C._dispatch_has_kernel_for_dispatch_key(f"pn2::{bf16}", key)  # noqa: E731
        assert has("CUDA") and has("Meta") and not has("CPU"), bf16
    for name in FWD:
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f"pn2::{name}_bf16", "Autograd")
    assert str(ops.mlp_layer_train_bf16._schemas[""]) == (
        "pn2::mlp_layer_train_bf16(Tensor x, Tensor weight, Tensor? bias, Tensor? gamma, "
        "Tensor? beta, float eps, bool relu) -> (Tensor out, Tensor y, Tensor mean, Tensor var)")


def test_names_tuple(ops):
    assert ops.TRAIN_BF16_NAMES == ("mlp_layer_train_bf16", "mlp_layer_train_bf16_grad",
                                    "mlp_layer_train_pool_bf16", "mlp_layer_train_pool_bf16_grad")
    for name in ops.TRAIN_BF16_NAMES:
        assert name in ops.__all__ and hasattr(ops, name)
        assert name not in ops.NAMES + ops.HOST_NAMES + ops.FEED_NAMES


def same_meta(a, b):
    assert len(a) == len(b)
    for u, v in zip(a, b):
        assert u.shape == v.shape and u.dtype == v.dtype and u.stride() == v.stride()
        assert u.device.type == v.device.type == "meta"


@pytest.mark.parametrize("lead", [(2, 64, 16), (5, 8), (0, 16), (3, 0, 8)], ids=str)
@pytest.mark.parametrize("bn", [True, False])
def test_meta_results_are_the_fp32_ops(ops, lead, bn):
    """Shapes, dtypes and strides of both ops and both grad ops under Meta, zero rows included:
    those of the fp32 namesakes, and the documented ones."""
    m = lambda *s, dt=torch.float32: torch.empty(s, device="meta", dtype=dt)  # noqa: E731
    x, w, b = m(*lead, 9), m(9, 40), m(40)
    gamma, beta = (m(40), m(40)) if bn else (None, None)
    for pooled in (False, True):
        fwd32 = ops.mlp_layer_train_pool if pooled else ops.mlp_layer_train
        fwd16 = ops.mlp_layer_train_pool_bf16 if pooled else ops.mlp_layer_train_bf16
        got = fwd16(x, w, b, gamma, beta, 1e-3, True)
        same_meta(got, fwd32(x, w, b, gamma, beta, 1e-3, True))
        out, y, mean, var = got[:4]
        assert y.shape == lead + (40,) and y.dtype == torch.float32 and y.is_contiguous()
        assert out.shape == (lead[:-1] if pooled else lead) + (40,)
        assert mean.shape == var.shape == ((40,) if bn else (0,))
        if pooled:
            assert got[4].shape == out.shape and got[4].dtype == torch.int32
        stats = (mean, var) if bn else (None, None)
        for need in (True, False):
            if pooled:
                tail = (m(*out.shape), got[4], x, w, y, *stats, gamma, beta, 1e-3, True, need)
                g16 = ops.mlp_layer_train_pool_bf16_grad(*tail)
                g32 = ops.mlp_layer_train_pool_grad(*tail)
            else:
                tail = (m(*out.shape), x, w, y, *stats, gamma, beta, 1e-3, True, need)
                g16 = ops.mlp_layer_train_bf16_grad(*tail)
                g32 = ops.mlp_layer_train_grad(*tail)
            same_meta(g16, g32)
            gx, gw, gb, gg, gbeta = g16
            assert gx.shape == (x.shape if need else (0,)) and gw.shape == (9, 40)
            assert gb.shape == (40,) and gg.shape == gbeta.shape == ((40,) if bn else (0,))


@pytest.mark.parametrize("pooled", [False, True])
def test_autograd_on_meta_tensors(ops, pooled):
    m = lambda *s: torch.empty(s, device="meta", requires_grad=True)  # noqa: E731
    x, w, b, gamma, beta = m(2, 10, 9), m(9, 32), m(32), m(32), m(32)
    fwd = ops.mlp_layer_train_pool_bf16 if pooled else ops.mlp_layer_train_bf16
    out, y, *rest = fwd(x, w, b, gamma, beta, 1e-3, True)
    assert out.requires_grad and not y.requires_grad and not any(t.requires_grad for t in rest)
    out.sum().backward()
    for t in (x, w, b, gamma, beta):
        assert t.grad is not None and t.grad.shape == t.shape


def test_shape_errors(ops):
    m = lambda *s: torch.empty(s, device="meta")  # noqa: E731
    with pytest.raises(ValueError):
        ops.mlp_layer_train_bf16(m(10, 8), m(9, 32), None, None, None, 1e-3, True)
    with pytest.raises(ValueError):
        ops.mlp_layer_train_pool_bf16(m(9), m(9, 32), None, None, None, 1e-3, True)
    with pytest.raises(ValueError):
        ops.mlp_layer_train_bf16(m(10, 9), m(9, 32), None, m(32), None, 1e-3, True)


def test_no_cpu_kernel(ops):
    z = torch.zeros
    with pytest.raises(NotImplementedError):
        ops.mlp_layer_train_bf16(z(10, 9), z(9, 32), None, None, None, 1e-3, True)
    with pytest.raises(NotImplementedError):
        ops.mlp_layer_train_pool_bf16(z(2, 5, 9), z(9, 32), None, None, None, 1e-3, True)
    with pytest.raises(NotImplementedError):
        ops.mlp_layer_train_bf16_grad(z(10, 32), z(10, 9), z(9, 32), z(10, 32), None, None, None,
                                      None, 1e-3, True, True)
    with pytest.raises(NotImplementedError):
        ops.mlp_layer_train_pool_bf16_grad(z(2, 32), z(2, 32, dtype=torch.int32), z(2, 5, 9),
                                           z(9, 32), z(2, 5, 32), None, None, None, None, 1e-3,
                                           True, True)


def test_wgrad_bf16_checks_arguments_without_launching(pn2):
    lib = pn2.lib()
    fake = 1 << 20  # never dereferenced by the checks
    ws = lib.pn2_mlp_wgrad_workspace_size(100, 9, 32)
    f = lib.pn2_mlp_wgrad_bf16
    assert f(None, fake, 100, 9, 32, fake, fake, ws, None) == E        # x
    assert f(fake, None, 100, 9, 32, fake, fake, ws, None) == E        # grad_y
    assert f(fake, fake, 100, 9, 32, None, fake, ws, None) == E        # grad_w
    assert f(fake, fake, 100, 9, 32, fake, None, ws, None) == E        # workspace
    assert f(fake, fake, 100, 9, 32, fake, fake, ws - 1, None) == E    # too small
    assert f(fake, fake, 0, 9, 32, fake, fake, ws, None) == E          # rows
    assert f(fake, fake, -1, 9, 32, fake, fake, ws, None) == E
    assert f(fake, fake, 1 << 31, 9, 32, fake, fake, 1 << 40, None) == E  # rows cap
    assert f(fake, fake, 100, 0, 32, fake, fake, ws, None) == E        # cin
    assert f(fake, fake, 100, 9, -3, fake, fake, ws, None) == E        # cout
    # more (cin tile, cout tile group) pairs than a grid's y extent
    wide = lib.pn2_mlp_wgrad_workspace_size(1, 32 * 600, 32 * 600)
    assert f(fake, fake, 1, 32 * 600, 32 * 600, fake, fake, wide, None) == E


def test_train_precision_setting(pn2):
    tu = pn2.tf_util
    store = tu.ParamStore()
    assert store.train_precision == "fp32" and store.precision == "fp32"
    assert tu.ParamStore(train_precision="bf16").train_precision == "bf16"
    with pytest.raises(ValueError):
        tu.ParamStore(train_precision="fp16")
    with pytest.raises(ValueError):
        store.set_train_precision("half")
    assert store.train_precision == "fp32"
    # the setter returns the store and packs nothing, so it drops nothing
    store._packed["kept"] = object()
    assert store.set_train_precision("bf16") is store and store.train_precision == "bf16"
    assert "kept" in store._packed
    # independent of the inference precision, both ways
    assert store.precision == "fp32"
    store.set_precision("bf16").set_train_precision("fp32")
    assert (store.precision, store.train_precision) == ("bf16", "fp32")
    only_inference = tu.ParamStore(precision="bf16")
    assert only_inference.train_precision == "fp32"
    only_training = tu.ParamStore(train_precision="bf16")
    assert only_training.precision == "fp32"


def test_layers_carry_the_store_setting(pn2):
    tu = pn2.tf_util
    store = tu.ParamStore(train_precision="bf16")
    layers = tu.torch_layers(store, ["a/conv0", "a/conv1"], 9, [32, 64])
    assert [L.train_precision for L in layers] == ["bf16", "bf16"]
    store.set_train_precision("fp32")
    assert tu.torch_layers(store, ["a/conv0"], 9, [32])[0].train_precision == "fp32"
    assert tu.TorchLayer({}).train_precision == "fp32"
    with pytest.raises(ValueError):
        tu.TorchLayer({}, train_precision="int8")
    with pytest.raises(ValueError):
        tu.mlp_train(torch.zeros(4, 9), layers, precision="fp16")


# ---------------------------------------------------------------- the reference's own sanity
@pytest.mark.parametrize("shape", R.WGRAD_SHAPES, ids=R.shape_id)
def test_reference_exact_inputs_are_exact(shape):
    """On the layout test's inputs E = F = E32: rounding changes nothing and fp32 sums are exact."""
    x, gy = R.exact_inputs(shape)
    assert np.array_equal(R.bf16_round(x), x) and np.array_equal(R.bf16_round(gy), gy)
    e, f, e32 = (R.wgrad(x, gy, m) for m in ("E", "F", "E32"))
    assert np.array_equal(e, f) and np.array_equal(e32.astype(np.float64), e)


@pytest.mark.parametrize("shape", R.WGRAD_SHAPES, ids=R.shape_id)
def test_reference_standin_wgrad(shape):
    """E32 within 1/64 of max|E - F| on the weight gradient's random inputs."""
    x, gy = R.random_inputs(shape)
    e, f, e32 = (R.wgrad(x, gy, m) for m in ("E", "F", "E32"))
    gap, err = np.abs(e - f).max(), np.abs(e32 - e).max()
    print(f"{R.shape_id(shape)}: max|E - F| {gap:.3g}, max|E32 - E| {err:.3g}")
    assert gap > 0 and err <= gap / 64


@pytest.mark.parametrize("case", R.LAYER_CASES + R.POOL_CASES, ids=R.shape_id)
def test_reference_standin_layer(case):
    """The same for the forward product and the input gradient of the ops' cases (grad_out
    stands for grad_y: the GPU tests take the real one from the device)."""
    p = R.layer_inputs(case, True)
    gy = R._rng(case, 9).uniform(-1, 1, p["x"].shape[:-1] + (case[-1],)).astype(np.float32)
    for what, f in (("y", lambda m: R.forward(p["x"], p["w"], p["b"], m)),
                    ("grad_x", lambda m: R.grad_x(gy, p["w"], m)),
                    ("grad_w", lambda m: R.wgrad(p["x"], gy, m))):
        e, ff, e32 = f("E"), f("F"), f("E32")
        gap, err = np.abs(e - ff).max(), np.abs(e32 - e).max()
        print(f"{R.shape_id(case)} {what}: max|E - F| {gap:.3g}, max|E32 - E| {err:.3g}")
        assert gap > 0 and err <= gap / 64


def test_act_ref_matches_the_layer_reference():
    """act_ref on a given y is mlp_train_ref.ref_layer's formula after y."""
    from mlp_train_ref import make_params, ref_layer
    p = make_params(torch, 300, 9, 40, True, seed=1)
    (out, y, mean, var), _ = ref_layer(torch, p, torch.float64, True)
    o, m, v, _ = R.act_ref(y.detach().numpy(), p["gamma"].numpy(), p["beta"].numpy(), True,
                           np.float64)
    assert np.abs(o - out.detach().numpy()).max() < 1e-12
    assert np.abs(m - mean.detach().numpy()).max() < 1e-12
    assert np.abs(v - var.detach().numpy()).max() < 1e-12
