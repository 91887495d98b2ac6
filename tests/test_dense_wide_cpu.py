"""CPU: the K-streamed layer kernel's entry points without a launch (pn2_dense_wide and
pn2_dense_wide_plan: PN2_EINVAL before any launch, rows = 0, the plan's numbers), the Meta kernel
of torch.ops.pn2.dense_wide, the ParamStore keyword and that pn2_shared_mlp_plan's answers are
what they were. tests/test_gpu_dense_wide.py runs the kernel on the MI355X."""
import ctypes

import pytest
import torch

from dense_wide_ref import CINS, COUTS, EINVAL, ROWS, L, lds_bytes, plan, resolve_cin, value_cases

FAKE = 1 << 20   # a 16-byte aligned address that is never read


def wide(x, rows, cin, layer, out):
    lib = L()
    tab = None if layer is None else (lib.MlpLayer * 1)(lib.MlpLayer(*layer))
    return lib.lib().pn2_dense_wide(x, rows, cin, tab, out, None)


def test_dense_wide_refuses_before_any_launch():
    good = (FAKE, 1280, 33, 0)
    assert wide(None, 10, 1280, good, FAKE) == EINVAL            # null x
    assert wide(FAKE, 10, 1280, good, None) == EINVAL            # null out
    assert wide(FAKE, 10, 1280, None, FAKE) == EINVAL            # null layer
    assert wide(FAKE, 10, 1280, (0, 1280, 33, 0), FAKE) == EINVAL  # null pack
    assert wide(FAKE, 10, 0, (FAKE, 0, 33, 0), FAKE) == EINVAL   # cin <= 0
    assert wide(FAKE, 10, -4, (FAKE, -4, 33, 0), FAKE) == EINVAL
    assert wide(FAKE, 10, 1280, (FAKE, 1280, 0, 0), FAKE) == EINVAL   # cout <= 0
    assert wide(FAKE, 10, 1280, (FAKE, 1280, -1, 0), FAKE) == EINVAL
    assert wide(FAKE, 10, 1280, (FAKE + 4, 1280, 33, 0), FAKE) == EINVAL  # misaligned pack
    assert wide(FAKE, 10, 1280, (FAKE, 1280, 33, L().PN2_MLP_BF16), FAKE) == EINVAL  # bf16 layer
    assert wide(FAKE, 10, 1280, (FAKE, 1280, 33, L().PN2_MLP_BF16 | L().PN2_MLP_RELU),
                FAKE) == EINVAL
    assert wide(FAKE, -1, 1280, good, FAKE) == EINVAL            # rows < 0
    assert wide(FAKE, 1 << 31, 1280, good, FAKE) == EINVAL       # rows > 2^31 - 1
    assert wide(FAKE, 10, 1279, good, FAKE) == EINVAL            # cin != the layer's
    assert wide(None, 0, 1280, good, None) == 0                  # no rows: OK, nothing to launch
    assert wide(FAKE, 0, 1280, (FAKE, 1280, 33, L().PN2_MLP_RELU), FAKE) == 0


def test_plan_refuses_the_same_arguments():
    assert plan(10, 0, 33)[0] == EINVAL and plan(10, -1, 33)[0] == EINVAL
    assert plan(10, 1280, 0)[0] == EINVAL and plan(10, 1280, -3)[0] == EINVAL
    assert plan(-1, 1280, 33)[0] == EINVAL and plan(1 << 31, 1280, 33)[0] == EINVAL
    assert plan(10, 1280, 33, packed=FAKE + 8)[0] == EINVAL
    assert plan(10, 1280, 33, packed=0)[0] == EINVAL
    assert plan(10, 1280, 33, flags=L().PN2_MLP_BF16)[0] == EINVAL
    assert plan(10, 1280, 33, flags=L().PN2_MLP_BF16)[1:] == (0, 0, 0)    # zeroed on error
    lib = L()
    tab = (lib.MlpLayer * 1)(lib.MlpLayer(FAKE, 1280, 33, 0))
    a, b = ctypes.c_int(-1), ctypes.c_int(-1)
    pa, pb = ctypes.addressof(a), ctypes.addressof(b)
    f = lib.lib().pn2_dense_wide_plan
    assert f(10, 1280, None, pa, pb, pa) == EINVAL               # null layer
    assert f(10, 1280, tab, None, pb, pa) == EINVAL              # null result pointers
    assert f(10, 1280, tab, pa, None, pb) == EINVAL
    assert f(10, 1280, tab, pa, pb, None) == EINVAL
    assert f(10, 1279, tab, pa, pb, pa) == EINVAL                # cin != the layer's
    assert plan(0, 1280, 33) == (0, 0, 0, 0)                     # no rows: nothing to plan


@pytest.mark.parametrize("rows", [1, 33, 70, 449, 1024, 4096, 32768, 1 << 20, (1 << 31) - 1])
def test_plan_numbers_are_positive_and_the_lds_fits(rows):
    """Every width up to the widest layers of the attention networks (12,288 in, 8,192 out): the
    numbers are positive, the slab is a multiple of 8, and two workgroups' LDS fit the CU's
    160 KiB."""
    for cin in (1, 7, 8, 1027, 1280, 2051, 4099, 8192, 12288):
        for cout in (1, 21, 32, 33, 64, 128, 256, 512, 8192):
            rc, rt, ks, ot = plan(rows, cin, cout)
            assert rc == 0, (rows, cin, cout)
            assert rt > 0 and ks > 0 and ot > 0 and ks % 8 == 0, (rows, cin, cout, rt, ks, ot)
            assert 2 * lds_bytes(rt, ks) <= 160 * 1024, (rows, cin, cout, rt, ks)
            # the slab and the tiles do not depend on cin
            assert plan(rows, 8, cout) == (rc, rt, ks, ot)
            # grid y
            assert -(-(-(-cout // 32)) // ot) <= 65535


def test_plan_takes_each_launch_shape():
    """The shapes the GPU tests rely on: few rows spread over the output tiles, many rows take
    two row tiles and two output tiles per wave."""
    assert plan(70, 1280, 256)[1:] == (1, 256, 4)
    assert plan(70, 1280, 33)[1:] == (2, 128, 2)
    assert plan(70, 1280, 21)[1:] == (4, 64, 1)
    assert plan(300, 257, 8192)[1:] == (1, 256, 8)
    assert plan(449, 40, 8192)[1:] == (2, 128, 8)
    assert plan(32768, 2051, 128)[1:] == (4, 64, 4)
    assert plan(256 * 256, 1280, 33)[1:] == (8, 32, 2)
    assert plan(1024, 12288, 256)[1:] == (1, 256, 4)


def test_value_cases_cover_the_boundaries():
    """The GPU value cases hit every rows / cin / cout of their sets, take the slab-relative cins
    from the plan, and reach all three accumulator shapes of the launch."""
    cases = value_cases()
    assert {c[0] for c in cases} >= set(ROWS) and {c[1] for c in cases} >= set(CINS)
    assert {c[2] for c in cases} == set(COUTS) and 24 <= len(cases) <= 48
    shapes = {plan(c[0], 8, c[2])[1:] for c in cases}
    assert {(1, 256, 4), (2, 128, 2), (4, 64, 1), (1, 256, 8), (2, 128, 8)} <= shapes
    assert resolve_cin("ks-1", 70, 256) == 255 and resolve_cin("2ks+9", 33, 21) == 137
    assert resolve_cin("ks", 31, 33) == 128 and resolve_cin(2051, 1, 1) == 2051


def m(*s, dt=torch.float32):
    return torch.empty(s, device="meta", dtype=dt)


def test_meta_kernel_shapes_and_dtypes():
    import pn2hip
    ops = pn2hip.ops
    assert str(ops.dense_wide._schemas[""]) == (
        "pn2::dense_wide(Tensor x, Tensor packed, int cin, int cout, bool relu) -> Tensor")
    has = lambda key: torch._C._dispatch_has_kernel_for_dispatch_key("pn2::dense_wide", key)  # noqa: E731
    assert has("CUDA") and has("Meta") and not has("CPU")
    nfloat = L().lib().pn2_mlp_packed_size(1280, 33) // 4
    out = ops.dense_wide(m(2, 5, 1280), m(nfloat), 1280, 33, True)
    assert out.shape == (2, 5, 33) and out.dtype == torch.float32 and out.is_contiguous()
    assert ops.dense_wide(m(0, 1280), m(nfloat), 1280, 33, False).shape == (0, 33)
    assert ops.dense_wide(m(7, 2560)[:, ::2], m(nfloat + 9), 1280, 33, False).stride() == (33, 1)
    with pytest.raises(ValueError):
        ops.dense_wide(m(5, 1279), m(nfloat), 1280, 33, True)       # x is not (..., cin)
    with pytest.raises(ValueError):
        ops.dense_wide(m(5, 1280), m(nfloat - 1), 1280, 33, True)   # pack too small
    with pytest.raises(ValueError):
        ops.dense_wide(m(5, 1280), m(nfloat), 1280, 0, True)
    with pytest.raises(TypeError):
        ops.dense_wide(m(5, 1280, dt=torch.float64), m(nfloat), 1280, 33, True)
    with pytest.raises(NotImplementedError):   # no CPU kernel: the dispatcher refuses
        ops.dense_wide(torch.zeros(5, 1280), torch.zeros(nfloat), 1280, 33, True)


def test_wide_layer_takes_gpu_tensors_only(pn2):
    """tf_util.WideLayer, what run_layers calls: a CPU tensor raises the project's usual text,
    and a bf16 pack is refused when the layer is made."""
    from types import SimpleNamespace
    tu = pn2.tf_util
    packed = SimpleNamespace(precision="fp32", cin=1280, cout=33, relu=True, buf=torch.zeros(4))
    layer = tu.WideLayer(packed)
    assert (layer.cin, layer.cout) == (1280, 33)
    with pytest.raises(RuntimeError, match="MI355X only"):
        layer(torch.zeros(5, 1280))
    with pytest.raises(TypeError):
        layer([[0.0] * 1280])
    packed.precision = "bf16"
    with pytest.raises(pn2.InvalidArgumentError, match="fp32 only"):
        tu.WideLayer(packed)


def test_wide_layers_keyword(pn2):
    tu = pn2.tf_util
    assert tu.ParamStore().wide_layers == tu.WIDE_LAYERS_DEFAULT
    assert tu.WIDE_LAYERS_DEFAULT in tu.WIDE_LAYERS == ("hip", "torch")
    for v in tu.WIDE_LAYERS:
        assert tu.ParamStore(wide_layers=v).wide_layers == v
    for bad in ("HIP", "", None, "bf16", 1):
        with pytest.raises(pn2.InvalidArgumentError):
            tu.ParamStore(wide_layers=bad)
    assert "wide_layers" not in tu.ParamStore(wide_layers="torch")   # a keyword, not a variable


def test_wide_accepts_and_plan_accepts_is_unchanged(pn2):
    """plan_accepts answers as before for the widths test_attn_net_cpu lists; wide_accepts takes
    every one of them, in both directions (the input gradient's layer is the transpose)."""
    ok, wide_ok = pn2.attention_layer.plan_accepts, pn2.attention_layer.wide_accepts
    for c in (8, 16, 32, 64):
        assert ok(c, (c,) * 4) and ok(c, (15 * c,)) and ok(5 * c, (c,)) and ok(c, (16 * c,))
    assert ok(1027, (64, 64, 128)) and ok(512, (8192,)) and ok(131, (16, 16, 16, 16))
    for cin, widths in ((2051, (128, 128, 256)), (4099, (256, 256, 512)), (12288, (256, 256)),
                        (2304, (256, 256)), (1280, (256, 128)), (1536, (256, 256)), (8192, (512,))):
        assert not ok(cin, widths), (cin, widths)
        assert wide_ok(cin, widths[0]) and wide_ok(widths[0], cin)
    assert not ok(8, (8,) * 7)
    assert wide_ok(1, 1) and not wide_ok(0, 8) and not wide_ok(8, 0)
