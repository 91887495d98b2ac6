"""The bf16 matrix-core mode without a GPU: the headroom of the chain bound on the very inputs
tests/test_gpu_mlp_bf16.py uses (E32, the float32 stand-in for the kernel, stays within 1/64 of
max|E - F| where the GPU test allows 1/16), the exact-operand inputs really are exact, and the
argument checks that need no launch. The evaluations E / F / E32 are in tests/mlp_bf16_ref.py.
"""
import importlib
import os

import numpy as np
import pytest

import mlp_bf16_ref as R
from conftest import PKG_NAME, ROOT


def test_bf16_round_is_nearest_even():
    x = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20,
                  1 + 2.0 ** -8 - 2.0 ** -20, 1.0, -1 - 2.0 ** -8, 3.0e38], np.float32)
    want = np.array([1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7, 1.0, 1.0, -1.0, 3.0e38], np.float32)
    got = R.bf16_round(x)
    assert np.array_equal(got[:6], want[:6])
    assert np.all((got.view(np.uint32) & 0xFFFF) == 0)
    try:
        import torch
    except ImportError:
        return
    y = np.random.default_rng(0).uniform(-4, 4, 4096).astype(np.float32)
    assert np.array_equal(R.bf16_round(y), torch.from_numpy(y).bfloat16().float().numpy())


def _check(what, evaluate):
    r, d = R.ratios(evaluate)
    print(f"{what}: max|E - F| = {d:.3g}, max|S - E| / max|E - F| = "
          + ", ".join(f"{m} {v:.2g}" for m, v in r.items()))
    assert d > 1e-4, f"{what}: the rounding must move the result (max|E - F| = {d:.3g})"
    assert max(r.values()) <= 1 / 64, (what, r)


@pytest.mark.parametrize("name", sorted(R.CHAINS))
def test_chain_bound_has_headroom(name):
    seeds = R.chain_seeds(name)
    assert len(set(seeds)) == 5
    for seed in seeds:
        _check(f"{name}/{seed}", R.chain_evaluate(name, seed))


@pytest.mark.parametrize("ns,C,pool,xyz_last", R.GROUP_CASES)
def test_group_bound_has_headroom(ns, C, pool, xyz_last):
    seed = R.group_seed(ns, C, pool, xyz_last)
    _check(f"group ns={ns} C={C} {pool} seed {seed}", R.group_evaluate(ns, C, pool, xyz_last, seed))


@pytest.mark.parametrize("C1", [0, 6])
def test_fp_bound_has_headroom(C1):
    seed = R.fp_seed(C1)
    _check(f"fp C1={C1} seed {seed}", R.fp_evaluate(C1, seed))


@pytest.mark.parametrize("C_in,widths,ns,B,M,add_max", R.ATTN_CASES)
def test_attention_bound_has_headroom(C_in, widths, ns, B, M, add_max):
    seed = R.attn_seed(C_in, tuple(widths), ns, B, M, add_max)
    _check(f"attention C={widths[-1]} add_max={add_max} seed {seed}",
           R.attn_evaluate(C_in, widths, ns, B, M, add_max, seed))


def test_exact_operands_are_exact():
    """The layout test's inputs: every evaluation gives the same bits, so the kernel's bf16 and
    fp32 paths must too."""
    cases = [(rows, cin, w) for rows in R.SHAPE_ROWS for cin in R.SHAPE_CINS
             for w in R.SHAPE_WIDTHS] + [R.BIG_SHAPE]
    for rows, cin, widths in cases:
        x, layers = R.exact_chain(np.random.default_rng([rows, cin, len(widths)]), rows, cin,
                                  widths)
        assert np.array_equal(R.bf16_round(x), x)
        y = x.astype(np.float64)
        for L in layers:
            assert np.array_equal(R.bf16_round(L["W"]), L["W"])
            y32 = y.astype(np.float32)
            assert np.array_equal(R.bf16_round(y32).astype(np.float64), y), (rows, cin, widths)
            y = R.layer_eval(y, L, "F")
        E, E32 = R.chain_eval(x, layers, "E"), R.chain_eval(x, layers, "E32")
        assert np.array_equal(E, y) and np.array_equal(E32.astype(np.float64), y)
        assert np.abs(y).max() > 0


# ---------------------------------------------------------------- argument checks (no launch)

def _header_text():
    with open(os.path.join(ROOT, "include", "pn2hip.h")) as fh:
        return fh.read()


def test_header_declares_the_mode_and_its_contract():
    pkg = importlib.import_module(PKG_NAME)
    assert pkg._lib.PN2_MLP_BF16 == 2 and pkg._lib.PN2_MLP_RELU == 1
    for name in ("pn2_mlp_packed_size_bf16", "pn2_mlp_pack_bf16"):
        assert name in pkg._lib.SIGNATURES
    assert pkg._lib.SIGNATURES["pn2_mlp_pack_bf16"] == pkg._lib.SIGNATURES["pn2_mlp_pack"]
    text = _header_text()
    for word in ("nearest-even", "ubnormal", "qkv[0]"):
        assert word in text


def _lib(pkg):
    return pkg._lib.lib()  # raises when the library is not built


@pytest.mark.parametrize("cin,cout", [(1, 1), (3, 32), (16, 33), (17, 64), (259, 512), (131, 21)])
def test_packed_size_bf16_formula(cin, cout):
    pkg = importlib.import_module(PKG_NAME)
    lib = _lib(pkg)
    assert int(lib.pn2_mlp_packed_size_bf16(cin, cout)) == R.packed_size_bf16(cin, cout)
    assert int(lib.pn2_mlp_packed_size_bf16(0, cout)) == 0
    # a 16-feature bf16 chunk takes the bytes of an 8-feature fp32 chunk
    assert R.packed_size_bf16(cin, cout) == int(lib.pn2_mlp_packed_size((cin + 1) // 2, cout))


def test_pack_bf16_rejects_an_undersized_buffer():
    """PN2_EINVAL before any launch: the pointers are never dereferenced on the host."""
    pkg = importlib.import_module(PKG_NAME)
    lib = _lib(pkg)
    need = int(lib.pn2_mlp_packed_size_bf16(19, 40))
    fake = 0x1000  # 16-byte aligned, never read: the size check comes first
    assert lib.pn2_mlp_pack_bf16(fake, None, None, None, 19, 40, fake, need - 1, None) == \
        pkg._lib.PN2_EINVAL
    assert lib.pn2_mlp_pack_bf16(fake, None, None, None, 19, 40, fake + 4, need, None) == \
        pkg._lib.PN2_EINVAL  # misaligned
    assert lib.pn2_mlp_pack_bf16(None, None, None, None, 19, 40, fake, need, None) == \
        pkg._lib.PN2_EINVAL


def test_bf16_query_is_rejected_before_any_launch():
    pkg = importlib.import_module(PKG_NAME)
    lib = _lib(pkg)
    L = pkg._lib
    fake = 0x1000
    layers = (L.MlpLayer * 1)(L.MlpLayer(fake, 3, 32, L.PN2_MLP_RELU | L.PN2_MLP_BF16))

    def qkv(qflag):
        return (L.MlpLayer * 3)(L.MlpLayer(fake, 32, 32, qflag),
                                L.MlpLayer(fake, 32, 32, L.PN2_MLP_BF16),
                                L.MlpLayer(fake, 32, 32, L.PN2_MLP_BF16))

    # B = 0: with valid arguments nothing is launched and the call returns PN2_OK
    args = (None, None, None, None, 0, 64, 0, 4, 32, L.PN2_USE_XYZ, 1, layers)
    assert lib.pn2_group_mlp_attention(*args, qkv(0), None, None, 0, None, None) == L.PN2_OK
    assert lib.pn2_group_mlp_attention(*args, qkv(L.PN2_MLP_BF16), None, None, 0, None,
                                       None) == L.PN2_EINVAL


def test_unknown_precision_is_rejected():
    pkg = importlib.import_module(PKG_NAME)
    tu = pkg.tf_util
    with pytest.raises(pkg.InvalidArgumentError):
        tu.ParamStore(precision="fp16")
    store = tu.ParamStore()
    assert store.precision == "fp32"
    with pytest.raises(pkg.InvalidArgumentError):
        store.set_precision("half")
    with pytest.raises(pkg.InvalidArgumentError):
        tu.packed_mlp(store, ["s/conv0"], 3, [32], precision="bfloat16")
    with pytest.raises(pkg.InvalidArgumentError):
        tu.packed_dense(store, "s/q", 32, 32, precision=16)
    with pytest.raises(pkg.InvalidArgumentError):
        tu.PackedLayer(np.zeros((3, 32), np.float32), precision="int8", device="cpu")


def test_set_precision_invalidates_the_packed_caches():
    pkg = importlib.import_module(PKG_NAME)
    store = pkg.tf_util.ParamStore(precision="bf16")
    assert store.precision == "bf16"
    store._packed["k"] = object()
    store._stamps["k"] = None
    assert store.set_precision("fp32") is store
    assert store.precision == "fp32" and not store._packed and not store._stamps
