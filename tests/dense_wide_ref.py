"""Shared by the tests of the K-streamed layer kernel (csrc/mlp_wide.hip: pn2_dense_wide,
pn2_dense_wide_plan, torch.ops.pn2.dense_wide): the cases, the launch shape of a case, the C
calls and the numpy float64 / float32 evaluation behind support.assert_close. Inputs are drawn
as the fused MLP's tests draw theirs (mlp_ref.make_layers). Not a test module."""
import ctypes
import functools
import importlib

import numpy as np

from conftest import PKG_NAME
from mlp_ref import make_layers, mlp_f32

EINVAL = -22


def L():
    return importlib.import_module(PKG_NAME + "._lib")


def plan(rows, cin, cout, flags=0, packed=1 << 20):
    """(rc, row_tiles, k_slab, out_tiles_per_wg) of pn2_dense_wide_plan: host only, the packed
    pointer is checked for alignment and never read."""
    lib = L()
    tab = (lib.MlpLayer * 1)(lib.MlpLayer(packed, cin, cout, flags))
    out = [ctypes.c_int(-1) for _ in range(3)]
    rc = lib.lib().pn2_dense_wide_plan(rows, cin, tab, *(ctypes.addressof(o) for o in out))
    return (rc,) + tuple(o.value for o in out)


def lds_bytes(row_tiles, k_slab):
    """A workgroup's LDS by the header's formula: two slab buffers of 32 * row_tiles rows."""
    return 2 * 32 * row_tiles * (k_slab + 4) * 4


# ---- (1) values: rows x cin x cout, trimmed to the pairs (i + j) even of the cin x cout grid
ROWS = (1, 31, 33, 70)
CINS = (1, 7, 1027, 1280, 2051, 4099, "ks-1", "ks", "ks+1", "2ks+9")
COUTS = (1, 21, 32, 33, 256, 8192)
# (bias, batch-norm affine, relu)
FLAGS = ((True, True, True), (False, False, False), (True, False, True), (False, True, False))


def resolve_cin(spec, rows, cout):
    """A cin of CINS: the literal, or the one around the case's own slab width."""
    if isinstance(spec, int):
        return spec
    ks = plan(rows, 8, cout)[2]   # the slab width depends on rows and cout only
    return {"ks-1": ks - 1, "ks": ks, "ks+1": ks + 1, "2ks+9": 2 * ks + 9}[spec]


def value_cases():
    cases = []
    for i, cin in enumerate(CINS):
        for j, cout in enumerate(COUTS):
            if (i + j) % 2:
                continue
            n = len(cases)
            cases.append((ROWS[(i // 2 + j) % 4], cin, cout) + FLAGS[n % 4])
    # the other two accumulator shapes of the launch (2 x 2 and 1 x 2 tiles per wave), which a
    # layer over few rows reaches only through many output tiles
    cases += [(449, 40, 8192, True, True, True), (300, "ks+1", 8192, True, False, True)]
    return cases


def case_id(case):
    return "-".join(str(int(v)) if isinstance(v, bool) else str(v) for v in case)


# ---- (2) bits against pn2_shared_mlp, on shapes both kernels take
BITS_CASES = [(rows, cin, cout) for cin in (40, 131, 1024, 1027) for cout in (21, 64, 256)
              for rows in (33, 70)]


def draw(rows, cin, cout, bias=True, bn=True, relu=True, seed=None):
    """(x, [layer]) as mlp_ref draws them; without `bias` the biases are zeros."""
    rng = np.random.default_rng(rows * 31 + cin + 7 * cout if seed is None else seed)
    layers = make_layers(rng, cin, [cout], bn=bn, relu=relu)
    if not bias:
        layers[0]["biases"] = np.zeros(cout, np.float32)
    x = rng.uniform(-1, 1, (rows, cin)).astype(np.float32)
    return x, layers


def ref_f64(x, layers):
    """mlp_ref.mlp_f32's formulas in float64 (scale and shift as float32 values, as packed)."""
    y = np.asarray(x, np.float64)
    for lay in layers:
        y = y @ lay["weights"].astype(np.float64) + lay["biases"].astype(np.float64)
        if lay.get("gamma") is not None:
            s = lay["gamma"].astype(np.float64) / np.sqrt(
                lay["moving_variance"].astype(np.float64) + 1e-3)
            t = lay["beta"].astype(np.float64) - lay["moving_mean"].astype(np.float64) * s
            y = y * s + t
        if lay["relu"]:
            y = np.maximum(y, 0)
    return y


ref_f32 = mlp_f32


def packed_layer(pkg, layer):
    """tf_util.PackedLayer (fp32) of one drawn layer, on the GPU."""
    return pkg.tf_util.PackedLayer(layer["weights"], layer["biases"], layer.get("gamma"),
                                   layer.get("beta"), layer.get("moving_mean"),
                                   layer.get("moving_variance"), relu=layer["relu"])


def call_c(torch, P, x, out=None):
    """pn2_dense_wide through the C ABI on device tensors; out defaults to a NaN-filled buffer,
    so an element that is not stored shows."""
    lib = L()
    rows = x.numel() // P.cin
    if out is None:
        out = torch.full((rows, P.cout), float("nan"), dtype=torch.float32, device=x.device)
    tab = (lib.MlpLayer * 1)(P.struct())
    lib.check(lib.lib().pn2_dense_wide(lib.ptr(x), rows, P.cin, tab, lib.ptr(out),
                                       lib.stream_of(x)), "dense_wide")
    return out


@functools.lru_cache(maxsize=None)
def run_value_case(case):
    """One value case on the GPU (C entry point, NaN-filled out) with its references, once."""
    import torch
    pkg = importlib.import_module(PKG_NAME)
    rows, cin_spec, cout, bias, bn, relu = case
    cin = resolve_cin(cin_spec, rows, cout)
    x, layers = draw(rows, cin, cout, bias, bn, relu)
    P = packed_layer(pkg, layers[0])
    xd = torch.from_numpy(x).cuda()
    got = call_c(torch, P, xd)
    torch.cuda.synchronize()
    return cin, xd, P, got, ref_f64(x, layers), ref_f32(x, layers)
