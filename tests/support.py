"""Shared by the test modules: the acceptance rule of the floating-point kernels, bit
comparisons, the GPU marks and the synthetic clouds. Not a test module and not a conftest:
pytest does not rewrite its asserts, so every assert here carries its own message."""
import numpy as np
import pytest

from conftest import gpu_available

gpu_marks = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]


def on_gpu(f):
    """gpu_marks on one test, for modules that also hold CPU tests."""
    for m in gpu_marks:
        f = m(f)
    return f


def _numpy(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


# ------------------------------------------------------------------------------ tolerance
def tolerance(ref64, ref32):
    """(tol, err32) of the project's floating-point bar

        max |gpu - f64|  <=  max(4 * max |fp32 - f64|,  1e-6 * (1 + max |f64|))

    where fp32 is the same reference evaluated in float32 on the CPU. Empty: (1e-6, 0)."""
    ref64 = np.asarray(_numpy(ref64), np.float64)
    ref32 = np.asarray(_numpy(ref32), np.float64)
    if not ref64.size:
        return 1e-6, 0.0
    err32 = np.abs(ref32 - ref64).max()
    return max(4 * err32, 1e-6 * (1 + np.abs(ref64).max())), err32


def assert_close(got, ref64, ref32, what):
    """got (numpy array or torch tensor, any device) is within tolerance(ref64, ref32) of ref64,
    has its shape and is finite."""
    got = np.asarray(_numpy(got), np.float64)
    ref64 = np.asarray(_numpy(ref64), np.float64)
    assert got.shape == ref64.shape, f"{what}: shape {got.shape}, expected {ref64.shape}"
    assert np.isfinite(got).all(), f"{what}: non-finite values"
    err = np.abs(got - ref64).max() if got.size else 0.0
    tol, err32 = tolerance(ref64, ref32)
    print(f"{what}: err {err:.3g} tol {tol:.3g} (fp32 err {err32:.3g})")
    assert err <= tol, f"{what}: max err {err:.3g} > tol {tol:.3g} (fp32 cpu err {err32:.3g})"


# ------------------------------------------------------------------------------------ bits
def f32_bits(a):
    """a as float32, its bit patterns as int32."""
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def raw_bits(a):
    """An array's bytes as unsigned integers of its own item size, no dtype cast: equality of
    bits, NaN and -0.0 included."""
    a = np.ascontiguousarray(_numpy(a))
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b, what=""):
    a, b = raw_bits(a), raw_bits(b)
    assert a.shape == b.shape and a.dtype == b.dtype, \
        f"{what}: {a.shape} of {a.dtype.itemsize} bytes vs {b.shape} of {b.dtype.itemsize} bytes"
    bad = np.flatnonzero(a.ravel() != b.ravel())
    assert bad.size == 0, f"{what}: the bits of {bad.size} of {a.size} values differ, " \
                          f"first at {bad[:1]}"


# ---------------------------------------------------------------------------------- clouds
def clouds(pkg, kind, B, N, seed=0):
    """(B, N, 3) float32 clouds of the parity tests' five kinds."""
    if kind in ("scannet", "uniform"):
        return pkg.synth.batch(range(seed, seed + B), N, kind)[0]
    if kind == "dup":  # every point the same: all distances tie
        return np.tile(np.array([[0.25, 0.5, 0.75]], np.float32), (B, N, 1)).reshape(B, N, 3)
    if kind == "grid":  # integer lattice: massive exact ties
        g = np.stack(np.meshgrid(*[np.arange(16)] * 3, indexing="ij"), -1).reshape(-1, 3)
        rng = np.random.default_rng(seed)
        return np.stack([g[rng.integers(0, len(g), N)] for _ in range(B)]).astype(np.float32)
    if kind == "fewuniq":  # 300 distinct points drawn with replacement: npoint > #unique
        rng = np.random.default_rng(seed)
        u = rng.random((300, 3)).astype(np.float32)
        return np.stack([u[rng.integers(0, 300, N)] for _ in range(B)])
    raise ValueError(kind)
