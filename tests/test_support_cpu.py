"""tests/support.py on hand-computed inputs: the tolerance rule, assert_close's four checks and
the bit comparisons. Every number below is exact in float64 (small multiples of powers of two
against the 1e-6 floor), so the expected tolerances are written as the rule's own expressions."""
import numpy as np
import pytest
import torch

from support import assert_close, f32_bits, raw_bits, same_bits, tolerance

REF64 = np.array([[1.0, -3.0, 0.5], [2.0, 0.0, -1.0]])   # max |ref64| = 3


def test_tolerance_floor():
    tol, err32 = tolerance(REF64, REF64.astype(np.float32))
    assert err32 == 0.0 and tol == 1e-6 * (1 + 3.0) == 4e-6


def test_tolerance_four_times_the_float32_error():
    ref32 = REF64.copy()
    ref32[1, 2] += 2.0 ** -10          # the largest float32 error
    ref32[0, 0] -= 2.0 ** -12
    tol, err32 = tolerance(REF64, ref32)
    assert err32 == 2.0 ** -10 and tol == 2.0 ** -8
    # just below the floor the floor wins: 4 * 2^-20 = 3.8e-6 < 4e-6
    tol, err32 = tolerance(REF64, REF64 + 2.0 ** -20)
    assert err32 == 2.0 ** -20 and tol == 4e-6


def test_tolerance_of_empty_arrays():
    assert tolerance(np.zeros((0, 4)), np.zeros((0, 4), np.float32)) == (1e-6, 0.0)
    assert_close(np.zeros((0, 4), np.float32), np.zeros((0, 4)), np.zeros((0, 4)), "empty")
    assert_close(torch.zeros(0), torch.zeros(0, dtype=torch.float64), torch.zeros(0), "empty")


def test_tolerance_takes_tensors_and_arrays_alike():
    ref32 = REF64 + 2.0 ** -10
    want = tolerance(REF64, ref32)
    assert tolerance(torch.from_numpy(REF64), torch.from_numpy(ref32)) == want
    assert tolerance(torch.from_numpy(REF64).requires_grad_(True), ref32) == want


def as_numpy(a):
    return np.asarray(a)


def as_torch(a):
    return torch.from_numpy(np.asarray(a)).requires_grad_(np.asarray(a).dtype.kind == "f")


@pytest.mark.parametrize("conv", [as_numpy, as_torch], ids=["numpy", "torch"])
def test_assert_close(conv, capsys):
    ref64 = REF64
    ref32 = REF64 + 2.0 ** -10                      # tol = 2^-8
    at = REF64.copy()
    at[0, 1] -= 2.0 ** -8                           # err == tol: exact in float32 too
    assert_close(conv(at.astype(np.float32)), conv(ref64), conv(ref32.astype(np.float32)), "at")
    assert "at: err 0.00391 tol 0.00391 (fp32 err 0.000977)" in capsys.readouterr().out
    above = at.copy()
    above[0, 1] = np.nextafter(np.float32(at[0, 1]), np.float32(-4))   # one float32 ulp further
    with pytest.raises(AssertionError, match="above: max err .* > tol"):
        assert_close(conv(above.astype(np.float32)), conv(ref64), conv(ref32), "above")
    with pytest.raises(AssertionError, match="shape"):
        assert_close(conv(REF64.T.copy()), conv(ref64), conv(ref32), "shape")
    with pytest.raises(AssertionError, match="shape"):   # not broadcast
        assert_close(conv(REF64[:1]), conv(ref64), conv(ref32), "shape")
    bad = REF64.copy()
    bad[1, 1] = np.nan
    with pytest.raises(AssertionError, match="nan: non-finite"):
        assert_close(conv(bad), conv(ref64), conv(ref32), "nan")
    bad[1, 1] = np.inf
    with pytest.raises(AssertionError, match="inf: non-finite"):
        assert_close(conv(bad), conv(ref64), conv(ref32), "inf")


def test_bits_tell_zero_from_minus_zero():
    a, b = np.array([0.0, 1.0], np.float32), np.array([-0.0, 1.0], np.float32)
    assert np.array_equal(a, b)
    assert f32_bits(a).dtype == np.int32 and f32_bits(b)[0] == np.int32(-2 ** 31)
    assert not np.array_equal(f32_bits(a), f32_bits(b))
    assert not np.array_equal(raw_bits(a), raw_bits(b))
    same_bits(a, a.copy(), "zero")
    with pytest.raises(AssertionError, match="zero: the bits of 1 of 2 values differ"):
        same_bits(a, b, "zero")
    with pytest.raises(AssertionError):
        same_bits(torch.from_numpy(a), torch.from_numpy(b), "zero")


def test_bits_tell_nan_payloads_apart():
    a = np.array([0x7FC00000, 0x7FC00001], np.uint32).view(np.float32)
    b = a[::-1].copy()
    assert np.isnan(a).all() and not np.array_equal(a, a)
    assert np.array_equal(f32_bits(a), f32_bits(a)) and not np.array_equal(f32_bits(a), f32_bits(b))
    assert np.array_equal(raw_bits(a), [0x7FC00000, 0x7FC00001])
    same_bits(a, a.copy(), "nan")
    with pytest.raises(AssertionError):
        same_bits(a, b, "nan")


def test_same_bits_refuses_differing_shapes_and_item_sizes():
    a = np.zeros((2, 3), np.float32)
    with pytest.raises(AssertionError):
        same_bits(a, a.reshape(3, 2), "shape")
    with pytest.raises(AssertionError):
        same_bits(a, a[:1], "shape")          # not broadcast
    with pytest.raises(AssertionError):
        same_bits(a, a.astype(np.float64), "item size")


def test_raw_bits_does_not_cast():
    i = np.array([1, -1, 1 << 30], np.int32)
    assert raw_bits(i).dtype == np.uint32 and np.array_equal(raw_bits(i), [1, 0xFFFFFFFF, 1 << 30])
    assert f32_bits(i)[0] == 0x3F800000                       # f32_bits does: 1 -> 1.0f
    assert raw_bits(np.array([1.0])).dtype == np.uint64
    assert raw_bits(np.array([True, False])).dtype == np.uint8
    assert raw_bits(torch.tensor([1, -1], dtype=torch.int32)).dtype == np.uint32
    assert raw_bits(i[::2]).shape == (2,)                     # a strided view: its own elements
    same_bits(i, i.view(np.float32), "an int32 array and the float32 array of its bytes")
