"""CPU: the training-mode geometry ops (csrc/geom_train.hip; torch.ops.pn2.group_concat_train,
group_concat_train_grad, fp_apply_train, fp_apply_train_grad): schemas, Meta shapes, no CPU
kernel, the exported entry points of the inverse index and the ordered gradients, and their
argument checks, which return PN2_EINVAL (or 0 for empty work) before any launch. No kernel runs
here; tests/test_gpu_geom_train.py runs them on the MI355X."""
import os
import re
import subprocess

import pytest
import torch

E = -22
NEW_ENTRY_POINTS = ("pn2_inverse_index_size", "pn2_inverse_index_build",
                    "pn2_group_point_grad_ordered", "pn2_three_interpolate_grad_ordered")
NEW_OPS = ("group_concat_train", "group_concat_train_grad", "fp_apply_train",
           "fp_apply_train_grad")
MAX_KEYS, MAX_SLOTS = 16384, 1 << 20  # PN2_INV_MAX_KEYS, PN2_INV_MAX_SLOTS (include/pn2hip.h)


@pytest.fixture(scope="module")
def ops():
    import pn2hip
    return pn2hip.ops


def test_schemas(ops):
    assert str(ops.group_concat_train._schemas[""]) == (
        "pn2::group_concat_train(Tensor xyz, Tensor? points, Tensor new_xyz, Tensor idx, "
        "bool use_xyz, bool xyz_last) -> Tensor")
    assert str(ops.group_concat_train_grad._schemas[""]) == (
        "pn2::group_concat_train_grad(Tensor grad_new_points, Tensor idx, int N, int C, "
        "int col0) -> Tensor")
    assert str(ops.fp_apply_train._schemas[""]) == (
        "pn2::fp_apply_train(Tensor dist, Tensor idx, Tensor? points1, Tensor points2) -> Tensor")
    assert str(ops.fp_apply_train_grad._schemas[""]) == (
        "pn2::fp_apply_train_grad(Tensor grad_out, Tensor dist, Tensor idx, int m, int C2, "
        "int C1) -> (Tensor, Tensor)")
    for name in NEW_OPS:
        assert name in ops.NAMES
        has = lambda key: torch._C._dispatch_has_kernel_for_dispatch_key(f"pn2::{name}", key)  # noqa: E731
        assert has("CUDA") and has("Meta") and not has("CPU")
    for name in ("group_concat_train", "fp_apply_train"):
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f"pn2::{name}", "Autograd")


def test_meta_shapes(ops):
    m = lambda *s, dt=torch.float32: torch.empty(s, device="meta", dtype=dt)  # noqa: E731
    xyz, pts, nx, idx = m(2, 100, 3), m(2, 100, 5), m(2, 16, 3), m(2, 16, 8, dt=torch.int32)
    for use_xyz, xyz_last, cout in ((True, False, 8), (True, True, 8), (False, False, 5)):
        out = ops.group_concat_train(xyz, pts, nx, idx, use_xyz, xyz_last)
        assert out.shape == (2, 16, 8, cout) and out.dtype == torch.float32
    assert ops.group_concat_train(xyz, None, nx, idx, True, False).shape == (2, 16, 8, 3)
    gp = ops.group_concat_train_grad(m(2, 16, 8, 8), idx, 100, 5, 3)
    assert gp.shape == (2, 100, 5) and gp.dtype == torch.float32
    assert ops.group_concat_train_grad(m(2, 16, 8, 8), idx, 1, 8, 0).shape == (2, 1, 8)

    dist, nidx = m(2, 50, 3), m(2, 50, 3, dt=torch.int32)
    out = ops.fp_apply_train(dist, nidx, m(2, 50, 7), m(2, 16, 12))
    assert out.shape == (2, 50, 19) and out.dtype == torch.float32
    assert ops.fp_apply_train(dist, nidx, None, m(2, 16, 12)).shape == (2, 50, 12)
    g2, g1 = ops.fp_apply_train_grad(m(2, 50, 19), dist, nidx, 16, 12, 7)
    assert g2.shape == (2, 16, 12) and g1.shape == (2, 50, 7)
    assert g2.dtype == g1.dtype == torch.float32
    g2, g1 = ops.fp_apply_train_grad(m(2, 50, 12), dist, nidx, 16, 12, 0)
    assert g2.shape == (2, 16, 12) and g1.shape == (2, 50, 0)


def test_autograd_on_meta_tensors(ops):
    """The C++ autograd runs end to end on fake tensors: points, points1 and points2 get a
    gradient of their own shape, the coordinates none."""
    m = lambda *s, dt=torch.float32, g=False: torch.empty(  # noqa: E731
        s, device="meta", dtype=dt, requires_grad=g)
    xyz, nx, idx = m(2, 100, 3), m(2, 16, 3), m(2, 16, 8, dt=torch.int32)
    for use_xyz, xyz_last in ((True, False), (True, True), (False, False)):
        pts = m(2, 100, 5, g=True)
        out = ops.group_concat_train(xyz, pts, nx, idx, use_xyz, xyz_last)
        assert out.requires_grad
        out.sum().backward()
        assert pts.grad.shape == (2, 100, 5)
    dist, nidx = m(2, 50, 3), m(2, 50, 3, dt=torch.int32)
    p1, p2 = m(2, 50, 7, g=True), m(2, 16, 12, g=True)
    ops.fp_apply_train(dist, nidx, p1, p2).sum().backward()
    assert p1.grad.shape == (2, 50, 7) and p2.grad.shape == (2, 16, 12)
    p2 = m(2, 16, 12, g=True)
    ops.fp_apply_train(dist, nidx, None, p2).sum().backward()
    assert p2.grad.shape == (2, 16, 12)
    p1 = m(2, 50, 7, g=True)  # points1 alone
    ops.fp_apply_train(dist, nidx, p1, m(2, 16, 12)).sum().backward()
    assert p1.grad.shape == (2, 50, 7)


@pytest.mark.parametrize("call", [
    lambda o, m, i: o.group_concat_train(m(2, 100), m(2, 100, 5), m(2, 16, 3), i(2, 16, 8), True, False),
    lambda o, m, i: o.group_concat_train(m(2, 100, 3), m(2, 100, 5), m(2, 16, 3), i(2, 128), True, False),
    lambda o, m, i: o.group_concat_train(m(2, 100, 3), m(2, 99, 5), m(2, 16, 3), i(2, 16, 8), True, True),
    lambda o, m, i: o.group_concat_train(m(2, 100, 3), m(200, 5), m(2, 16, 3), i(2, 16, 8), True, True),
    lambda o, m, i: o.group_concat_train_grad(m(2, 128, 8), i(2, 16, 8), 100, 5, 3),      # rank
    lambda o, m, i: o.group_concat_train_grad(m(2, 16, 8, 8), i(2, 128), 100, 5, 3),      # rank
    lambda o, m, i: o.group_concat_train_grad(m(2, 16, 8, 8), i(2, 16, 4), 100, 5, 3),    # ns
    lambda o, m, i: o.group_concat_train_grad(m(2, 16, 8, 8), i(2, 16, 8), 100, 6, 3),    # col0 + C
    lambda o, m, i: o.group_concat_train_grad(m(2, 16, 8, 8), i(2, 16, 8), 100, 5, -1),
    lambda o, m, i: o.group_concat_train_grad(m(2, 16, 8, 8), i(2, 16, 8), -1, 5, 0),
    lambda o, m, i: o.fp_apply_train(m(2, 50), i(2, 50, 3), None, m(2, 16, 12)),          # rank
    lambda o, m, i: o.fp_apply_train(m(2, 50, 3), i(2, 50), None, m(2, 16, 12)),
    lambda o, m, i: o.fp_apply_train(m(2, 50, 3), i(2, 50, 3), None, m(32, 12)),
    lambda o, m, i: o.fp_apply_train(m(2, 50, 3), i(2, 50, 3), m(2, 49, 7), m(2, 16, 12)),
    lambda o, m, i: o.fp_apply_train_grad(m(100, 19), m(2, 50, 3), i(2, 50, 3), 16, 12, 7),
    lambda o, m, i: o.fp_apply_train_grad(m(2, 50, 19), m(2, 50, 3), i(2, 50, 3), 16, 12, 6),
    lambda o, m, i: o.fp_apply_train_grad(m(2, 50, 19), m(2, 50), i(2, 50, 3), 16, 12, 7),
    lambda o, m, i: o.fp_apply_train_grad(m(2, 50, 19), m(2, 50, 3), i(2, 50, 3), -1, 12, 7),
])
def test_shape_errors(ops, call):
    m = lambda *s: torch.empty(s, device="meta")  # noqa: E731
    i = lambda *s: torch.empty(s, device="meta", dtype=torch.int32)  # noqa: E731
    with pytest.raises(ValueError):
        call(ops, m, i)


def test_no_cpu_kernel(ops):
    z = torch.zeros
    zi = lambda *s: torch.zeros(s, dtype=torch.int32)  # noqa: E731
    with pytest.raises(NotImplementedError):
        ops.group_concat_train(z(2, 100, 3), z(2, 100, 5), z(2, 16, 3), zi(2, 16, 8), True, False)
    with pytest.raises(NotImplementedError):
        ops.group_concat_train_grad(z(2, 16, 8, 8), zi(2, 16, 8), 100, 5, 3)
    with pytest.raises(NotImplementedError):
        ops.fp_apply_train(z(2, 50, 3), zi(2, 50, 3), None, z(2, 16, 12))
    with pytest.raises(NotImplementedError):
        ops.fp_apply_train_grad(z(2, 50, 12), z(2, 50, 3), zi(2, 50, 3), 16, 12, 0)


def test_mirror_refuses_cpu_tensors(pn2):
    """The training path of the mirror names the device, as every other mirror function does."""
    pu = pn2.pointnet_util
    with pytest.raises(RuntimeError, match="MI355X only"):
        pu.group_concat(torch.zeros(2, 100, 3), torch.zeros(2, 100, 5, requires_grad=True),
                        torch.zeros(2, 16, 3), torch.zeros(2, 16, 8, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="MI355X only"):
        pu.fp_interpolate(torch.zeros(2, 50, 3), torch.zeros(2, 16, 3), None,
                          torch.zeros(2, 16, 12, requires_grad=True))


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
    assert re.search(rf"#define PN2_INV_MAX_KEYS {MAX_KEYS}\b", text)
    assert "#define PN2_INV_MAX_SLOTS (1 << 20)" in text


def test_inverse_index_size(pn2):
    size = pn2.lib().pn2_inverse_index_size
    # offsets (B, K + 1) and slots (B, S), int32, each padded to 16 bytes
    assert size(1, 1, 1) == 16 + 16
    assert size(2, 8, 3) == 32 + 64
    assert size(16, 8192, 1024) == 4 * (16 * 1025 + 3) // 16 * 16 + 4 * 16 * 8192
    for B, S, K in ((0, 8, 3), (-1, 8, 3), (2, -1, 3), (2, 8, -1)):
        assert size(B, S, K) == 0
    base = (3, 100, 17)
    for axis in range(3):
        prev = 0
        for v in list(range(0, 70)) + [1000, 16384, 65535]:
            args = list(base)
            args[axis] = v
            got = size(*args)
            assert got % 16 == 0 and got >= prev, (axis, v)
            prev = got
    # 64-bit: 65535 clouds of the largest index
    assert size(65535, MAX_SLOTS, MAX_KEYS) > 65535 * 4 * (MAX_SLOTS + MAX_KEYS)


def test_inverse_index_build_checks_arguments_without_launching(pn2):
    lib = pn2.lib()
    fake = 1 << 20  # 16-byte aligned, never dereferenced by the checks
    ws = lib.pn2_inverse_index_size(2, 128, 100)

    def build(**kw):
        names = ("keys", "B", "S", "K", "inv", "inv_bytes", "stream")
        args = dict(zip(names, (fake, 2, 128, 100, fake, ws, None)))
        args.update(kw)
        return lib.pn2_inverse_index_build(*[args[n] for n in names])

    assert build(keys=None) == E and build(inv=None) == E          # null buffers
    assert build(inv_bytes=ws - 1) == E                            # one byte too small
    assert build(inv_bytes=0) == E
    for off in (4, 8, 12):
        assert build(inv=fake + off) == E                          # not 16-byte aligned
    for kw in (dict(B=-1), dict(S=-1), dict(K=-1)):
        assert build(**kw) == E, kw
    big = 1 << 40
    assert build(K=MAX_KEYS + 1, inv_bytes=big) == E               # the counts' LDS
    assert build(S=MAX_SLOTS + 1, inv_bytes=big) == E
    assert build(B=65536, inv_bytes=big) == E                      # clouds are grid rows
    # no clouds or no slots: a no-op that returns 0, whatever the buffers
    assert build(B=0) == 0 and build(S=0) == 0
    assert build(B=0, keys=None, inv=None, inv_bytes=0) == 0
    assert build(S=0, keys=None, inv=None, inv_bytes=0) == 0
    assert build(B=0, K=-1) == E                                   # the shape is checked first


def test_ordered_gradients_check_arguments_without_launching(pn2):
    lib = pn2.lib()
    fake = 1 << 20

    def group(**kw):
        names = ("grad_out", "ld", "col0", "inv", "B", "N", "C", "M", "nsample", "grad_points",
                 "stream")
        args = dict(zip(names, (fake, 67, 3, fake, 2, 100, 64, 16, 8, fake, None)))
        args.update(kw)
        return lib.pn2_group_point_grad_ordered(*[args[n] for n in names])

    def interp(**kw):
        names = ("grad_out", "ld", "col0", "inv", "weight", "B", "n", "C", "m", "grad_points",
                 "stream")
        args = dict(zip(names, (fake, 128, 0, fake, fake, 2, 50, 128, 16, fake, None)))
        args.update(kw)
        return lib.pn2_three_interpolate_grad_ordered(*[args[n] for n in names])

    for fn, bufs in ((group, ("grad_out", "inv", "grad_points")),
                     (interp, ("grad_out", "inv", "weight", "grad_points"))):
        for name in bufs:
            assert fn(**{name: None}) == E, name                   # null buffers
        for off in (4, 8, 12):
            assert fn(inv=fake + off) == E                         # a misaligned index
        assert fn(B=-1) == E and fn(C=-1) == E and fn(ld=-1) == E and fn(col0=-1) == E
        assert fn(B=65536) == E
        # no clouds: a no-op that returns 0, whatever the buffers; the shape is checked first
        assert fn(B=0) == 0
        assert fn(B=0, **{n: None for n in bufs}) == 0
        assert fn(C=0) == 0
        assert fn(B=0, col0=-1) == E
    # col0 + C > ld
    assert group(ld=66) == E and group(ld=64, col0=1) == E and group(C=65) == E
    assert interp(ld=127) == E and interp(col0=1) == E
    assert interp(ld=129, col0=1, B=0) == 0
    for kw in (dict(N=-1), dict(M=-1), dict(nsample=-1), dict(N=MAX_KEYS + 1),
               dict(M=1 << 10, nsample=(1 << 10) + 1), dict(M=1 << 16, nsample=1 << 16)):
        assert group(**kw) == E, kw
    assert group(N=0) == 0 and group(N=0, grad_points=None) == 0
    for kw in (dict(n=-1), dict(m=-1), dict(m=MAX_KEYS + 1), dict(n=MAX_SLOTS // 3 + 1)):
        assert interp(**kw) == E, kw
    assert interp(m=0) == 0
