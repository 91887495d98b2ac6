"""GPU: the training-mode geometry of the SA and FP modules (csrc/geom_train.hip): the inverse
index, the ordered gradients of group_point and three_interpolate, the ops
torch.ops.pn2.group_concat_train / fp_apply_train and their wiring into pointnet_util.

Every bitwise comparison is np.array_equal on the raw fp32 (np.array_equal(-0.0, +0.0) is True,
so the sign of an untouched row is checked on the bit patterns as well).

  ordered grouping gradient       against the plain float32 loop `gp[key[s]] += go[s]` over
                                  ascending s, starting from +0.0
  ordered interpolation gradient  against the host twin pn2cpu_three_interpolate_grad (the
                                  reference's CPU loop, tf_interpolate.cpp:131-153)
  the ops                         forward against the fused no-grad kernels; gradients against
                                  the `_grad` ops (bits) and against a float64 evaluation with
                                  the project's tolerance (tests/support.py):
      max |gpu - f64|  <=  max(4 * max |fp32 - f64|,  1e-6 * (1 + max |f64|))
                                  where fp32 is the old composition's float-atomic gradient
  launch limits                   one case on each side of PN2_INV_MAX_KEYS, PN2_INV_MAX_SLOTS
                                  and the 65535 clouds of grid y, with integer-valued gradients
                                  (every partial sum is exact, so float64 np.add.at must match
                                  bit for bit, as in tests/test_gpu_launch_limits.py)
"""
import collections
import ctypes
import importlib

import numpy as np
import pytest

from conftest import PKG_NAME
from support import assert_close, gpu_marks

pytestmark = gpu_marks

E = -22
MAX_KEYS, MAX_SLOTS, MAX_BATCH = 16384, 1 << 20, 65535  # include/pn2hip.h


@pytest.fixture(scope="module")
def env():
    import torch
    pkg = importlib.import_module(PKG_NAME)
    import pn2hip
    return pkg, pn2hip.ops, torch, torch.device("cuda:0")


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a, b) and \
        np.array_equal(a.view(np.uint32) >> 31, b.view(np.uint32) >> 31)


# ---------------------------------------------------------------------------- C ABI helpers
def build_index(env, keys, K):
    """pn2_inverse_index_build over keys (B, S) int32 on the device -> the int32 workspace."""
    pkg, _, torch, dev = env
    lib = pkg.lib()
    B, S = int(keys.shape[0]), int(keys.shape[1])
    size = lib.pn2_inverse_index_size(B, S, K)
    assert size % 16 == 0 and size > 0
    inv = torch.full((size // 4,), -7, dtype=torch.int32, device=dev)
    assert inv.data_ptr() % 16 == 0
    rc = lib.pn2_inverse_index_build(keys.data_ptr(), B, S, K, inv.data_ptr(), size,
                                     torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    return inv


def index_parts(inv, B, S, K):
    w = inv.cpu().numpy()
    base = (B * (K + 1) + 3) // 4 * 4
    return w[:B * (K + 1)].reshape(B, K + 1), w[base:base + B * S].reshape(B, S)


def ordered_group_grad(env, go, keys, N, C, col0, guard=3):
    """pn2_group_point_grad_ordered of go (B, S, ld) float32 and keys (B, S) int32 (numpy):
    grad_points (B, N, C), written between `guard` sentinel rows that must stay untouched."""
    pkg, _, torch, dev = env
    B, S, ld = go.shape
    got = torch.from_numpy(np.ascontiguousarray(go)).to(dev)
    kt = torch.from_numpy(np.ascontiguousarray(keys, np.int32)).to(dev)
    inv = build_index(env, kt, N)
    SENT = 12345.0
    buf = torch.full((guard + B * N + guard, C), SENT, dtype=torch.float32, device=dev)
    rc = pkg.lib().pn2_group_point_grad_ordered(
        got.data_ptr(), ld, col0, inv.data_ptr(), B, N, C, S, 1,
        buf.data_ptr() + guard * C * 4, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[:guard] == SENT).all() and (out[guard + B * N:] == SENT).all(), "guard rows"
    return out[guard:guard + B * N].reshape(B, N, C), inv


def loop_group_grad(go, keys, N, C, col0):
    """The plain loop: for s in range(S): gp[key[s]] += go[s], float32, from +0.0; a key
    outside [0, N) is dropped."""
    B, S, _ = go.shape
    gp = np.zeros((B, N, C), np.float32)
    for b in range(B):
        for s in range(S):
            k = int(keys[b, s])
            if 0 <= k < N:
                gp[b, k] = gp[b, k] + go[b, s, col0:col0 + C]
    return gp


def ordered_interp_grad(env, go, idx, weight, m, C, col0):
    pkg, _, torch, dev = env
    B, n, ld = go.shape
    got = torch.from_numpy(np.ascontiguousarray(go)).to(dev)
    it = torch.from_numpy(np.ascontiguousarray(idx, np.int32)).to(dev)
    wt = torch.from_numpy(np.ascontiguousarray(weight, np.float32)).to(dev)
    inv = build_index(env, it.reshape(B, 3 * n), m)
    gp = torch.full((B, m, C), 12345.0, dtype=torch.float32, device=dev)
    rc = pkg.lib().pn2_three_interpolate_grad_ordered(
        got.data_ptr(), ld, col0, inv.data_ptr(), wt.data_ptr(), B, n, C, m, gp.data_ptr(),
        torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    return gp.cpu().numpy()


def twin_interp_grad(env, go, idx, weight, m):
    """pn2cpu_three_interpolate_grad on contiguous host arrays (B, n, C)."""
    pkg = env[0]
    go = np.ascontiguousarray(go, np.float32)
    idx = np.ascontiguousarray(idx, np.int32)
    weight = np.ascontiguousarray(weight, np.float32)
    B, n, C = go.shape
    gp = np.full((B, m, C), 777.0, np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    assert pkg.lib().pn2cpu_three_interpolate_grad(p(go), p(idx), p(weight), B, n, C, m, p(gp)) == 0
    return gp


# ---------------------------------------------------------------- ordered grouping gradient
B0, N0, M0, NS0 = 2, 100, 16, 8


@pytest.fixture(scope="module")
def group_case(env):
    """Shared inputs of the grouping cases: random idx, and idx from query_ball_point (which
    pads a group with copies of its first neighbour)."""
    pkg, _, torch, dev = env
    rng = np.random.default_rng(11)
    idx_rand = rng.integers(0, N0, (B0, M0 * NS0)).astype(np.int32)
    xyz = torch.from_numpy(rng.random((B0, N0, 3), np.float32)).to(dev)
    ball, cnt = pkg.tf_grouping.query_ball_point(0.3, NS0, xyz, xyz[:, :M0].contiguous())
    assert int(cnt.min()) < NS0, "some group must be padded"
    go = rng.standard_normal((B0, M0 * NS0, 263)).astype(np.float32)
    return idx_rand, ball.cpu().numpy().reshape(B0, M0 * NS0), go


@pytest.mark.parametrize("C", [1, 5, 64, 67, 260])
@pytest.mark.parametrize("layout", ["plain", "ssg", "msg"])
@pytest.mark.parametrize("source", ["random", "ball"])
def test_ordered_group_grad_equals_the_loop(env, group_case, C, layout, source):
    idx = group_case[0] if source == "random" else group_case[1]
    ld, col0 = {"plain": (C, 0), "ssg": (C + 3, 3), "msg": (C + 3, 0)}[layout]
    go = np.ascontiguousarray(group_case[2][:, :, :ld])
    got, _ = ordered_group_grad(env, go, idx, N0, C, col0)
    assert bits_equal(got, loop_group_grad(go, idx, N0, C, col0))


def test_inverse_index_is_the_stable_sort(env, group_case):
    _, _, torch, dev = env
    for keys in group_case[:2]:
        inv = build_index(env, torch.from_numpy(keys).to(dev), N0)
        off, slots = index_parts(inv, B0, M0 * NS0, N0)
        for b in range(B0):
            counts = np.bincount(keys[b], minlength=N0)
            assert np.array_equal(off[b], np.concatenate([[0], np.cumsum(counts)]))
            assert np.array_equal(slots[b], np.argsort(keys[b], kind="stable"))


def test_ordered_group_grad_single_point(env):
    rng = np.random.default_rng(3)
    go = rng.standard_normal((2, 24, 8)).astype(np.float32)
    idx = np.zeros((2, 24), np.int32)
    got, _ = ordered_group_grad(env, go, idx, 1, 5, 3)
    assert bits_equal(got, loop_group_grad(go, idx, 1, 5, 3))


@pytest.mark.parametrize("pattern", ["one_key", "two_keys"])
def test_ordered_group_grad_long_segments(env, pattern):
    """B = 1, N = 4, M = 64, ns = 32: all 2,048 slots on key 2 (longer than a wave and than a
    1,024-thread workgroup), or alternating between keys 1 and 3. Keys never named give +0.0."""
    rng = np.random.default_rng(5)
    S, N, C = 64 * 32, 4, 7
    idx = np.full((1, S), 2, np.int32) if pattern == "one_key" else \
        (1 + 2 * (np.arange(S) % 2)).astype(np.int32).reshape(1, S)
    go = rng.standard_normal((1, S, C + 3)).astype(np.float32)
    got, inv = ordered_group_grad(env, go, idx, N, C, 3)
    assert bits_equal(got, loop_group_grad(go, idx, N, C, 3))
    unused = [0, 1, 3] if pattern == "one_key" else [0, 2]
    assert (got[0, unused].view(np.uint32) == 0).all(), "a point no group took is +0.0"
    off, slots = index_parts(inv, 1, S, N)
    assert np.array_equal(slots[0], np.argsort(idx[0], kind="stable"))
    assert off[0, N] == S


def test_inverse_index_segment_length_thresholds(env):
    """Segments on each side of the sort kernel's thresholds, their slots interleaved at random:
    64, 128, 256 and 512 slots (one, two, four and eight registers per lane; 512 is the longest
    segment ranked in registers, 513 is rebuilt by the scan)."""
    rng = np.random.default_rng(8)
    lengths = [1, 63, 64, 65, 127, 128, 129, 0, 255, 256, 257, 511, 512, 513, 2]
    N = len(lengths)
    keys = rng.permutation(np.repeat(np.arange(N, dtype=np.int32), lengths))
    keys = np.stack([keys, rng.permutation(keys)])
    S = keys.shape[1]
    go = rng.standard_normal((2, S, 3)).astype(np.float32)
    got, inv = ordered_group_grad(env, go, keys, N, 3, 0)
    off, slots = index_parts(inv, 2, S, N)
    for b in range(2):
        assert np.array_equal(off[b], np.concatenate([[0], np.cumsum(lengths)]))
        assert np.array_equal(slots[b], np.argsort(keys[b], kind="stable"))
    assert bits_equal(got, loop_group_grad(go, keys, N, 3, 0))


def test_ordered_group_grad_drops_out_of_range_keys(env):
    rng = np.random.default_rng(6)
    S, N, C = M0 * NS0, 10, 6
    idx = rng.integers(-1, N + 1, (2, S)).astype(np.int32)  # -1 and N among them
    assert (idx == -1).any() and (idx == N).any()
    idx[1, :5] = [-1, N, 2 ** 31 - 1, -2 ** 31, N + 100]
    go = rng.standard_normal((2, S, C)).astype(np.float32)
    got, inv = ordered_group_grad(env, go, idx, N, C, 0, guard=64)  # (guard rows checked inside)
    assert bits_equal(got, loop_group_grad(go, idx, N, C, 0))
    off, slots = index_parts(inv, 2, S, N)
    for b in range(2):
        ok = (idx[b] >= 0) & (idx[b] < N)
        assert off[b, N] == ok.sum()
        order = np.argsort(np.where(ok, idx[b], N), kind="stable")[:ok.sum()]
        assert np.array_equal(slots[b, :ok.sum()], order)
        assert (slots[b, ok.sum():] == -7).all(), "slots past the total are not written"


# ----------------------------------------------------------- ordered interpolation gradient
def interp_inputs(seed, B, n, C, m, ld=None):
    rng = np.random.default_rng(seed)
    go = rng.standard_normal((B, n, ld or C)).astype(np.float32)
    idx = rng.integers(0, m, (B, n, 3)).astype(np.int32)
    weight = (rng.random((B, n, 3), np.float32) + np.float32(0.01)).astype(np.float32)
    return go, idx, weight


@pytest.mark.parametrize("C", [1, 5, 128, 260])
@pytest.mark.parametrize("m", [1, 3, 16])
def test_ordered_interp_grad_equals_the_host_twin(env, C, m):
    go, idx, weight = interp_inputs(100 + C + m, 2, 50, C, m)
    if m >= 3:  # rows that name one known point twice and three times
        idx[0, 0] = [2, 2, 1]
        idx[0, 1] = [0, 0, 0]
        idx[1, 49] = [1, 2, 1]
    got = ordered_interp_grad(env, go, idx, weight, m, C, 0)
    assert bits_equal(got, twin_interp_grad(env, go, idx, weight, m))


def test_ordered_interp_grad_single_unknown_point(env):
    go, idx, weight = interp_inputs(7, 2, 1, 5, 4)
    got = ordered_interp_grad(env, go, idx, weight, 4, 5, 0)
    assert bits_equal(got, twin_interp_grad(env, go, idx, weight, 4))


def test_ordered_interp_grad_long_segments(env):
    """n = 3000 unknown points on m = 2 known ones: segments of about 4,500 slots."""
    go, idx, weight = interp_inputs(8, 2, 3000, 5, 2)
    got = ordered_interp_grad(env, go, idx, weight, 2, 5, 0)
    assert bits_equal(got, twin_interp_grad(env, go, idx, weight, 2))


@pytest.mark.parametrize("C,ld,col0", [(5, 12, 3), (128, 131, 0), (64, 67, 3)])
def test_ordered_interp_grad_reads_columns_in_place(env, C, ld, col0):
    go, idx, weight = interp_inputs(9 + C, 2, 50, C, 16, ld=ld)
    got = ordered_interp_grad(env, go, idx, weight, 16, C, col0)
    assert bits_equal(got, twin_interp_grad(env, go[:, :, col0:col0 + C], idx, weight, 16))


# ------------------------------------------------------------------------------------- ops
class OpCounter:
    """Counts the pn2 operators that reach the dispatcher, autograd's backward calls included."""

    def __init__(self, torch):
        from torch.utils._python_dispatch import TorchDispatchMode
        counts = self.counts = collections.Counter()

        class Mode(TorchDispatchMode):
            def __torch_dispatch__(self, func, types, args=(), kwargs=None):
                counts[func.name()] += 1
                return func(*args, **(kwargs or {}))

        self.mode = Mode()

    def __enter__(self):
        self.mode.__enter__()
        return self.counts

    def __exit__(self, *a):
        return self.mode.__exit__(*a)


@pytest.fixture(scope="module")
def sa_case(env):
    pkg, _, torch, dev = env
    rng = np.random.default_rng(21)
    xyz = torch.from_numpy(rng.random((2, 300, 3), np.float32)).to(dev)
    points = torch.from_numpy(rng.standard_normal((2, 300, 13)).astype(np.float32)).to(dev)
    new_xyz = xyz[:, :40].contiguous()
    idx, _ = pkg.tf_grouping.query_ball_point(0.25, 16, xyz, new_xyz)
    return xyz, points, new_xyz, idx


LAYOUTS = [(True, False), (True, True), (False, False)]  # SSG, MSG, use_xyz=False


@pytest.mark.parametrize("use_xyz,xyz_last", LAYOUTS)
def test_group_concat_train_forward_and_gradient(env, sa_case, use_xyz, xyz_last):
    pkg, ops, torch, dev = env
    xyz, points, new_xyz, idx = sa_case
    pu = pkg.pointnet_util
    with torch.no_grad():
        ref, ref_gx = pu.group_concat(xyz, points, new_xyz, idx, use_xyz, xyz_last)
    assert torch.equal(ops.group_concat_train(xyz, points, new_xyz, idx, use_xyz, xyz_last), ref)
    # through the public function: the op runs, the forward bits and grouped_xyz are unchanged
    p = points.clone().requires_grad_()
    with OpCounter(torch) as counts:
        out, gx = pu.group_concat(xyz, p, new_xyz, idx, use_xyz, xyz_last)
        g = torch.from_numpy(np.random.default_rng(22).standard_normal(
            tuple(out.shape)).astype(np.float32)).to(dev)
        out.backward(g)
    assert counts["pn2::group_concat_train"] == 1 and counts["pn2::group_concat_train_grad"] == 1
    assert counts["pn2::group_point_grad"] == 0 and counts["pn2::group_point"] == 0
    assert torch.equal(out, ref) and torch.equal(gx, ref_gx) and not gx.requires_grad
    C = points.shape[2]
    col0 = 3 if (use_xyz and not xyz_last) else 0
    assert torch.equal(p.grad, ops.group_concat_train_grad(g, idx, 300, C, col0))
    # against the old composition's float-atomic gradient, float64 as the reference
    p_old = points.clone().requires_grad_()
    old, _ = pu.group_concat(xyz, p_old, new_xyz, idx, use_xyz, xyz_last, ordered_grad=False)
    assert torch.equal(old, ref)
    old.backward(g)
    ref64 = np.zeros((2, 300, C))
    gn = g.cpu().numpy().astype(np.float64)[..., col0:col0 + C].reshape(2, -1, C)
    for b in range(2):
        np.add.at(ref64[b], idx[b].cpu().numpy().reshape(-1), gn[b])
    assert_close(p.grad.cpu().numpy(), ref64, p_old.grad.cpu().numpy(), "grad_points")
    # a gradient that is not contiguous is made so once
    p2 = points.clone().requires_grad_()
    out2 = ops.group_concat_train(xyz, p2, new_xyz, idx, use_xyz, xyz_last)
    out2.backward(g.transpose(1, 2).contiguous().transpose(1, 2))
    assert torch.equal(p2.grad, p.grad)


def test_group_concat_without_points_or_gradient_is_unchanged(env, sa_case):
    pkg, ops, torch, dev = env
    xyz, points, new_xyz, idx = sa_case
    with OpCounter(torch) as counts:
        pkg.pointnet_util.group_concat(xyz, points, new_xyz, idx)         # no gradient asked
        pkg.pointnet_util.group_concat(xyz, None, new_xyz, idx)           # nothing to scatter
    assert counts["pn2::group_concat_train"] == 0
    out = ops.group_concat_train(xyz, None, new_xyz, idx, True, False)
    assert torch.equal(out, pkg.pointnet_util.group_concat(xyz, None, new_xyz, idx)[0])


@pytest.fixture(scope="module")
def fp_case(env):
    pkg, _, torch, dev = env
    rng = np.random.default_rng(31)
    xyz1 = torch.from_numpy(rng.random((2, 200, 3), np.float32)).to(dev)
    xyz2 = xyz1[:, :37].contiguous()  # some unknown points coincide with known ones (dist 0)
    p1 = torch.from_numpy(rng.standard_normal((2, 200, 9)).astype(np.float32)).to(dev)
    p2 = torch.from_numpy(rng.standard_normal((2, 37, 21)).astype(np.float32)).to(dev)
    return xyz1, xyz2, p1, p2


@pytest.mark.parametrize("with_points1", [True, False])
def test_fp_apply_train_forward_and_gradient(env, fp_case, with_points1):
    pkg, ops, torch, dev = env
    xyz1, xyz2, p1, p2 = fp_case
    if not with_points1:
        p1 = None
    pu = pkg.pointnet_util
    with torch.no_grad():
        ref = pu.fp_interpolate(xyz1, xyz2, p1, p2)
    dist, idx = pkg.tf_interpolate.three_nn(xyz1, xyz2)
    assert torch.equal(ops.fp_apply_train(dist, idx, p1, p2), ref)
    a1 = p1.clone().requires_grad_() if with_points1 else None
    a2 = p2.clone().requires_grad_()
    with OpCounter(torch) as counts:
        out = pu.fp_interpolate(xyz1, xyz2, a1, a2)
        g = torch.from_numpy(np.random.default_rng(32).standard_normal(
            tuple(out.shape)).astype(np.float32)).to(dev)
        out.backward(g)
    assert counts["pn2::fp_apply_train"] == 1 and counts["pn2::fp_apply_train_grad"] == 1
    assert counts["pn2::three_interpolate_grad"] == 0 and counts["pn2::three_interpolate"] == 0
    assert torch.equal(out, ref)
    C2, C1 = 21, 9 if with_points1 else 0
    g2, g1 = ops.fp_apply_train_grad(g, dist, idx, 37, C2, C1)
    assert torch.equal(a2.grad, g2)
    if with_points1:
        assert torch.equal(a1.grad, g1) and torch.equal(g1, g[:, :, C2:])
    # bit for bit the reference's CPU loop on the forward's weights
    weight = pkg.tf_interpolate.idw_weights(dist)
    twin = twin_interp_grad(env, g[:, :, :C2].cpu().numpy(), idx.cpu().numpy(),
                            weight.cpu().numpy(), 37)
    assert bits_equal(g2.cpu().numpy(), twin)
    # against the old composition's float-atomic gradient, float64 as the reference
    o2 = p2.clone().requires_grad_()
    interp = pkg.tf_interpolate.three_interpolate(o2, idx, weight)
    interp.backward(g[:, :, :C2].contiguous())
    ref64 = np.zeros((2, 37, C2))
    gw = g[:, :, :C2].cpu().numpy().astype(np.float64)[:, :, None, :] * \
        weight.cpu().numpy().astype(np.float64)[..., None]
    for b in range(2):
        np.add.at(ref64[b], idx[b].cpu().numpy().reshape(-1), gw[b].reshape(-1, C2))
    assert_close(g2.cpu().numpy(), ref64, o2.grad.cpu().numpy(), "grad_points2")
    # points1 alone asks for a gradient: its columns, no index
    if with_points1:
        b1 = p1.clone().requires_grad_()
        with OpCounter(torch) as counts:
            pu.fp_interpolate(xyz1, xyz2, b1, p2).backward(g)
        assert counts["pn2::fp_apply_train"] == 1 and counts["pn2::fp_apply_train_grad"] == 0
        assert torch.equal(b1.grad, g[:, :, C2:])


def test_backward_twice_gives_equal_bits(env):
    pkg, ops, torch, dev = env
    rng = np.random.default_rng(41)
    B, N, M, ns, C = 2, 1024, 128, 16, 6
    xyz = torch.from_numpy(rng.random((B, N, 3), np.float32)).to(dev)
    _, new_xyz = pkg.tf_sampling.farthest_point_sample_and_gather(M, xyz)
    idx, _ = pkg.tf_grouping.query_ball_point(0.2, ns, xyz, new_xyz)
    g = torch.from_numpy(rng.standard_normal((B, M, ns, C + 3)).astype(np.float32)).to(dev)
    runs = [ops.group_concat_train_grad(g, idx, N, C, 3) for _ in range(2)]
    assert torch.equal(runs[0], runs[1])
    n, m, C2 = 1024, 128, 24
    dist, nidx = pkg.tf_interpolate.three_nn(xyz, new_xyz)
    g = torch.from_numpy(rng.standard_normal((B, n, C2 + 5)).astype(np.float32)).to(dev)
    runs = [ops.fp_apply_train_grad(g, dist, nidx, m, C2, 5) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


# ------------------------------------------------------------------------ the whole step
def reduced_step(env, seed):
    """A reduced pointnet2_sem_seg: two SA and two FP modules, fc1, dropout with a fixed seed,
    fc2 and get_loss, on a fresh trainable store. Returns the loss, the input-feature gradient
    and every parameter gradient."""
    pkg, _, torch, dev = env
    pu, tu = pkg.pointnet_util, pkg.tf_util
    rng = np.random.default_rng(51)
    B, N, classes = 2, 1024, 5
    xyz = torch.from_numpy(rng.random((B, N, 3), np.float32)).to(dev)
    feats = torch.from_numpy(rng.standard_normal((B, N, 6)).astype(np.float32)).to(dev)
    feats.requires_grad_()
    labels = torch.from_numpy(rng.integers(0, classes, (B, N)).astype(np.int32)).to(dev)
    smpw = torch.from_numpy((rng.random((B, N)) > 0.2).astype(np.float32) * 1.5).to(dev)
    store = tu.ParamStore(seed=seed).trainable(dev)
    x1, p1, _ = pu.pointnet_sa_module(xyz, feats, 128, 0.2, 16, [16, 16, 32], None, False, True,
                                      None, "layer1", params=store)
    x2, p2, _ = pu.pointnet_sa_module(x1, p1, 32, 0.4, 16, [32, 32, 64], None, False, True, None,
                                      "layer2", params=store)
    f1 = pu.pointnet_fp_module(x1, x2, p1, p2, [32, 32], True, None, "fa_layer1", params=store)
    f0 = pu.pointnet_fp_module(xyz, x1, feats, f1, [32, 16], True, None, "fa_layer2",
                               params=store)
    net = tu.conv1d(f0, 16, 1, "fc1", padding="VALID", bn=True, is_training=True, bn_decay=None,
                    params=store)
    net = tu.dropout(net, True, "dp1", keep_prob=0.5, seed=1234)
    net = tu.conv1d(net, classes, 1, "fc2", padding="VALID", activation_fn=None,
                    is_training=True, params=store)
    loss = pkg.pointnet2_sem_seg.get_loss(net, labels, smpw)
    loss.backward()
    grads = {k: v.grad for k, v in store.items() if v.requires_grad}
    return loss.detach(), feats.grad, grads


def test_whole_training_step_is_reproducible(env):
    pkg, _, torch, dev = env
    with OpCounter(torch) as counts:
        loss_a, gf_a, grads_a = reduced_step(env, 3)
    assert counts["pn2::group_concat_train"] == 2 and counts["pn2::group_concat_train_grad"] == 2
    assert counts["pn2::fp_apply_train"] == 2 and counts["pn2::fp_apply_train_grad"] == 2
    assert counts["pn2::group_point_grad"] == 0 and counts["pn2::three_interpolate_grad"] == 0
    loss_b, gf_b, grads_b = reduced_step(env, 3)
    assert torch.equal(loss_a, loss_b)
    assert gf_a is not None and torch.equal(gf_a, gf_b) and float(gf_a.abs().max()) > 0
    # 2 x 3 SA layers, 2 x 2 FP layers and fc1 with weights, biases, gamma, beta; fc2 without BN
    assert sorted(grads_a) == sorted(grads_b) and len(grads_a) == 11 * 4 + 2
    for name in grads_a:
        assert grads_a[name] is not None and grads_b[name] is not None, name
        assert torch.equal(grads_a[name], grads_b[name]), name
    assert sum(float(g.abs().max()) > 0 for g in grads_a.values()) >= 30


def test_xyz_gradient_keeps_the_atomic_composition(env, sa_case, fp_case):
    pkg, ops, torch, dev = env
    xyz, points, new_xyz, idx = sa_case
    pu = pkg.pointnet_util
    x = xyz.clone().requires_grad_()
    p = points.clone().requires_grad_()
    with OpCounter(torch) as counts:
        out, _ = pu.group_concat(x, p, new_xyz, idx)
        g = torch.from_numpy(np.random.default_rng(61).standard_normal(
            tuple(out.shape)).astype(np.float32)).to(dev)
        out.backward(g)
    assert counts["pn2::group_concat_train"] == 0 and counts["pn2::group_point_grad"] == 2
    assert x.grad is not None and float(x.grad.abs().max()) > 0
    with torch.no_grad():
        assert torch.equal(out, pu.group_concat(xyz, points, new_xyz, idx)[0])
    C = points.shape[2]
    ref64 = np.zeros((2, 300, C))
    gn = g.cpu().numpy().astype(np.float64)[..., 3:].reshape(2, -1, C)
    for b in range(2):
        np.add.at(ref64[b], idx[b].cpu().numpy().reshape(-1), gn[b])
    ordered = ops.group_concat_train_grad(g, idx, 300, C, 3)
    assert_close(p.grad.cpu().numpy(), ref64, ordered.cpu().numpy(), "atomic grad_points")
    # new_xyz alone asking for a gradient keeps it as well
    nx = new_xyz.clone().requires_grad_()
    with OpCounter(torch) as counts:
        pu.group_concat(xyz, points.clone().requires_grad_(), nx, idx)[0].sum().backward()
    assert counts["pn2::group_concat_train"] == 0 and nx.grad is not None
    # and so does the FP geometry
    xyz1, xyz2, p1, p2 = fp_case
    a2 = p2.clone().requires_grad_()
    with OpCounter(torch) as counts:
        pu.fp_interpolate(xyz1.clone().requires_grad_(), xyz2, p1, a2).sum().backward()
    assert counts["pn2::fp_apply_train"] == 0 and counts["pn2::three_interpolate_grad"] == 1
    assert a2.grad is not None


def test_knn_grouping_keeps_the_composition(env, sa_case):
    """The kNN grouping of the attention modules (sample_and_group(knn=True)) is not rewired."""
    pkg, _, torch, dev = env
    xyz, points, _, _ = sa_case
    p = points.clone().requires_grad_()
    with OpCounter(torch) as counts:
        _, new_points, _, _ = pkg.pointnet_util.sample_and_group(40, 0.25, 16, xyz, p, knn=True)
        new_points.sum().backward()
    assert counts["pn2::group_concat_train"] == 0 and counts["pn2::group_point_grad"] >= 1
    with OpCounter(torch) as counts:
        _, new_points, _, _ = pkg.pointnet_util.sample_and_group(40, 0.25, 16, xyz, p)
        new_points.sum().backward()
    assert counts["pn2::group_concat_train"] == 1 and counts["pn2::group_point_grad"] == 0


# ----------------------------------------------------------------------------- launch limits
def exact_group_check(env, keys, N, C=1):
    """Integer-valued gradients: every partial sum is exact, float64 np.add.at must match."""
    rng = np.random.default_rng(71)
    B, S = keys.shape
    go = rng.integers(-2, 3, (B, S, C)).astype(np.float32)
    got, _ = ordered_group_grad(env, go, keys, N, C, 0)
    ref = np.zeros((B, N, C))
    for b in range(B):
        np.add.at(ref[b], keys[b], go[b].astype(np.float64))
    assert np.abs(ref).max() < 2 ** 24
    assert np.array_equal(got.astype(np.float64), ref)


def test_inverse_index_key_bound(env):
    """K = PN2_INV_MAX_KEYS keys (the counts fill the workgroup's dynamic LDS) runs; one more is
    rejected before any launch."""
    pkg, _, torch, dev = env
    rng = np.random.default_rng(72)
    keys = rng.integers(0, MAX_KEYS, (1, 40000)).astype(np.int32)
    keys[0, :2] = [0, MAX_KEYS - 1]
    exact_group_check(env, keys, MAX_KEYS)
    lib = pkg.lib()
    size = lib.pn2_inverse_index_size(1, 64, MAX_KEYS + 1)
    buf = torch.zeros(size // 4, dtype=torch.int32, device=dev)
    k = torch.zeros(64, dtype=torch.int32, device=dev)
    assert lib.pn2_inverse_index_build(k.data_ptr(), 1, 64, MAX_KEYS + 1, buf.data_ptr(), size,
                                       None) == E
    assert lib.pn2_group_point_grad_ordered(buf.data_ptr(), 1, 0, buf.data_ptr(), 1, MAX_KEYS + 1,
                                            1, 64, 1, buf.data_ptr(), None) == E
    torch.cuda.synchronize()
    assert int(buf.abs().max()) == 0, "a rejected call writes nothing"


def test_inverse_index_slot_bound(env):
    """S = PN2_INV_MAX_SLOTS slots per cloud over four keys (segments of about 262,144 slots,
    each rebuilt by one wave's scan of the cloud) runs; one more slot is rejected."""
    pkg, _, torch, dev = env
    rng = np.random.default_rng(73)
    keys = rng.integers(0, 4, (1, MAX_SLOTS)).astype(np.int32)
    exact_group_check(env, keys, 4)
    lib = pkg.lib()
    buf = torch.zeros(64, dtype=torch.int32, device=dev)
    big = 1 << 40  # (the sizes are checked before the workspace is)
    assert lib.pn2_inverse_index_build(buf.data_ptr(), 1, MAX_SLOTS + 1, 4, buf.data_ptr(), big,
                                       None) == E
    assert lib.pn2_group_point_grad_ordered(buf.data_ptr(), 1, 0, buf.data_ptr(), 1, 4, 1,
                                            MAX_SLOTS + 1, 1, buf.data_ptr(), None) == E
    assert lib.pn2_three_interpolate_grad_ordered(buf.data_ptr(), 1, 0, buf.data_ptr(),
                                                  buf.data_ptr(), 1, MAX_SLOTS // 3 + 1, 1, 4,
                                                  buf.data_ptr(), None) == E
    torch.cuda.synchronize()
    assert int(buf.abs().max()) == 0


def test_inverse_index_batch_bound(env):
    """B = 65535 clouds (grid y of the sort and gradient kernels) runs; 65536 is rejected."""
    pkg, _, torch, dev = env
    rng = np.random.default_rng(74)
    keys = rng.integers(0, 2, (MAX_BATCH, 3)).astype(np.int32)
    exact_group_check(env, keys, 2, C=2)
    lib = pkg.lib()
    buf = torch.zeros(64, dtype=torch.int32, device=dev)
    assert lib.pn2_inverse_index_build(buf.data_ptr(), MAX_BATCH + 1, 3, 2, buf.data_ptr(),
                                       1 << 40, None) == E
    assert lib.pn2_group_point_grad_ordered(buf.data_ptr(), 1, 0, buf.data_ptr(), MAX_BATCH + 1, 2,
                                            1, 3, 1, buf.data_ptr(), None) == E
    torch.cuda.synchronize()
    assert int(buf.abs().max()) == 0
