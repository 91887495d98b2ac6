"""GPU: the launchers' size limits -- batch chunking, grid-stride loops, fallbacks, rejections.

Nearly every index / gather / scatter kernel divides by a runtime divisor with FastDiv
(csrc/common.h), which is exact only while numerator * divisor < 2^32. The launchers keep that
bound by splitting the batch into several launches with offset pointers, by capping the grid
(the kernel then strides over its tasks), by taking another kernel, or by PN2_EINVAL. Every
test here first asserts, in plain integers and in FastDiv's own terms (`LIM`, the grid
constants below), that its shape is on the side of the bound it is meant for, so a shape that
is shrunk later fails the assertion instead of silently losing the coverage. Inputs differ per
cloud and indices reach 0 and N - 1, so a wrong chunk offset changes the result.

Per test: the bound, and the code that enforces it (csrc/).

  test_three_interpolate_chunked, test_three_interpolate_grad_chunked
      B*n*n >= 2^32 (rows b*n + j divided by n): interp.hip batch_chunk, the b0 loops of
      pn2_three_interpolate / pn2_three_interpolate_grad (15 + 1, 15 + 15 + 1, 1 + 1 launches).
  test_three_interpolate_rejects_n_65536            n*n >= 2^32: batch_chunk `per_b >= 2^32`.
  test_three_interpolate_channel_bound              rows*C*C >= 2^32: batch_chunk's first line.
  test_group_point_chunked, test_group_point_grad_chunked, test_group_concat_chunked
      B*M*M >= 2^32 (groups divided by M) and B*M*ns*ns >= 2^32 (rows divided by ns):
      group.hip batch_chunk, the b0 loops of launch_group and pn2_group_point_grad.
  test_group_accepts_m_65535_rejects_m_65536        M*M >= 2^32: batch_chunk `(lim - 1) / g`.
  test_group_channel_bound                          rows*Cout*Cout >= 2^32: batch_chunk.
  test_attention_generic_grid_stride, test_attention_grad_grid_stride
      G*H > 16384 waves: attn.hip grid_for (256 * 16 blocks of 4 waves), the `task += nwaves`
      loops of attn_reduce_generic_kernel / attn_reduce_grad_kernel.
  test_attention_specialised_sweeps
      tasks > 2 * 8192 and odd: grid_for(.., kAttnBlocksPerCu = 8), attn_reduce_kernel's
      `t0 += nwaves * TIF` loop and its `ok[1]` tail; and one sweep (tasks < 8192, odd).
  test_group_pool_grid_stride, test_group_pool_weighted_nsample_edges
      G > 16384 waves: grid_for, group_pool_kernel's `g +=` loop; ns <= 256 for weighted_avg:
      pn2_group_pool (the kernel's s_w[..][256]).
  test_attention_fallback_reduce, test_attention_fallback_layers
      G*(C/4)^2 >= 2^32: attn.hip attn_small_tasks, the generic launch of pn2_attn_reduce and
      the `big` list of pn2_attn_reduce_layers.
  test_prob_sample_more_clouds_than_grid_y          B > 65535: prob.hip `gy`, the
      `b += gridDim.y` loop of prob_search_kernel.
  test_three_nn_and_fp_batch_guard                  B > 65535 (blockIdx.y / the FP layer table):
      interp.hip pn2_three_nn, pn2_fp_fused.
  test_ball_group_layers_element_bound              E*Cout >= 2^32: sa_group.hip
      pn2_ball_group_layers.
  test_ball_group_grid_element_bound                nsmax*cout*cout >= 2^32: grid.hip
      ball_query_grid.
  test_fp_column_bound                              64*cw*cw >= 2^32: interp.hip fp_plan and
      fp_grid_launch (the latter's own test repeats fp_plan's with the same 64 rows, and
      fp_plan runs first, so it is pinned through pn2_fp_grid_fused, not separately).
  test_attention_large_logits                       no bound: logits of +-200 (max subtraction,
      segment width of the per-head reductions), all three attention kernels.

Left out: the third chunk condition of group.hip batch_chunk (B*M*ns >= 2^31 rows in one
launch). Reaching it needs 2^31 int32 indices, 8 GiB, before any output.

Exactness: features are small multiples of 2^-8, interpolation weights are the powers of two
(0.5, 0.25, 0.25) permuted per row and incoming gradients are small integers, so every product
and every partial sum is exact in fp32 whatever the order of the float atomics; the float64
restatements (np.add.at for the scatters) must then match bit for bit, with no tolerance.
"""
import importlib

import numpy as np
import pytest

from conftest import PKG_NAME
from support import f32_bits, gpu_marks

pytestmark = gpu_marks

TOL = dict(rtol=1e-5, atol=1e-5)  # README "Correctness targets"

# FastDiv (csrc/common.h): fdiv(n, d) is exact while n * d < LIM
LIM = 2 ** 32
# attn.hip: workgroups of 4 waves; grid_for caps the grid at 256 * per_cu workgroups
WAVES_PER_BLOCK = 4
GRID_CAP_WAVES = 256 * 16 * WAVES_PER_BLOCK  # generic attention, its grad, group_pool
SPEC_CAP_WAVES = 256 * 8 * WAVES_PER_BLOCK   # attn_reduce_kernel (kAttnBlocksPerCu = 8)
SPEC_TIF = 2                                 # its tasks in flight per wave (kAttnTif)
GRID_Y_MAX = 65535
TILE_ELEMS = 2048  # output floats per workgroup tile (group.hip / interp.hip kTileElems)


@pytest.fixture(scope="module")
def env():
    import torch

    from oracle import oracle as O
    O.set_threads(16)
    pkg = importlib.import_module(PKG_NAME)
    return pkg, O, torch, torch.device("cuda:0")


def _same_bits(a, b):
    return np.array_equal(f32_bits(a), f32_bits(b))


def _launches(B, *per_cloud):
    """Launches a batch of B clouds needs when one launch may hold only as many clouds as keep
    every numerator * divisor product (per_cloud: the product for one cloud) below LIM."""
    clouds = min((LIM - 1) // p for p in per_cloud)
    assert clouds >= 1
    return -(-B // clouds)


def _tile_rows(C):
    return 1 if C >= TILE_ELEMS else TILE_ELEMS // C


_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


# ------------------------------------------------------------------ three_interpolate (+grad)

def _interp_case(B, n, m, C):
    """Inputs (different per cloud, indices reach 0 and m - 1) and both float64 references."""
    def make():
        rng = np.random.default_rng([B, n, m, C])
        pts = (rng.integers(-2048, 2048, (B, m, C)) / 256.0).astype(np.float32)
        idx = rng.integers(0, m, (B, n, 3)).astype(np.int32)
        idx[:, 0, :] = 0
        idx[:, -1, :] = m - 1
        if n == 1:
            idx[:, 0, :] = [0, m // 2, m - 1]
        w = np.full((B, n, 3), 0.25, np.float32)
        np.put_along_axis(w, rng.integers(0, 3, (B, n, 1)), 0.5, axis=2)
        go = rng.integers(-8, 9, (B, n, C)).astype(np.float32)
        bi = np.arange(B)[:, None, None]
        w64 = w.astype(np.float64)[..., None]
        fwd = (pts.astype(np.float64)[bi, idx] * w64).sum(2)          # (B, n, C)
        grad = np.zeros((B * m, C), np.float64)
        np.add.at(grad, (bi * m + idx).ravel(),
                  (go.astype(np.float64)[:, :, None, :] * w64).reshape(-1, C))
        assert np.abs(grad).max() < 2 ** 22  # every partial sum is an exact multiple of 0.25
        return pts, idx, w, go, fwd, grad.reshape(B, m, C)
    return _cached(("interp", B, n, m, C), make)


# (B, n, m, launches)
INTERP_CASES = [(16, 16384, 8, 2), (31, 16384, 8, 3), (2, 46341, 8, 2), (2, 65535, 8, 2)]


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("B,n,m,launches", INTERP_CASES)
def test_three_interpolate_chunked(env, B, n, m, launches, C):
    """three_interpolate over more clouds than one launch's row / n division holds: exactly the
    float64 restatement, bit-equal to the oracle and, cloud by cloud, to the cloud run alone."""
    pkg, O, torch, dev = env
    assert B * n * n >= LIM and n * n < LIM and _launches(B, n * n) == launches
    assert _tile_rows(C) * C * C < LIM
    pts, idx, w, _, fwd, _ = _interp_case(B, n, m, C)
    tp, ti, tw = (torch.from_numpy(a).to(dev) for a in (pts, idx, w))
    got = pkg.tf_interpolate.three_interpolate(tp, ti, tw)
    gn = got.cpu().numpy()
    assert np.array_equal(gn.astype(np.float64), fwd), "differs from the float64 restatement"
    assert _same_bits(gn, O.three_interpolate(pts, idx, w)), "differs from the oracle"
    for b in range(B):
        alone = pkg.tf_interpolate.three_interpolate(tp[b:b + 1], ti[b:b + 1], tw[b:b + 1])
        assert torch.equal(alone[0], got[b]), f"cloud {b} differs from the cloud run alone"


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("B,n,m,launches", INTERP_CASES)
def test_three_interpolate_grad_chunked(env, B, n, m, launches, C):
    """three_interpolate_grad (float atomics) over the same batches: integer gradients and
    power-of-two weights make every sum exact, so it must equal np.add.at in float64."""
    pkg, O, torch, dev = env
    assert B * n * n >= LIM and n * n < LIM and _launches(B, n * n) == launches
    _, idx, w, go, _, grad = _interp_case(B, n, m, C)
    got = pkg.tf_interpolate.three_interpolate_grad(
        torch.zeros((B, m, C), device=dev), torch.from_numpy(idx).to(dev),
        torch.from_numpy(w).to(dev), torch.from_numpy(go).to(dev)).cpu().numpy()
    assert np.array_equal(got.astype(np.float64), grad)


def test_three_interpolate_rejects_n_65536(env):
    """n = 65536: one cloud's rows times the divisor n is already 2^32, no chunk can hold it.
    Forward and grad raise (PN2_EINVAL) instead of returning numbers."""
    pkg, O, torch, dev = env
    n, m, C = 65536, 8, 1
    assert n * n >= LIM
    pts = torch.zeros((1, m, C), device=dev)
    idx = torch.zeros((1, n, 3), dtype=torch.int32, device=dev)
    w = torch.zeros((1, n, 3), device=dev)
    with pytest.raises(pkg.InvalidArgumentError):
        pkg.tf_interpolate.three_interpolate(pts, idx, w)
    with pytest.raises(pkg.InvalidArgumentError):
        pkg.tf_interpolate.three_interpolate_grad(pts, idx, w, torch.zeros((1, n, C), device=dev))


def test_three_interpolate_channel_bound(env):
    """Tile elements divided by C: C = 65535 is accepted and exact, C = 65536 is rejected."""
    pkg, O, torch, dev = env
    B, n, m, C = 1, 1, 3, 65535
    assert _tile_rows(C) * C * C < LIM <= _tile_rows(C + 1) * (C + 1) * (C + 1)
    pts, idx, w, go, fwd, grad = _interp_case(B, n, m, C)
    ti, tw = torch.from_numpy(idx).to(dev), torch.from_numpy(w).to(dev)
    got = pkg.tf_interpolate.three_interpolate(torch.from_numpy(pts).to(dev), ti, tw).cpu().numpy()
    assert np.array_equal(got.astype(np.float64), fwd)
    assert _same_bits(got, O.three_interpolate(pts, idx, w))
    gg = pkg.tf_interpolate.three_interpolate_grad(torch.zeros((B, m, C), device=dev), ti, tw,
                                                   torch.from_numpy(go).to(dev)).cpu().numpy()
    assert np.array_equal(gg.astype(np.float64), grad)
    big = torch.zeros((B, m, C + 1), device=dev)
    with pytest.raises(pkg.InvalidArgumentError):
        pkg.tf_interpolate.three_interpolate(big, ti, tw)
    with pytest.raises(pkg.InvalidArgumentError):
        pkg.tf_interpolate.three_interpolate_grad(big, ti, tw, torch.zeros((B, n, C + 1), device=dev))


# ------------------------------------------------------- group_point (+grad), group_concat

def _group_case(B, N, M, ns, C):
    def make():
        rng = np.random.default_rng([B, N, M, ns, C])
        xyz = (rng.integers(-2048, 2048, (B, N, 3)) / 256.0).astype(np.float32)
        pts = (rng.integers(-2048, 2048, (B, N, C)) / 256.0).astype(np.float32)
        new_xyz = (rng.integers(-2048, 2048, (B, M, 3)) / 256.0).astype(np.float32)
        idx = rng.integers(0, N, (B, M, ns)).astype(np.int32)
        idx[:, 0, 0] = 0
        idx[:, -1, -1] = N - 1
        return xyz, pts, new_xyz, idx
    return _cached(("group", B, N, M, ns, C), make)


# (B, N, M, ns, launches): the groups / M division, then the rows / ns division
GROUP_CASES = [(16, 8, 16384, 1, 2), (64, 32, 64, 1024, 2)]


def _assert_group_chunked(B, M, ns, launches):
    assert B * M * M >= LIM or B * M * ns * ns >= LIM
    assert M * M < LIM and M * ns * ns < LIM
    assert _launches(B, M * M, M * ns * ns) == launches
    assert B * M * ns < 2 ** 31  # (not the row-count condition, which is left out)


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("B,N,M,ns,launches", GROUP_CASES)
def test_group_point_chunked(env, B, N, M, ns, launches, C):
    pkg, O, torch, dev = env
    _assert_group_chunked(B, M, ns, launches)
    _, pts, _, idx = _group_case(B, N, M, ns, C)
    tp, ti = torch.from_numpy(pts).to(dev), torch.from_numpy(idx).to(dev)
    got = pkg.tf_grouping.group_point(tp, ti)
    gn = got.cpu().numpy()
    ref = pts.astype(np.float64)[np.arange(B)[:, None, None], idx]
    assert np.array_equal(gn.astype(np.float64), ref), "differs from the float64 restatement"
    assert _same_bits(gn, O.group_point(pts, idx)), "differs from the oracle"
    for b in range(B):
        alone = pkg.tf_grouping.group_point(tp[b:b + 1], ti[b:b + 1])
        assert torch.equal(alone[0], got[b]), f"cloud {b} differs from the cloud run alone"


def _group_grad_f64(N, idx, go):
    B, M, ns, C = go.shape
    g = np.zeros((B * N, C), np.float64)
    np.add.at(g, (np.arange(B)[:, None, None] * N + idx).ravel(),
              go.astype(np.float64).reshape(-1, C))
    assert np.abs(g).max() < 2 ** 24
    return g.reshape(B, N, C)


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("B,N,M,ns,launches", GROUP_CASES)
def test_group_point_grad_chunked(env, B, N, M, ns, launches, C):
    pkg, O, torch, dev = env
    _assert_group_chunked(B, M, ns, launches)
    _, pts, _, idx = _group_case(B, N, M, ns, C)
    go = np.random.default_rng([7, B, M, ns, C]).integers(-8, 9, (B, M, ns, C)).astype(np.float32)
    got = pkg.tf_grouping.group_point_grad(torch.from_numpy(pts).to(dev),
                                           torch.from_numpy(idx).to(dev),
                                           torch.from_numpy(go).to(dev)).cpu().numpy()
    assert np.array_equal(got.astype(np.float64), _group_grad_f64(N, idx, go))


# (points?, use_xyz, xyz_last)
LAYOUTS = {"xyz_only": (False, True, False), "xyz_first": (True, True, False),
           "xyz_last": (True, True, True), "points_only": (True, False, False)}


def _group_concat_f64(xyz, pts, new_xyz, idx, use_xyz, xyz_last):
    bi = np.arange(xyz.shape[0])[:, None, None]
    gx = xyz.astype(np.float64)[bi, idx] - new_xyz.astype(np.float64)[:, :, None, :]
    if pts is None:
        return gx, gx
    gp = pts.astype(np.float64)[bi, idx]
    if not use_xyz:
        return gp, gx
    return np.concatenate([gp, gx] if xyz_last else [gx, gp], axis=-1), gx


def _check_group_concat(env, case, layout, per_cloud=True):
    pkg, O, torch, dev = env
    xyz, pts, new_xyz, idx = case
    has_pts, use_xyz, xyz_last = LAYOUTS[layout]
    if not has_pts:
        pts = None
    t = lambda a: None if a is None else torch.from_numpy(a).to(dev)  # noqa: E731
    tx, tp, tn, ti = t(xyz), t(pts), t(new_xyz), t(idx)
    run = lambda s: pkg.pointnet_util.group_concat(  # noqa: E731
        tx[s], None if tp is None else tp[s], tn[s], ti[s], use_xyz=use_xyz, xyz_last=xyz_last,
        want_grouped_xyz=True)
    out, gx = run(slice(None))
    ref_out, ref_gx = _group_concat_f64(xyz, pts, new_xyz, idx, use_xyz, xyz_last)
    on, gn = out.cpu().numpy(), gx.cpu().numpy()
    assert np.array_equal(on.astype(np.float64), ref_out), "new_points: float64 restatement"
    assert np.array_equal(gn.astype(np.float64), ref_gx), "grouped_xyz: float64 restatement"
    o_out, o_gx = O.group_concat(xyz, pts, new_xyz, idx, use_xyz=use_xyz, xyz_last=xyz_last)
    assert _same_bits(on, o_out), "new_points differs from the oracle"
    if pts is not None:
        assert _same_bits(gn, o_gx), "grouped_xyz differs from the oracle"
    if per_cloud:
        for b in range(xyz.shape[0]):
            o1, g1 = run(slice(b, b + 1))
            assert torch.equal(o1[0], out[b]) and torch.equal(g1[0], gx[b]), \
                f"cloud {b} differs from the cloud run alone"


@pytest.mark.parametrize("layout,C", [("xyz_only", 1), ("xyz_first", 1), ("xyz_first", 3),
                                      ("xyz_last", 1), ("xyz_last", 3), ("points_only", 1),
                                      ("points_only", 3)])
@pytest.mark.parametrize("B,N,M,ns,launches", GROUP_CASES)
def test_group_concat_chunked(env, B, N, M, ns, launches, layout, C):
    """The fused group + centre + concat in its three xyz layouts and points-only, each with
    grouped_xyz (points-only writes it in a second chunked launch_group)."""
    _assert_group_chunked(B, M, ns, launches)
    Cout = {"xyz_only": 3, "points_only": C}.get(layout, C + 3)
    assert _tile_rows(Cout) * Cout * Cout < LIM
    _check_group_concat(env, _group_case(B, N, M, ns, C), layout)


def test_group_accepts_m_65535_rejects_m_65536(env):
    """M = 65535 (one cloud, groups / M still exact) gives exact values; M = 65536 raises."""
    pkg, O, torch, dev = env
    B, N, M, ns, C = 1, 8, 65535, 1, 3
    assert B * M * M < LIM <= (M + 1) * (M + 1) and M * ns * ns < LIM
    case = _group_case(B, N, M, ns, C)
    _, pts, _, idx = case
    tp, ti = torch.from_numpy(pts).to(dev), torch.from_numpy(idx).to(dev)
    got = pkg.tf_grouping.group_point(tp, ti).cpu().numpy()
    assert np.array_equal(got.astype(np.float64), pts.astype(np.float64)[0][idx])
    assert _same_bits(got, O.group_point(pts, idx))
    go = np.random.default_rng(65535).integers(-8, 9, (B, M, ns, C)).astype(np.float32)
    gg = pkg.tf_grouping.group_point_grad(tp, ti, torch.from_numpy(go).to(dev)).cpu().numpy()
    assert np.array_equal(gg.astype(np.float64), _group_grad_f64(N, idx, go))
    for layout in LAYOUTS:
        _check_group_concat(env, case, layout, per_cloud=False)
    M = 65536
    ti = torch.zeros((B, M, ns), dtype=torch.int32, device=dev)
    zeros = lambda *s: torch.zeros(s, device=dev)  # noqa: E731
    with pytest.raises(pkg.InvalidArgumentError):
        pkg.tf_grouping.group_point(tp, ti)
    with pytest.raises(pkg.InvalidArgumentError):
        pkg.tf_grouping.group_point_grad(tp, ti, zeros(B, M, ns, C))
    for has_pts, use_xyz, xyz_last in LAYOUTS.values():
        with pytest.raises(pkg.InvalidArgumentError):
            pkg.pointnet_util.group_concat(zeros(B, N, 3), tp if has_pts else None,
                                           zeros(B, M, 3), ti, use_xyz=use_xyz,
                                           xyz_last=xyz_last)


def test_group_channel_bound(env):
    """Tile elements divided by Cout: Cout = 65535 accepted and exact, 65536 rejected."""
    pkg, O, torch, dev = env
    C = 65535
    assert _tile_rows(C) * C * C < LIM <= _tile_rows(C + 1) * (C + 1) * (C + 1)
    rng = np.random.default_rng(C)
    pts = (rng.integers(-2048, 2048, (1, 1, C)) / 256.0).astype(np.float32)
    idx = np.zeros((1, 1, 1), np.int32)
    tp, ti = torch.from_numpy(pts).to(dev), torch.from_numpy(idx).to(dev)
    got = pkg.tf_grouping.group_point(tp, ti).cpu().numpy()
    assert _same_bits(got, pts.reshape(1, 1, 1, C)) and _same_bits(got, O.group_point(pts, idx))
    go = rng.integers(-8, 9, (1, 1, 1, C)).astype(np.float32)
    gg = pkg.tf_grouping.group_point_grad(tp, ti, torch.from_numpy(go).to(dev)).cpu().numpy()
    assert _same_bits(gg, go.reshape(1, 1, C))
    xyz = np.array([[[0.25, -1.5, 3.0]]], np.float32)
    new_xyz = np.array([[[1.0, 0.5, -0.125]]], np.float32)
    _check_group_concat(env, (xyz, pts[..., :C - 3], new_xyz, idx), "xyz_first", per_cloud=False)
    _check_group_concat(env, (xyz, pts[..., :C - 3], new_xyz, idx), "xyz_last", per_cloud=False)
    big = torch.zeros((1, 1, C + 1), device=dev)
    with pytest.raises(pkg.InvalidArgumentError):
        pkg.tf_grouping.group_point(big, ti)
    with pytest.raises(pkg.InvalidArgumentError):
        pkg.tf_grouping.group_point_grad(big, ti, torch.zeros((1, 1, 1, C + 1), device=dev))
    with pytest.raises(pkg.InvalidArgumentError):  # Cout = C - 2 + 3 = 65536
        pkg.pointnet_util.group_concat(torch.from_numpy(xyz).to(dev), big[..., :C - 2],
                                       torch.from_numpy(new_xyz).to(dev), ti)


# ------------------------------------------------------------------ attention, group_pool

def _torch_attention(Q, K, V):
    """attention_layer.py:35-42 in plain torch (as tests/test_gpu_parity.py), reshape quirk
    included; float64 inputs give the float64 reference."""
    import torch
    B, M, ns, C = K.shape
    H = C // 4
    q = Q.reshape(B, M, H, 1, 4)
    k = K.reshape(B, M, H, ns, 4)
    v = V.reshape(B, M, H, ns, 4)
    w = torch.softmax(q @ k.transpose(-1, -2) / 2.0, dim=-1)
    return (w @ v).reshape(B, M, C)


def _qkv(seed, B, M, ns, C):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, (B, M, C)).astype(np.float32),
            rng.uniform(-1, 1, (B, M, ns, C)).astype(np.float32),
            rng.uniform(-1, 1, (B, M, ns, C)).astype(np.float32))


def _attention_f64(Q, K, V):
    import torch
    return _torch_attention(*(torch.from_numpy(a).double() for a in (Q, K, V))).numpy()


def _attention_grads_f64(Q, K, V, G):
    import torch
    rs = [torch.from_numpy(a).double().requires_grad_(True) for a in (Q, K, V)]
    _torch_attention(*rs).backward(torch.from_numpy(G).double())
    return [r.grad.numpy() for r in rs]


def _attention_grad_capi(env, Q, K, V, G):
    """pn2_attn_reduce_grad through the C ABI into NaN-filled outputs: an element the kernel
    never wrote stays NaN and fails the comparison."""
    pkg, O, torch, dev = env
    B, M, ns, C = K.shape
    tq, tk, tv, tg = (torch.from_numpy(a).to(dev) for a in (Q, K, V, G))
    outs = [torch.full_like(t, float("nan")) for t in (tq, tk, tv)]
    rc = pkg.lib().pn2_attn_reduce_grad(tq.data_ptr(), tk.data_ptr(), tv.data_ptr(),
                                        tg.data_ptr(), B, M, ns, C, outs[0].data_ptr(),
                                        outs[1].data_ptr(), outs[2].data_ptr(),
                                        torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0
    return [o.cpu().numpy() for o in outs]


# ns = 20 has no specialised instance: one wave per (group, head), 2 heads
STRIDE_M, STRIDE_NS, STRIDE_C = 8300, 20, 8


def _assert_generic_strides(M, ns, C):
    tasks = M * (C // 4)
    assert ns not in (8, 16, 32, 64, 128)
    # a second sweep that is partial: a few workgroups past the cap, not all of them
    assert GRID_CAP_WAVES + WAVES_PER_BLOCK < tasks < 2 * GRID_CAP_WAVES


def test_attention_generic_grid_stride(env):
    pkg, O, torch, dev = env
    M, ns, C = STRIDE_M, STRIDE_NS, STRIDE_C
    _assert_generic_strides(M, ns, C)
    Q, K, V = _qkv(1, 1, M, ns, C)
    got = pkg.attention_layer.attention_reduce(*(torch.from_numpy(a).to(dev) for a in (Q, K, V)))
    np.testing.assert_allclose(got.cpu().numpy(), _attention_f64(Q, K, V), **TOL)


def test_attention_grad_grid_stride(env):
    """dQ, dK, dV of 16600 (group, head) tasks on 16384 waves; every element written."""
    pkg, O, torch, dev = env
    M, ns, C = STRIDE_M, STRIDE_NS, STRIDE_C
    _assert_generic_strides(M, ns, C)
    Q, K, V = _qkv(2, 1, M, ns, C)
    G = np.random.default_rng(3).uniform(-1, 1, Q.shape).astype(np.float32)
    got = _attention_grad_capi(env, Q, K, V, G)
    for name, g, r in zip(("dQ", "dK", "dV"), got, _attention_grads_f64(Q, K, V, G)):
        np.testing.assert_allclose(g, r, err_msg=name, **TOL)
    # and through autograd, as the attention modules' training path reaches the kernel
    ts = [torch.from_numpy(a).to(dev).requires_grad_(True) for a in (Q, K, V)]
    pkg.attention_layer.attention_reduce(*ts).backward(torch.from_numpy(G).to(dev))
    for t, g in zip(ts, got):
        assert _same_bits(t.grad.cpu().numpy(), g)


@pytest.mark.parametrize("M", [16389, 4099])
def test_attention_specialised_sweeps(env, M):
    """ns = 8, C = 12: 8 heads per wave task, so one task per group. M = 16389: the grid is
    capped, the first sweep takes tasks 0 .. 16383 two per wave and the second sweep's waves
    have a valid first task and no second one. M = 4099: one sweep, odd, so the last wave's
    second task is past the end."""
    pkg, O, torch, dev = env
    ns, C = 8, 12
    lanes_per_head = min(ns, 64)
    steps = -(-(C // 4) // (64 // lanes_per_head))
    tasks = M * steps
    waves = -(-tasks // SPEC_TIF)  # launched: capped at SPEC_CAP_WAVES
    assert tasks % 2 == 1 and tasks * steps * steps < LIM
    if M == 16389:
        assert waves > SPEC_CAP_WAVES
        assert SPEC_TIF * SPEC_CAP_WAVES < tasks < SPEC_TIF * SPEC_CAP_WAVES + SPEC_CAP_WAVES
    else:
        assert tasks < SPEC_CAP_WAVES and waves <= SPEC_CAP_WAVES
    Q, K, V = _qkv(M, 1, M, ns, C)
    got = pkg.attention_layer.attention_reduce(*(torch.from_numpy(a).to(dev) for a in (Q, K, V)))
    np.testing.assert_allclose(got.cpu().numpy(), _attention_f64(Q, K, V), **TOL)


def _pool_f64(x, g, mode):
    """pointnet_util.py:130-145 in float64 numpy: (B,M,ns,C) -> (B,M,1,C')."""
    x = x.astype(np.float64)
    if mode == "max":
        return x.max(2, keepdims=True)
    if mode == "avg":
        return x.mean(2, keepdims=True)
    if mode == "weighted_avg":
        e = np.exp(-5.0 * np.sqrt((g.astype(np.float64) ** 2).sum(-1, keepdims=True)))
        return (x * (e / e.sum(2, keepdims=True))).sum(2, keepdims=True)
    return np.concatenate([x.mean(2, keepdims=True), x.max(2, keepdims=True)], -1)


def _pool_inputs(M, ns, C):
    def make():
        rng = np.random.default_rng([M, ns, C])
        return (rng.uniform(-1, 1, (1, M, ns, C)).astype(np.float32),
                rng.uniform(-0.2, 0.2, (1, M, ns, 3)).astype(np.float32))
    return _cached(("pool", M, ns, C), make)


@pytest.mark.parametrize("mode", ["max", "avg", "weighted_avg", "max_and_avg"])
def test_group_pool_grid_stride(env, mode):
    pkg, O, torch, dev = env
    M, ns, C = 16500, 5, 70
    assert GRID_CAP_WAVES + WAVES_PER_BLOCK < M < 2 * GRID_CAP_WAVES and C % 64 != 0
    x, g = _pool_inputs(M, ns, C)
    got = pkg.pointnet_util.group_pool(torch.from_numpy(x).to(dev), mode,
                                       torch.from_numpy(g).to(dev)).cpu().numpy()
    np.testing.assert_allclose(got, _pool_f64(x, g, mode), **TOL)


def test_group_pool_weighted_nsample_edges(env):
    """weighted_avg keeps a group's ns weights in 256 LDS floats per wave: ns = 1 and ns = 256
    are accepted, ns = 257 is rejected."""
    pkg, O, torch, dev = env
    M, C = 301, 70
    for ns in (1, 256):
        x, g = _pool_inputs(M, ns, C)
        got = pkg.pointnet_util.group_pool(torch.from_numpy(x).to(dev), "weighted_avg",
                                           torch.from_numpy(g).to(dev)).cpu().numpy()
        np.testing.assert_allclose(got, _pool_f64(x, g, "weighted_avg"), **TOL)
    with pytest.raises(pkg.InvalidArgumentError):
        pkg.pointnet_util.group_pool(torch.zeros((1, 2, 257, 4), device=dev), "weighted_avg",
                                     torch.zeros((1, 2, 257, 3), device=dev))


# ------------------------------------------------------- the attn_small_tasks fallback

@pytest.fixture(scope="module")
def fallback_case(env):
    """B = 1, M = 64, ns = 8, C = 32768 (K and V 67 MB each), made and referenced (float64) on
    the GPU: the CPU would take most of the test's time budget."""
    pkg, O, torch, dev = env
    M, ns, C = 64, 8, 32768
    assert M * (C // 4) ** 2 >= LIM > (M - 1) * (C // 4) ** 2
    gen = torch.Generator(device=dev).manual_seed(32768)
    Q = torch.rand((1, M, C), generator=gen, device=dev) * 2 - 1
    K = torch.rand((1, M, ns, C), generator=gen, device=dev) * 2 - 1
    V = torch.rand((1, M, ns, C), generator=gen, device=dev) * 2 - 1
    ref = _torch_attention(Q.double(), K.double(), V.double()).cpu().numpy()
    return Q, K, V, ref


def test_attention_fallback_reduce(env, fallback_case):
    """A layer whose task count times steps^2 reaches 2^32 takes the generic kernel (its task
    arithmetic is 64-bit) although ns = 8 has a specialised instance."""
    pkg, O, torch, dev = env
    Q, K, V, ref = fallback_case
    got = pkg.attention_layer.attention_reduce(Q, K, V)
    np.testing.assert_allclose(got.cpu().numpy(), ref, **TOL)


def test_attention_fallback_layers(env, fallback_case):
    """The same layer next to a small one in one pn2_attn_reduce_layers call: the small layer
    runs in the layers kernel (bit-equal to attention_reduce alone), the large one generic."""
    pkg, O, torch, dev = env
    Q, K, V, ref = fallback_case
    small = [torch.from_numpy(a).to(dev) for a in _qkv(7, 1, 7, 8, 12)]
    assert 7 * (12 // 4) ** 2 < LIM
    alone = pkg.attention_layer.attention_reduce(*small)
    for order in ([small, (Q, K, V)], [(Q, K, V), small]):
        outs = pkg.attention_layer.attention_reduce_layers(order)
        o_small, o_big = (outs[0], outs[1]) if order[0] is small else (outs[1], outs[0])
        assert torch.equal(o_small, alone)
        np.testing.assert_allclose(o_big.cpu().numpy(), ref, **TOL)
    np.testing.assert_allclose(alone.cpu().numpy(),
                               _attention_f64(*(t.cpu().numpy() for t in small)), **TOL)


# ------------------------------------------------------------------ the other bounds

def test_prob_sample_more_clouds_than_grid_y(env):
    """B = 65540 rows on a grid of 65535 in y: rows 65535 .. 65539 are a second trip of the
    search kernel's row loop. Draws sit mid-way inside their bins, so fp32 and float64 agree."""
    pkg, O, torch, dev = env
    B, N, M = 65540, 3, 2
    assert B > GRID_Y_MAX
    rng = np.random.default_rng(B)
    w = rng.uniform(0.1, 1.0, (B, N)).astype(np.float32)
    cum = np.cumsum(w.astype(np.float64), axis=1)
    edges = np.concatenate([np.zeros((B, 1)), cum], axis=1) / cum[:, -1:]
    want = rng.integers(0, N, (B, M))
    want[0], want[-1] = [0, N - 1], [N - 1, 0]
    lo, hi = np.take_along_axis(edges, want, 1), np.take_along_axis(edges, want + 1, 1)
    r = ((lo + hi) / 2).astype(np.float32)
    # every draw is farther from each boundary of the cumulative sums than fp32 can move it
    q = r.astype(np.float64) * cum[:, -1:]
    assert np.abs(q[:, :, None] - cum[:, None, :]).min() > 1e-3 * cum[:, -1].max()
    ref = (cum[:, None, :] < q[:, :, None]).sum(-1)  # searchsorted(cum[b], q, "left") per row
    assert np.array_equal(ref, want) and set(np.unique(ref)) == {0, 1, 2}
    got = pkg.tf_sampling.prob_sample(torch.from_numpy(w).to(dev),
                                      torch.from_numpy(r).to(dev)).cpu().numpy()
    assert np.array_equal(got, ref), f"{(got != ref).sum()} indices differ from float64"
    assert np.array_equal(got, O.prob_sample(w, r)), "differs from the oracle"


def test_three_nn_and_fp_batch_guard(env):
    """three_nn and the fused FP layer put the cloud in blockIdx.y / reject B > 65535:
    B = 65535 (n = 1, m = 3) matches float64 numpy, B = 65536 raises."""
    pkg, O, torch, dev = env
    B, n, m, C1, C2 = 65535, 1, 3, 1, 2
    assert B == GRID_Y_MAX
    rng = np.random.default_rng(B)
    # lattice coordinates: squared distances are exact in fp32, ties keep the lower index
    x1 = (rng.integers(0, 64, (B + 1, n, 3)) / 64.0).astype(np.float32)
    x2 = (rng.integers(0, 64, (B + 1, m, 3)) / 64.0).astype(np.float32)
    p1 = rng.uniform(-1, 1, (B + 1, n, C1)).astype(np.float32)
    p2 = rng.uniform(-1, 1, (B + 1, m, C2)).astype(np.float32)
    t1, t2, tp1, tp2 = (torch.from_numpy(a).to(dev) for a in (x1, x2, p1, p2))
    d2 = ((x2.astype(np.float64)[:, None] - x1.astype(np.float64)[:, :, None]) ** 2).sum(-1)
    order = np.argsort(d2, axis=-1, kind="stable")[:B]
    dist64 = np.take_along_axis(d2[:B], order, -1)
    dist, idx = pkg.tf_interpolate.three_nn(t1[:B], t2[:B])
    assert np.array_equal(idx.cpu().numpy(), order)
    assert np.array_equal(dist.cpu().numpy().astype(np.float64), dist64)
    r = 1.0 / np.maximum(dist64, 1e-10)
    wgt = r / r.sum(-1, keepdims=True)
    interp = (p2.astype(np.float64)[np.arange(B)[:, None, None], order] * wgt[..., None]).sum(2)
    ref = np.concatenate([interp, p1[:B].astype(np.float64)], -1)
    got = pkg.pointnet_util.fp_interpolate(t1[:B], t2[:B], tp1[:B], tp2[:B]).cpu().numpy()
    np.testing.assert_allclose(got, ref, **TOL)
    np.testing.assert_allclose(got, O.fp_fused(x1[:B], x2[:B], p1[:B], p2[:B]), **TOL)
    with pytest.raises(pkg.InvalidArgumentError):
        pkg.tf_interpolate.three_nn(t1, t2)
    with pytest.raises(pkg.InvalidArgumentError):
        pkg.pointnet_util.fp_interpolate(t1, t2, tp1, tp2)


def test_ball_group_layers_element_bound(env):
    """pn2_ball_group_layers divides a workgroup's E = qpb * nsample * Cout tile elements by
    Cout. At nsample = 128 (its maximum) one query per workgroup, points only: Cout = 5792 is
    accepted and bit-equal to the oracle's ball query + group, Cout = 5793 is rejected."""
    pkg, O, torch, dev = env
    B, N, M, ns, C, radius = 2, 4, 2, 128, 5792, 0.5
    assert ns * C * C < LIM <= ns * (C + 1) * (C + 1)
    assert ns * C * 4 > 32 * 1024  # one query already exceeds the tile: qpb = 1
    rng = np.random.default_rng(C)
    xyz = rng.random((B, N, 3)).astype(np.float32)
    new_xyz = xyz[:, :M] + np.float32(0.125)
    pts = rng.uniform(-1, 1, (B, N, C + 1)).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    (idx, cnt, out), = pkg.pointnet_util.ball_group_layers(
        [(radius, ns, t(xyz), t(pts[..., :C]), t(new_xyz))], use_xyz=False)
    ridx, rcnt = O.ball_query(xyz, new_xyz, radius, ns)
    assert len(np.unique(rcnt)) > 1
    assert np.array_equal(idx.cpu().numpy(), ridx) and np.array_equal(cnt.cpu().numpy(), rcnt)
    assert _same_bits(out.cpu().numpy(), O.group_point(pts[..., :C], ridx))
    with pytest.raises(pkg.InvalidArgumentError):
        pkg.pointnet_util.ball_group_layers([(radius, ns, t(xyz), t(pts), t(new_xyz))],
                                            use_xyz=False)


def test_ball_group_grid_element_bound(env):
    """The grid grouping kernel divides a query's nsample * Cout elements by Cout = C + 3. At
    C = 4096 (its maximum): nsample = 255 accepted and bit-equal to the oracle, 256 rejected."""
    pkg, O, torch, dev = env
    B, N, M, ns, C, radius = 2, 40, 3, 255, 4096, 0.4
    cout = C + 3
    assert ns * cout * cout < LIM <= (ns + 1) * cout * cout
    rng = np.random.default_rng(cout)
    xyz = rng.random((B, N, 3)).astype(np.float32)
    new_xyz = np.ascontiguousarray(xyz[:, :M]) + np.float32(0.0625)
    pts = rng.uniform(-1, 1, (B, N, C)).astype(np.float32)
    tx, tp, tn = (torch.from_numpy(a).to(dev) for a in (xyz, pts, new_xyz))
    grid = pkg.tf_grouping.BallGrid(tx, radius)
    ridx, rcnt = O.ball_query(xyz, new_xyz, radius, ns)
    assert len(np.unique(rcnt)) > 1
    for xyz_last in (False, True):
        idx, cnt, out = pkg.pointnet_util.ball_group(radius, ns, tx, tp, tn, grid, xyz_last=xyz_last)
        assert np.array_equal(idx.cpu().numpy(), ridx) and np.array_equal(cnt.cpu().numpy(), rcnt)
        ref, _ = O.group_concat(xyz, pts, new_xyz, ridx, use_xyz=True, xyz_last=xyz_last)
        assert _same_bits(out.cpu().numpy(), ref)
    with pytest.raises(pkg.InvalidArgumentError):
        pkg.pointnet_util.ball_group(radius, ns + 1, tx, tp, tn, grid)


def test_fp_column_bound(env):
    """The FP kernels divide a workgroup's 64 rows x cw column elements by cw. With m > 2048
    known points the search variant does not split the channels, and C2 = 1 keeps the columns
    scalar, so cw = C2 + C1: 8191 columns are accepted (pn2_fp_fused and pn2_fp_grid_fused,
    against the oracle; the concat is a copy), 8192 are rejected by both."""
    pkg, O, torch, dev = env
    B, n, m, C2, C1 = 2, 1, 2049, 1, 8190
    cw = C2 + C1
    assert 64 * cw * cw < LIM <= 64 * (cw + 1) * (cw + 1) and 2 * m > 4096 and C2 % 4 != 0
    rng = np.random.default_rng(cw)
    x1 = rng.random((B, n, 3)).astype(np.float32)
    x2 = rng.random((B, m, 3)).astype(np.float32)
    p1 = rng.uniform(-1, 1, (B, n, C1 + 1)).astype(np.float32)
    p2 = rng.uniform(-1, 1, (B, m, C2)).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    t1, t2, tp1, tp1big, tp2 = t(x1), t(x2), t(p1[..., :C1]), t(p1), t(p2)
    ref = O.fp_fused(x1, x2, p1[..., :C1], p2)
    got = pkg.pointnet_util.fp_interpolate(t1, t2, tp1, tp2).cpu().numpy()
    np.testing.assert_allclose(got, ref, **TOL)
    assert _same_bits(got[..., C2:], p1[..., :C1])
    with pytest.raises(pkg.InvalidArgumentError):
        pkg.pointnet_util.fp_interpolate(t1, t2, tp1big, tp2)
    # the one-launch grid variant (C ABI: the wrapper takes it only for large searches)
    L, st = pkg.lib(), torch.cuda.current_stream(dev).cuda_stream
    out = torch.full((B, n, cw), float("nan"), device=dev)
    rc = L.pn2_fp_grid_fused(t1.data_ptr(), t2.data_ptr(), None, tp1.data_ptr(), C1,
                             tp2.data_ptr(), C2, B, n, m, out.data_ptr(), None, None, st)
    assert rc == 0
    np.testing.assert_allclose(out.cpu().numpy(), ref, **TOL)
    assert _same_bits(out.cpu().numpy()[..., C2:], p1[..., :C1])
    big = torch.empty((B, n, cw + 1), device=dev)
    rc = L.pn2_fp_grid_fused(t1.data_ptr(), t2.data_ptr(), None, tp1big.data_ptr(), C1 + 1,
                             tp2.data_ptr(), C2, B, n, m, big.data_ptr(), None, None, st)
    assert rc == -22  # PN2_EINVAL


# ------------------------------------------------------------------ attention numerics

def _attention_np(Q, K, V, dtype):
    """The same formula in plain numpy at `dtype` (max subtracted, as any softmax must)."""
    B, M, ns, C = K.shape
    H = C // 4
    q = Q.astype(dtype).reshape(B, M, H, 1, 4)
    k = K.astype(dtype).reshape(B, M, H, ns, 4)
    v = V.astype(dtype).reshape(B, M, H, ns, 4)
    s = (q * k).sum(-1) / dtype(2)
    e = np.exp(s - s.max(-1, keepdims=True))
    return ((e / e.sum(-1, keepdims=True))[..., None] * v).sum(-2).reshape(B, M, C)


@pytest.mark.parametrize("ns", [8, 20, 128])
def test_attention_large_logits(env, ns):
    """Integer Q and K in [-10, 10]: the logits q.k / 2 are exact in fp32 and span +-200 within
    a head (recorded span: +-200, not lowered), far past where exp overflows without the max
    subtraction; neighbouring heads of one wave have very different maxima, so a reduction over
    the wrong segment width leaks one head's max into another. ns = 8 and 128 take the
    specialised kernel, 20 the generic one, and each runs the grad kernel. A plain fp32 numpy
    evaluation is checked to be within the 1e-5 target of float64 first."""
    pkg, O, torch, dev = env
    B, M, C = 2, 37, 32
    rng = np.random.default_rng(200 + ns)
    Q = rng.integers(-10, 11, (B, M, C)).astype(np.float32)
    K = rng.integers(-10, 11, (B, M, ns, C)).astype(np.float32)
    K[:, :, 0, :4], Q[:, :, :4] = 10.0, 10.0     # head 0's first pseudo-key: logit +200 ...
    K[:, :, 0, 4:8] = -10.0                      # ... and its second (the next 4 floats): -200
    V = rng.uniform(-1, 1, (B, M, ns, C)).astype(np.float32)
    G = rng.uniform(-1, 1, (B, M, C)).astype(np.float32)
    logits = (Q.reshape(B, M, C // 4, 1, 4) * K.reshape(B, M, C // 4, ns, 4)).sum(-1) / 2
    assert logits.max() == 200 and logits.min() == -200
    ref = _attention_f64(Q, K, V)
    np.testing.assert_allclose(_attention_np(Q, K, V, np.float32),
                               _attention_np(Q, K, V, np.float64), **TOL)
    np.testing.assert_allclose(_attention_np(Q, K, V, np.float64), ref, rtol=1e-12, atol=1e-12)
    got = pkg.attention_layer.attention_reduce(*(torch.from_numpy(a).to(dev) for a in (Q, K, V)))
    np.testing.assert_allclose(got.cpu().numpy(), ref, **TOL)
    grads = _attention_grad_capi(env, Q, K, V, G)
    for name, g, r in zip(("dQ", "dK", "dV"), grads, _attention_grads_f64(Q, K, V, G)):
        np.testing.assert_allclose(g, r, err_msg=name, **TOL)
