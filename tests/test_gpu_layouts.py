"""The ops on misaligned, offset and strided inputs.

torch's allocator hands out 512-byte aligned, contiguous tensors, and every other GPU test
passes those. The library chooses between 16-byte vector and per-float code paths at run time
from the pointers it is given; this file runs the other side of each choice:

  * a contiguous view that starts 4, 8 or 12 bytes into an allocation (`offset_view`), for
    inputs and, through the C ABI, for caller-owned outputs;
  * the second cloud of a batch whose clouds are not a multiple of 16 bytes long;
  * non-contiguous views (channel slices, transposes, stride-0 batches, step slices).

Each case first asserts, in plain integers mirrored from the launcher, that it is on the side
of the predicate it is meant for (a case edited later fails there instead of silently losing
its branch). Expected values come from the oracle / the float64 references of the suite, and
every case also asserts that the misaligned or strided call returns the bits of the same op on
an aligned contiguous clone: the two branches of each kernel issue the same arithmetic in the
same order, only the width of the memory access differs.
"""
import importlib

import numpy as np
import pytest

import mlp_train_ref as R
from conftest import PKG_NAME
from mlp_ref import fused, make_layers, mlp_f32
from support import assert_close, on_gpu, same_bits

TOL = dict(rtol=1e-5, atol=1e-5)  # the README's bound for the floating-point attention kernels


@pytest.fixture(scope="module")
def env():
    import torch

    import pn2hip
    from oracle import oracle as O
    O.set_threads(16)
    pkg = importlib.import_module(PKG_NAME)
    return pkg, O, torch, torch.device("cuda:0"), pn2hip.ops


# ------------------------------------------------------------------------------- helpers
def offset_view(t, k):
    """A contiguous copy of t that starts k elements into a fresh (aligned) flat buffer."""
    import torch
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    view = buf[k:k + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous()
    assert view.data_ptr() % 16 == (k * t.element_size()) % 16
    return view


def res(t):
    """The pointer's residue modulo 16 (None: an absent tensor counts as aligned)."""
    return 0 if t is None else t.data_ptr() % 16


def stream(torch, dev):
    return torch.cuda.current_stream(dev).cuda_stream


def tdev(torch, dev, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# =============================================================================== 1. sampler
# fps_cull.h: the culled SA1 sampler copies its cloud (P = inp + b*N*3) into LDS with float4
# loads when P is 16-byte aligned, dwords otherwise.
SAMPLER = [
    # (N, offset in floats, schedule, residues of the two clouds)
    (4100, 1, 0, (4, 4)),
    (4100, 2, 0, (8, 8)),
    (4099, 0, 0, (0, 4)),   # cloud 0 aligned, cloud 1 not: both branches in one launch
    (4099, 0, 1, (0, 4)),   # PN2_FPS_BLOCKSCAN: the schedule with no vector path
]


@pytest.fixture(scope="module")
def sampler_ref(env):
    pkg, O = env[0], env[1]
    out = {}
    for N in (4100, 4099):
        x = pkg.synth.batch([0, 1], N, "scannet")[0]
        idx = O.fps(x, 64)
        out[N] = (x, idx, O.gather_point(x, idx))
    return out


@on_gpu
@pytest.mark.parametrize("N,k,sched,want", SAMPLER)
def test_sampler_on_misaligned_clouds(env, sampler_ref, N, k, sched, want):
    pkg, O, torch, dev, ops = env
    B, M = 2, 64
    x_np, ref_idx, ref_xyz = sampler_ref[N]
    x = tdev(torch, dev, x_np)
    assert res(x) == 0
    v = offset_view(x, k) if k else x
    assert 4096 < N <= 8192  # the culled sampler with its cloud in LDS (fps.hip fps_impl)
    assert tuple((v.data_ptr() + b * N * 12) % 16 for b in range(B)) == want
    if sched == 0:
        got_idx = pkg.tf_sampling.farthest_point_sample(M, v)
        got_idx2, got_xyz = pkg.tf_sampling.farthest_point_sample_and_gather(M, v)
        same_bits(got_idx, got_idx2, "sample vs sample_and_gather")
    else:
        assert sched == pkg._lib.PN2_FPS_BLOCKSCAN
        got_idx = torch.empty((B, M), dtype=torch.int32, device=dev)
        got_xyz = torch.empty((B, M, 3), dtype=torch.float32, device=dev)
        rc = pkg.lib().pn2_fps_gather_sched(v.data_ptr(), B, N, M, got_idx.data_ptr(),
                                            got_xyz.data_ptr(), sched, stream(torch, dev))
        assert rc == 0
    torch.cuda.synchronize()
    assert pkg.lib().pn2_fault_status(1) == 0
    assert np.array_equal(got_idx.cpu().numpy(), ref_idx)
    same_bits(got_xyz, ref_xyz, "new_xyz")
    if k:  # the aligned clone
        a_idx, a_xyz = pkg.tf_sampling.farthest_point_sample_and_gather(M, x)
        same_bits(got_idx, a_idx, "idx vs aligned")
        same_bits(got_xyz, a_xyz, "new_xyz vs aligned")


# ===================================================================== 2. FP interpolation
# interp.hip fp_plan: v2 = C2 % 4 == 0 and points2, out 16-byte aligned; v1 = 4 / 2 / 1 from
# C1 and the 16- / 8-byte alignment of points1 (1 whenever !v2).
def fp_variant(C1, C2, r1, r2, rout):
    v2 = C2 % 4 == 0 and r2 == 0 and rout == 0
    v1 = 1 if not v2 else 4 if C1 % 4 == 0 and r1 == 0 else 2 if C1 % 2 == 0 and r1 % 8 == 0 else 1
    return int(v2), v1


FP = [
    # (C1, C2, k1, k2, kout, (v2, v1))
    (0, 8, 0, 1, 0, (0, 1)),
    (8, 8, 2, 0, 0, (1, 2)),
    (8, 8, 1, 0, 0, (1, 1)),
    (6, 8, 0, 0, 0, (1, 2)),
    (6, 8, 1, 0, 0, (1, 1)),
    (8, 8, 0, 0, 1, (0, 1)),   # a caller-owned output: through the C ABI
    (5, 7, 0, 0, 0, (0, 1)),   # all scalar
    (8, 8, 0, 0, 0, (1, 4)),   # the aligned variant, for the same-bits comparison's other side
]
FP_B, FP_N, FP_M = 2, 70, 9


@pytest.fixture(scope="module")
def fp_ref(env):
    pkg, O = env[0], env[1]
    rng = np.random.default_rng(11)
    x1 = pkg.synth.batch([3, 4], FP_N, "scannet")[0]
    x2 = np.ascontiguousarray(x1[:, rng.choice(FP_N, FP_M, replace=False)])
    dist, idx = O.three_nn(x1, x2)
    out = {"x1": x1, "x2": x2, "dist": dist, "idx": idx}
    for C1, C2 in sorted({(c[0], c[1]) for c in FP}):
        p1 = rng.uniform(-1, 1, (FP_B, FP_N, C1)).astype(np.float32) if C1 else None
        p2 = rng.uniform(-1, 1, (FP_B, FP_M, C2)).astype(np.float32)
        g = rng.uniform(-1, 1, (FP_B, FP_N, C1 + C2)).astype(np.float32)
        out[C1, C2] = (p1, p2, g, O.fp_fused(x1, x2, p1, p2))
    return out


def fp_fused_c(pkg, torch, dev, x1, x2, p1, p2, out):
    C1 = 0 if p1 is None else int(p1.shape[2])
    rc = pkg.lib().pn2_fp_fused(x1.data_ptr(), x2.data_ptr(), None if p1 is None else p1.data_ptr(),
                                C1, p2.data_ptr(), int(p2.shape[2]), FP_B, FP_N, FP_M,
                                out.data_ptr(), stream(torch, dev))
    assert rc == 0
    torch.cuda.synchronize()
    return out


@on_gpu
@pytest.mark.parametrize("C1,C2,k1,k2,kout,want", FP)
def test_fp_interpolation_variants(env, fp_ref, C1, C2, k1, k2, kout, want):
    pkg, O, torch, dev, ops = env
    p1_np, p2_np, g_np, ref = fp_ref[C1, C2]
    T = lambda a: tdev(torch, dev, a)  # noqa: E731
    x1, x2, dist, idx = (T(fp_ref[k]) for k in ("x1", "x2", "dist", "idx"))
    p1a, p2a = T(p1_np), T(p2_np)
    p1 = offset_view(p1a, k1) if k1 else p1a
    p2 = offset_view(p2a, k2) if k2 else p2a
    empty = lambda: torch.full((FP_B, FP_N, C1 + C2), float("nan"), device=dev)  # noqa: E731
    out = offset_view(empty(), kout) if kout else empty()
    assert res(p1a) == 0 and res(p2a) == 0
    assert fp_variant(C1, C2, res(p1), res(p2), res(out)) == want
    # pn2_fp_fused (the search inside the kernel)
    got = fp_fused_c(pkg, torch, dev, x1, x2, p1, p2, out)
    same_bits(got, ref, "pn2_fp_fused vs oracle")
    aligned = fp_fused_c(pkg, torch, dev, x1, x2, p1a, p2a, empty())
    same_bits(got, aligned, "pn2_fp_fused vs aligned")
    if kout:
        return  # (the wrappers below allocate their own, aligned, output)
    # pn2_fp_apply (precomputed neighbours): its own allocation is aligned, so the variant is
    # the one asserted above
    got = pkg.pointnet_util.fp_apply((dist, idx), p1, p2)
    same_bits(got, ref, "fp_apply vs oracle")
    same_bits(got, pkg.pointnet_util.fp_apply((dist, idx), p1a, p2a), "fp_apply vs aligned")
    # fp_apply_train and its gradient (an offset grad_out too)
    leaves = [None if p1 is None else p1.detach().requires_grad_(True),
              p2.detach().requires_grad_(True)]
    o = ops.fp_apply_train(dist, idx, leaves[0], leaves[1])
    same_bits(o, ref, "fp_apply_train vs oracle")
    g = offset_view(T(g_np), 1)
    o.backward(g)
    g2a, g1a = ops.fp_apply_train_grad(T(g_np), dist, idx, FP_M, C2, C1)
    same_bits(leaves[1].grad, g2a, "grad_points2 vs aligned")
    w64 = O.idw_weights(fp_ref["dist"]).astype(np.float64)
    ref64 = np.zeros((FP_B, FP_M, C2))
    for b in range(FP_B):
        for j in range(FP_N):
            for t in range(3):
                ref64[b, fp_ref["idx"][b, j, t]] += w64[b, j, t] * g_np[b, j, :C2].astype(np.float64)
    ref32 = O.three_interpolate_grad(FP_M, fp_ref["idx"], O.idw_weights(fp_ref["dist"]),
                                     np.ascontiguousarray(g_np[:, :, :C2]))
    assert_close(leaves[1].grad.cpu().numpy(), ref64, ref32, "grad_points2")
    if C1:
        same_bits(leaves[0].grad, g_np[:, :, C2:], "grad_points1")
        same_bits(g1a, g_np[:, :, C2:], "grad_points1 (op)")


# ========================================================================= 3. fused grouping
# sa_group.hip: g.vec = features and C % 4 == 0 and ns % 4 == 0 and no grouped_xyz output and
# 4 * Cout <= kSgVecFloats and points, new_points 16-byte aligned.
K_SG_VEC_FLOATS = 4096
SG_B, SG_N, SG_M, SG_C, SG_R = 2, 256, 16, 8, 0.4
SG = [
    # (ns, k_points, k_new_points, vec)
    (8, 0, 0, True),
    (8, 1, 0, False),
    (8, 0, 1, False),   # a caller-owned output: through the C ABI
    (6, 0, 0, False),   # scalar by ns % 4
]


def sg_vec(C, ns, Cout, r_points, r_out):
    return C % 4 == 0 and ns % 4 == 0 and 4 * Cout <= K_SG_VEC_FLOATS and r_points == 0 and r_out == 0


@pytest.fixture(scope="module")
def sg_ref(env):
    pkg, O = env[0], env[1]
    xyz = pkg.synth.batch([5, 6], SG_N, "scannet")[0]
    pts = np.random.default_rng(5).uniform(-1, 1, (SG_B, SG_N, SG_C)).astype(np.float32)
    new_xyz = O.gather_point(xyz, O.fps(xyz, SG_M))
    out = {"xyz": xyz, "points": pts, "new_xyz": new_xyz}
    for ns in (8, 6):
        idx, cnt = O.ball_query(xyz, new_xyz, SG_R, ns)
        out[ns] = (idx, cnt, O.group_concat(xyz, pts, new_xyz, idx)[0])
    return out


def ball_group_layers_c(pkg, torch, dev, xyz, points, new_xyz, ns, new_points):
    L = pkg._lib
    idx = torch.empty((SG_B, SG_M, ns), dtype=torch.int32, device=dev)
    cnt = torch.empty((SG_B, SG_M), dtype=torch.int32, device=dev)
    arr = (L.SaLayer * 1)()
    a = arr[0]
    a.xyz, a.points, a.new_xyz = xyz.data_ptr(), points.data_ptr(), new_xyz.data_ptr()
    a.N, a.C, a.M, a.nsample, a.radius, a.flags = SG_N, SG_C, SG_M, ns, SG_R, L.PN2_USE_XYZ
    a.idx, a.pts_cnt, a.grouped_xyz, a.new_points = (idx.data_ptr(), cnt.data_ptr(), None,
                                                     new_points.data_ptr())
    assert pkg.lib().pn2_ball_group_layers(arr, 1, SG_B, stream(torch, dev)) == 0
    torch.cuda.synchronize()
    return idx, cnt, new_points


@on_gpu
@pytest.mark.parametrize("ns,kp,ko,vec", SG)
def test_fused_grouping_write_phases(env, sg_ref, ns, kp, ko, vec):
    pkg, O, torch, dev, ops = env
    T = lambda a: tdev(torch, dev, a)  # noqa: E731
    xyz, pa, new_xyz = T(sg_ref["xyz"]), T(sg_ref["points"]), T(sg_ref["new_xyz"])
    ref_idx, ref_cnt, ref_np = sg_ref[ns]
    assert ref_cnt.min() >= 1 and (ref_cnt < ns).any() and (ref_cnt == ns).any()
    p = offset_view(pa, kp) if kp else pa
    Cout = SG_C + 3
    empty = lambda: torch.full((SG_B, SG_M, ns, Cout), float("nan"), device=dev)  # noqa: E731
    out = offset_view(empty(), ko) if ko else empty()
    assert res(pa) == 0
    assert sg_vec(SG_C, ns, Cout, res(p), res(out)) == vec
    idx, cnt, got = ball_group_layers_c(pkg, torch, dev, xyz, p, new_xyz, ns, out)
    assert np.array_equal(idx.cpu().numpy(), ref_idx) and np.array_equal(cnt.cpu().numpy(), ref_cnt)
    same_bits(got, ref_np, "pn2_ball_group_layers vs oracle")
    same_bits(got, ball_group_layers_c(pkg, torch, dev, xyz, pa, new_xyz, ns, empty())[2],
              "vs aligned")
    if ko:
        return
    # pointnet_util's layer path (its own, aligned, output)
    (i2, c2, np2), = pkg.pointnet_util.ball_group_layers([(SG_R, ns, xyz, p, new_xyz)])
    assert np.array_equal(i2.cpu().numpy(), ref_idx)
    same_bits(np2, ref_np, "ball_group_layers vs oracle")
    # pn2_ball_group_grid: the grid kernel writes the same rows from the same points pointer
    grid = pkg.tf_grouping.BallGrid(xyz, SG_R)
    i3, c3, np3 = pkg.pointnet_util.ball_group(SG_R, ns, xyz, p, new_xyz, grid)
    assert np.array_equal(i3.cpu().numpy(), ref_idx) and np.array_equal(c3.cpu().numpy(), ref_cnt)
    same_bits(np3, ref_np, "ball_group vs oracle")


# ============================================================================ 4. fused MLPs
# mlp.hip: a source segment is gathered as float4 only when its width is a multiple of 4 AND
# its pointer is 16-byte aligned (x; points; points2, and points1 with C2 % 4 == 0 as well);
# out_vec (float4 stores of the staged last layer) needs cout % 4 == 0 and an aligned out.
def seg_vec(width, r, extra=True):
    return width % 4 == 0 and r == 0 and extra


# (an offset out only where out_vec can be on: cout % 4 == 0)
SHARED = [(cin, widths, which) for cin in (8, 12, 9) for widths in ([32, 21], [32, 64])
          for which in ("x", "out") if which == "x" or widths[-1] % 4 == 0]


@on_gpu
@pytest.mark.parametrize("cin,widths,which", SHARED)
def test_shared_mlp_on_offset_buffers(env, cin, widths, which):
    pkg, O, torch, dev, ops = env
    rows, cout = 77, widths[-1]
    rng = np.random.default_rng(cin * 100 + cout)
    layers = make_layers(rng, cin, widths)
    x_np = rng.uniform(-1, 1, (rows, cin)).astype(np.float32)
    mlp = fused(pkg, layers)
    xa = tdev(torch, dev, x_np)
    x = offset_view(xa, 1) if which == "x" else xa
    empty = lambda: torch.full((rows, cout), float("nan"), device=dev)  # noqa: E731
    out = offset_view(empty(), 1) if which == "out" else empty()
    assert res(xa) == 0
    if which == "x":
        assert not seg_vec(cin, res(x)) and seg_vec(cin, res(xa)) == (cin % 4 == 0)
    else:
        # out_vec is off here. For the aligned call it is on only if choose_R_staged
        # (mlp.hip) stages the last layer through LDS, an occupancy decision over the device's
        # LDS budget that plain integers of the case cannot mirror: where it does not stage,
        # both calls store from registers and this sub-case only pins that an offset out works.
        assert cout % 4 == 0 and res(out) == 4
    tab, n = mlp.table()

    def run(xi, oi):
        assert pkg.lib().pn2_shared_mlp(xi.data_ptr(), rows, cin, n, tab, oi.data_ptr(),
                                        stream(torch, dev)) == 0
        torch.cuda.synchronize()
        return oi
    got = run(x, out)
    assert_close(got.cpu().numpy(), O.mlp_f64(x_np, layers), mlp_f32(x_np, layers), "shared_mlp")
    same_bits(got, run(xa, empty()), "shared_mlp vs aligned")
    if which == "x":  # the wrapper
        same_bits(mlp(x), got, "SharedMLP.__call__")


@on_gpu
@pytest.mark.parametrize("pooling", ["max", None])
def test_group_mlp_on_offset_points(env, sg_ref, pooling):
    pkg, O, torch, dev, ops = env
    T = lambda a: tdev(torch, dev, a)  # noqa: E731
    ns = 8
    idx_np, _, grouped = sg_ref[ns]
    gxyz = O.group_concat(sg_ref["xyz"], sg_ref["points"], sg_ref["new_xyz"], idx_np)[1]
    layers = make_layers(np.random.default_rng(3), SG_C + 3, [32, 64])
    pa = T(sg_ref["points"])
    p = offset_view(pa, 1)
    assert SG_C % 4 == 0 and res(pa) == 0 and not seg_vec(SG_C, res(p)) and seg_vec(SG_C, res(pa))
    args = (T(sg_ref["xyz"]), None, T(sg_ref["new_xyz"]), T(idx_np), fused(pkg, layers), pooling)
    run = lambda pts: pkg.pointnet_util.group_mlp(args[0], pts, *args[2:])  # noqa: E731
    got = run(p)
    y64, y32 = O.mlp_f64(grouped, layers), mlp_f32(grouped, layers)
    if pooling is not None:
        y64, y32 = O.pool_f64(y64, gxyz, pooling), O.pool_f64(y32, gxyz, pooling)
    assert_close(got.cpu().numpy(), y64, y32, f"group_mlp {pooling}")
    same_bits(got, run(pa), "group_mlp vs aligned")


@on_gpu
@pytest.mark.parametrize("add_max", [False, True])
def test_group_mlp_attention_on_offset_points(env, sg_ref, add_max):
    """pn2_group_mlp_attention shares group_mlp_impl's predicate: an offset `points` takes the
    per-float gather. Reference: float64 MLP of the oracle's grouping, the attention of
    tests/model_train_ref.py, the batch norm; rtol 1e-4 / atol 2e-5 as in
    tests/test_gpu_mlp.py test_fused_attention_matches_unfused."""
    pkg, O, torch, dev, ops = env
    import model_train_ref as MR
    al, tu = pkg.attention_layer, pkg.tf_util
    T = lambda a: tdev(torch, dev, a)  # noqa: E731
    ns, C = 8, 32
    idx_np, _, grouped = sg_ref[ns]
    layers = make_layers(np.random.default_rng(13), SG_C + 3, [C])
    store = tu.ParamStore(seed=5)
    g = np.random.default_rng(C)
    for k, (lo, hi) in {"moving_mean": (-.1, .1), "moving_variance": (.5, 2), "gamma": (.5, 1.5),
                        "beta": (-.2, .2)}.items():
        store[f"s/s/{k}"] = torch.from_numpy(g.uniform(lo, hi, C).astype(np.float32))
    for d in al._attention_scopes("s"):
        store[f"{d}/bias"] = torch.from_numpy(g.uniform(-.1, .1, C).astype(np.float32))
    pa = T(sg_ref["points"])
    p = offset_view(pa, 1)
    assert SG_C % 4 == 0 and res(pa) == 0 and not seg_vec(SG_C, res(p)) and seg_vec(SG_C, res(pa))
    run = lambda pts: al.group_mlp_attention(T(sg_ref["xyz"]), pts, T(sg_ref["new_xyz"]),  # noqa: E731
                                             T(idx_np), fused(pkg, layers), store, "s", add_max)
    got = run(p)
    same_bits(got, run(pa), "group_mlp_attention vs aligned")
    X = torch.from_numpy(O.mlp_f64(grouped, layers))
    w = []
    for d in al._attention_scopes("s"):
        v = store.dense(d, C, C)
        w += [v["weights"].detach().cpu().double(), v["biases"].detach().cpu().double()]
    scale, shift = (t.cpu().double() for t in tu.bn_affine(store, "s/s", C, dev))
    ref = MR.attention_core(X, *w) * scale + shift
    if add_max:
        ref = ref + X.max(dim=2).values
    np.testing.assert_allclose(got.cpu().numpy(), ref.numpy(), rtol=1e-4, atol=2e-5)


@on_gpu
@pytest.mark.parametrize("which", ["points1", "points2"])
def test_fp_module_on_offset_points(env, fp_ref, which):
    pkg, O, torch, dev, ops = env
    T = lambda a: tdev(torch, dev, a)  # noqa: E731
    C1, C2, widths = 4, 8, [32, 16]
    rng = np.random.default_rng(21)
    p1_np = rng.uniform(-1, 1, (FP_B, FP_N, C1)).astype(np.float32)
    p2_np = rng.uniform(-1, 1, (FP_B, FP_M, C2)).astype(np.float32)
    layers = make_layers(rng, C1 + C2, widths)
    store = pkg.tf_util.ParamStore()
    for i, L in enumerate(layers):
        s = f"fa/conv_{i}"
        store[f"{s}/weights"] = torch.from_numpy(L["weights"])
        store[f"{s}/biases"] = torch.from_numpy(L["biases"])
        for k in ("gamma", "beta", "moving_mean", "moving_variance"):
            store[f"{s}/bn/{k}"] = torch.from_numpy(L[k])
    p1a, p2a = T(p1_np), T(p2_np)
    p1 = offset_view(p1a, 1) if which == "points1" else p1a
    p2 = offset_view(p2a, 1) if which == "points2" else p2a
    assert res(p1a) == 0 and res(p2a) == 0
    vecA, vecB = seg_vec(C2, res(p2)), seg_vec(C1, res(p1), C2 % 4 == 0)
    assert (vecA, vecB) == ((True, False) if which == "points1" else (False, True))
    run = lambda a, b: pkg.pointnet_util.pointnet_fp_module(  # noqa: E731
        T(fp_ref["x1"]), T(fp_ref["x2"]), a, b, widths, False, None, "fa", params=store)
    got = run(p1, p2)
    x = O.fp_fused(fp_ref["x1"], fp_ref["x2"], p1_np, p2_np)
    assert_close(got.cpu().numpy(), O.mlp_f64(x, layers), mlp_f32(x, layers), "fp_mlp")
    same_bits(got, run(p1a, p2a), "fp_mlp vs aligned")


@on_gpu
@pytest.mark.parametrize("pool", [False, True])
def test_training_layers_on_offset_buffers(env, pool):
    """mlp_layer_train{,_pool} and their _grad ops with x and grad_out 4 bytes off: the rows
    kernel (linear_rows in csrc/torch_ops.cpp -> pn2_shared_mlp) takes its per-float gather."""
    pkg, O, torch, dev, ops = env
    if pool:
        groups, ns, cin, cout = 26, 5, 8, 32   # 130 rows
        p = R.pool_make_params(torch, groups, ns, cin, cout, True, seed=9)
    else:
        cin, cout = 8, 32
        p = R.make_params(torch, 130, cin, cout, True, seed=9)
    d = {k: v.to(dev) for k, v in p.items()}
    x, go = offset_view(d["x"], 1), offset_view(d["go"], 1)
    assert cin % 4 == 0 and res(d["x"]) == 0 and not seg_vec(cin, res(x)) and res(go) == 4
    fwd = ops.mlp_layer_train_pool if pool else ops.mlp_layer_train
    bwd = ops.mlp_layer_train_pool_grad if pool else ops.mlp_layer_train_grad
    tail = lambda xi: (xi, d["w"], d["b"], d["gamma"], d["beta"], R.EPS, True)  # noqa: E731
    got, want = fwd(*tail(x)), fwd(*tail(d["x"]))
    for a, b in zip(got, want):
        same_bits(a, b, "forward vs aligned")
    out, y, mean, var, *arg = got
    saved = lambda xi: (*arg, xi, d["w"], y, mean, var, d["gamma"], d["beta"], R.EPS, True, True)  # noqa: E731
    ggot, gwant = bwd(go, *saved(x)), bwd(d["go"], *saved(d["x"]))
    for a, b in zip(ggot, gwant):
        same_bits(a, b, "backward vs aligned")
    plain = ops.mlp_layer_train(*tail(d["x"]))[0]
    mask = (plain > 0).cpu()
    if pool:
        assert torch.equal(out, plain.max(dim=1).values)
        flat = dict(p, x=p["x"].reshape(-1, cin))
        f64, f32 = (R.ref_layer(torch, flat, dt, True)[0] for dt in (torch.float64, torch.float32))
        pooled = lambda z: z.reshape(groups, ns, cout).max(dim=1).values  # noqa: E731
        assert_close(out, pooled(f64[0]), pooled(f32[0]), "out")
        assert_close(y.reshape(-1, cout), f64[1], f32[1], "y")
        assert_close(mean, f64[2], f32[2], "mean")
        assert_close(var, f64[3], f32[3], "var")
        refs = {dt: R.pool_ref_grads(torch, p, dt, True, mask, arg[0].cpu())
                for dt in (torch.float64, torch.float32)}
    else:
        f64, f32 = (R.ref_layer(torch, p, dt, True)[0] for dt in (torch.float64, torch.float32))
        for i, name in enumerate(("out", "y", "mean", "var")):
            assert_close(got[i], f64[i], f32[i], name)
        refs = {dt: R.ref_grads(torch, p, dt, True, mask) for dt in (torch.float64, torch.float32)}
    r64, r32 = refs[torch.float64], refs[torch.float32]
    for g, k in zip(ggot, ("x", "w", "b", "gamma", "beta")):
        assert_close(g, r64[k], r32[k], "grad_" + k)


# ============================================================================ 5. row gathers
# scene.hip gather_rows_kernel / predict.hip map_back_rows_kernel: 16-byte units only when the
# row size and both pointers allow it, 4-byte units otherwise.
ROWS = [(rb, ks, kd) for rb in (12, 16, 32) for ks, kd in ((0, 0), (1, 0), (0, 1))]


def v16(row_bytes, r_src, r_dst):
    return row_bytes % 16 == 0 and r_src == 0 and r_dst == 0


@on_gpu
@pytest.mark.parametrize("row_bytes,ks,kd", ROWS)
def test_gather_rows_units(env, row_bytes, ks, kd):
    pkg, O, torch, dev, ops = env
    rng = np.random.default_rng(row_bytes + ks + 2 * kd)
    nsrc, n, w = 301, 257, row_bytes // 4
    src_np = rng.uniform(-1, 1, (nsrc, w)).astype(np.float32)
    idx_np = rng.integers(0, nsrc, n).astype(np.int32)
    idx_np[:2] = (0, nsrc - 1)
    src = tdev(torch, dev, src_np)
    dst = torch.full((n, w), float("nan"), device=dev)
    assert res(src) == 0 and res(dst) == 0
    if ks:
        src = offset_view(src, ks)
    if kd:
        dst = offset_view(dst, kd)
    assert v16(row_bytes, res(src), res(dst)) == (row_bytes % 16 == 0 and not ks and not kd)
    rc = pkg.lib().pn2_gather_rows(src.data_ptr(), nsrc, row_bytes, tdev(torch, dev, idx_np).data_ptr(),
                                   n, dst.data_ptr(), stream(torch, dev))
    assert rc == 0
    torch.cuda.synchronize()
    same_bits(dst, src_np[idx_np], "pn2_gather_rows")


def map_back_case(torch, dev, row_bytes, ks, kd):
    """keys that reach the first and last row of values, rows of another batch (left as they
    are) and empty keys (zeroed); the expected out by numpy indexing."""
    rng = np.random.default_rng(row_bytes * 7 + ks + 2 * kd)
    rows, n, w, row0 = 211, 307, row_bytes // 4, 1000
    values_np = rng.uniform(-1, 1, (rows, w)).astype(np.float32)
    win = rng.integers(-60, rows + 60, n)   # outside [0, rows): another batch's row
    win[:2] = (0, rows - 1)
    empty = rng.uniform(size=n) < 0.2
    empty[:2] = False
    keys_np = np.where(empty, 0, ((win + row0 + 1) << 8) | rng.integers(0, 21, n)).astype(np.int64)
    before = rng.uniform(-1, 1, (n, w)).astype(np.float32)
    want = before.copy()
    inside = ~empty & (win >= 0) & (win < rows)
    want[inside] = values_np[win[inside]]
    want[empty] = 0
    assert inside.sum() > 50 and (~inside & ~empty).sum() > 20 and empty.sum() > 20
    values = torch.from_numpy(values_np).to(dev)
    out = torch.from_numpy(before).to(dev)
    if ks:
        values = offset_view(values, ks)
    if kd:
        out = offset_view(out, kd)
    return values, row0, torch.from_numpy(keys_np).to(dev), out, want


def check_map_back(torch, dev, ops, row_bytes, ks, kd):
    values, row0, keys, out, want = map_back_case(torch, dev, row_bytes, ks, kd)
    assert v16(row_bytes, res(values), res(out)) == (row_bytes % 16 == 0 and not ks and not kd)
    ops.map_back_rows(values, row0, keys, out)
    same_bits(out, want, "map_back_rows")


@on_gpu
@pytest.mark.parametrize("row_bytes,ks,kd", ROWS)
def test_map_back_rows_units(env, row_bytes, ks, kd):
    pkg, O, torch, dev, ops = env
    check_map_back(torch, dev, ops, row_bytes, ks, kd)


@pytest.mark.parametrize("row_bytes,ks,kd", ROWS)
def test_map_back_rows_host_twin(row_bytes, ks, kd):
    """The same cases on CPU tensors (csrc/cpu_predict.cpp): runs anywhere."""
    import torch

    import pn2hip
    check_map_back(torch, "cpu", pn2hip.ops, row_bytes, ks, kd)


def test_in_place_arguments_reject_views_on_the_host():
    """keys and out are written in place: a non-contiguous one is rejected with a clear
    error, never copied to a temporary that the update would be lost in."""
    import torch

    import pn2hip
    ops = pn2hip.ops
    keys = torch.zeros(8, dtype=torch.int64)
    wide = torch.zeros(8, 2, dtype=torch.int64)
    mask, orig = torch.ones(4, dtype=torch.uint8), torch.arange(4, dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.scene_vote(None, mask, orig, 0, wide[:, 0])
    ops.scene_vote(None, mask, orig, 0, keys)
    out = torch.zeros(8, 6)
    with pytest.raises(ValueError, match="contiguous"):
        ops.map_back_rows(torch.ones(4, 3), 0, keys, out[:, :3])
    assert not wide.any() and not out.any()
    # strided values and masks are read through a contiguous copy
    vals = torch.arange(24, dtype=torch.float32).reshape(4, 6)
    got = torch.zeros(8, 3)
    ops.map_back_rows(vals[:, 3:], 0, keys, got)
    assert torch.equal(got[:4], vals[:, 3:]) and not got[4:].any()


# ================================== 6. ops behind an alignment-demanding C function (attention)
AT_B, AT_M, AT_NS, AT_C = 2, 5, 8, 8


@pytest.fixture(scope="module")
def attn_ref(env):
    O = env[1]
    rng = np.random.default_rng(8)
    Q = rng.uniform(-1, 1, (AT_B, AT_M, AT_C)).astype(np.float32)
    K = rng.uniform(-1, 1, (AT_B, AT_M, AT_NS, AT_C)).astype(np.float32)
    V = rng.uniform(-1, 1, (AT_B, AT_M, AT_NS, AT_C)).astype(np.float32)
    G = rng.uniform(-1, 1, (AT_B, AT_M, AT_C)).astype(np.float32)
    return Q, K, V, G, O.attn_reduce(Q, K, V)


def torch_attention(torch, Q, K, V):
    """attention_layer.py:35-42 in float64 (tests/test_gpu_parity.py _torch_attention)."""
    B, M, ns, C = K.shape
    q, k, v = Q.reshape(B, M, C // 4, 1, 4), K.reshape(B, M, C // 4, ns, 4), V.reshape(B, M, C // 4, ns, 4)
    return (torch.softmax(q @ k.transpose(-1, -2) / 2.0, dim=-1) @ v).reshape(B, M, C)


@on_gpu
@pytest.mark.parametrize("which", [0, 1, 2, 3])
@pytest.mark.parametrize("k", [1, 2])
def test_attention_accepts_misaligned_tensors(env, attn_ref, which, k):
    """pn2_attn_reduce{,_layers,_grad} return PN2_EINVAL for a misaligned pointer; both front
    ends copy such an argument to a fresh allocation, so the call returns and matches."""
    pkg, O, torch, dev, ops = env
    al = pkg.attention_layer
    *arrs, ref = attn_ref
    aligned = [tdev(torch, dev, a) for a in arrs]
    args = list(aligned)
    args[which] = offset_view(aligned[which], k)
    assert res(args[which]) == 4 * k and all(res(a) == 0 for a in aligned)
    Q, K, V, G = args
    if which < 3:
        got = al.attention_reduce(Q, K, V)
        np.testing.assert_allclose(got.cpu().numpy(), ref, **TOL)
        same_bits(got, al.attention_reduce(*aligned[:3]), "attn_reduce vs aligned")
        # two layers in one launch: the offset layer and an aligned one
        lay = al.attention_reduce_layers([(Q, K, V), tuple(aligned[:3])])
        same_bits(lay[0], got, "attention_reduce_layers[0]")
        same_bits(lay[1], got, "attention_reduce_layers[1]")
    grads = al.attention_reduce_grad(Q, K, V, G)
    for a, b in zip(grads, al.attention_reduce_grad(*aligned)):
        same_bits(a, b, "attn_reduce_grad vs aligned")
    rs = [torch.from_numpy(a).double().requires_grad_(True) for a in arrs[:3]]
    torch_attention(torch, *rs).backward(torch.from_numpy(arrs[3]).double())
    for g, r in zip(grads, rs):
        np.testing.assert_allclose(g.cpu().numpy(), r.grad.numpy(), **TOL)


@on_gpu
@pytest.mark.parametrize("which", ["x", "grad_att", "grad_pmax", "q", "kv", "arg",
                                   "wq", "bq", "wk", "bk", "wv", "bv"])
def test_attention_training_accepts_misaligned_tensors(env, which):
    """Every tensor argument of attn_kv_train and attn_kv_train_grad 4 bytes off in turn (the
    weights reach pn2_mlp_pack and the at::cat / .t() copies; q, kv and grad_att reach
    pn2_attn_kv_reduce_grad, which demands alignment, through a copy)."""
    pkg, O, torch, dev, ops = env
    import model_train_ref as MR
    g = torch.Generator().manual_seed(4)
    u = lambda *s: (torch.rand(*s, generator=g) * 2 - 1)  # noqa: E731
    C = AT_C
    x = u(AT_B, AT_M, AT_NS, C)
    weights = [u(C, C) * 0.5, u(C) * 0.1, u(C, C) * 0.5, u(C) * 0.1, u(C, C) * 0.5, u(C) * 0.1]
    ga, gp = u(AT_B, AT_M, C), u(AT_B, AT_M, C)
    D = lambda t: t.to(dev)  # noqa: E731
    xa, wd = D(x), [D(w) for w in weights]
    base = ops.attn_kv_train(xa, *wd, True)
    att, pmax, arg, q, kv = base
    named = {"x": xa, "grad_att": D(ga), "grad_pmax": D(gp), "q": q, "kv": kv, "arg": arg}
    wnames = ("wq", "bq", "wk", "bk", "wv", "bv")
    named.update(zip(wnames, wd))
    assert all(res(t) == 0 for t in named.values())
    a = dict(named)
    a[which] = offset_view(named[which], 1)
    assert res(a[which]) == 4
    if which == "x" or which in wnames:
        for s, t in zip(ops.attn_kv_train(a["x"], *[a[k] for k in wnames], True), base):
            same_bits(s, t, "attn_kv_train vs aligned")
    call = lambda n: ops.attn_kv_train_grad(n["grad_att"], n["grad_pmax"], n["arg"], n["x"],  # noqa: E731
                                            n["wq"], n["wk"], n["wv"], n["q"], n["kv"], True)
    got = call(a)
    for s, t in zip(got, call(named)):
        same_bits(s, t, "attn_kv_train_grad vs aligned")
    f64 = MR.attention_core(x.double(), *[w.double() for w in weights])
    f32 = MR.attention_core(x, *weights)
    assert_close(att.cpu().numpy(), f64.numpy(), f32.numpy(), "att")
    same_bits(pmax, x.max(dim=2).values, "pmax")
    r64 = MR.attention_op_grads(x, weights, ga, gp, arg, torch.float64)
    r32 = MR.attention_op_grads(x, weights, ga, gp, arg, torch.float32)
    for s, t64, t32, name in zip(got, r64, r32, ("x", "wq", "bq", "wk", "bk", "wv", "bv")):
        assert_close(s.cpu().numpy(), t64.numpy(), t32.numpy(), "grad_" + name)


# ========================================================================= 7. strided inputs
def layouts(torch, t):
    """Non-contiguous views with t's shape: (a) a channel slice of a wider tensor, (b) a
    transposed view, (c) a stride-0 batch, (d) a step slice -- whichever t's shape allows. The
    values are t's, except for (c), whose batch entries are all t[0]."""
    out = {}
    if t.dim() >= 2:
        wide = torch.zeros(t.shape[:-1] + (t.shape[-1] + 3,), dtype=t.dtype, device=t.device)
        wide[..., 3:] = t
        out["slice"] = wide[..., 3:]
        out["transpose"] = t.transpose(-1, -2).contiguous().transpose(-1, -2)
        wide2 = torch.zeros((t.shape[0], 2 * t.shape[1]) + t.shape[2:], dtype=t.dtype, device=t.device)
        wide2[:, ::2] = t
        out["step"] = wide2[:, ::2]
    if t.shape[0] > 1:
        out["expand"] = t[:1].expand(t.shape)
    return {k: v for k, v in out.items() if not v.is_contiguous()}


def as_tuple(x):
    return tuple(x) if isinstance(x, (tuple, list)) else (x,)


def strided_sweep(torch, dev, call, args_np, ref=None, exact=True, skip=(), atomic=False,
                  ref_expand=True):
    """call(*tensors) with each tensor argument in turn in each layout: the outputs equal those
    of the contiguous clone bit for bit, and the reference `ref(*numpy args)` (bit for bit, or
    within TOL when not `exact`). atomic: the kernel sums with float atomics (the reference's
    gradient kernels, tf_sampling_g.cu / tf_grouping_g.cu / tf_interpolate.cpp), so two runs
    of it need not agree in the last bit: the clone comparison is within TOL too.
    exact="f32": `ref` returns (float64, float32) pairs, compared by assert_close (the training
    layers' tolerance). A None in ref's result skips that output. ref_expand=False: no
    reference for the stride-0 batch (arguments saved by a forward no longer belong together
    once one of them has its batch entries replaced)."""
    base = [tdev(torch, dev, a) if isinstance(a, np.ndarray) else a for a in args_np]
    ran = 0
    for i, t in enumerate(base):
        if not hasattr(t, "dim") or i in skip:
            continue
        for name, view in layouts(torch, t).items():
            clone = view.contiguous()
            assert not view.is_contiguous() and clone.is_contiguous() and res(clone) == 0
            a_v, a_c = list(base), list(base)
            a_v[i], a_c[i] = view, clone
            got, want = as_tuple(call(*a_v)), as_tuple(call(*a_c))
            for g, w in zip(got, want):
                if atomic:
                    np.testing.assert_allclose(g.cpu().numpy(), w.cpu().numpy(), **TOL)
                else:
                    same_bits(g, w, f"arg {i} as {name}")
            if ref is not None and (ref_expand or name != "expand"):
                r = ref(*[a.cpu().numpy() if hasattr(a, "cpu") else a for a in a_c])
                r = r if isinstance(r, list) else as_tuple(r)
                for g, w in zip(got, r):
                    if w is None:
                        continue
                    if exact == "f32":
                        assert_close(g.cpu().numpy(), w[0], w[1], f"arg {i} as {name}")
                    elif exact:
                        same_bits(g, w, f"arg {i} as {name} vs reference")
                    else:
                        np.testing.assert_allclose(g.cpu().numpy(), w, **TOL)
            ran += 1
    assert ran > 0
    return ran


def O_fp_apply(O):
    """fp_apply by the oracle's separate ops: IDW weights, three_interpolate, concat."""
    return lambda d, i, a, b: np.concatenate([O.three_interpolate(b, i, O.idw_weights(d)), a], -1)


def small(env):
    pkg, O = env[0], env[1]
    rng = np.random.default_rng(2)
    B, N, M, ns, C = 2, 96, 12, 8, 8
    xyz = pkg.synth.batch([7, 8], N, "scannet")[0]
    new_xyz = O.gather_point(xyz, O.fps(xyz, M))
    idx, _ = O.ball_query(xyz, new_xyz, 0.5, ns)
    pts = rng.uniform(-1, 1, (B, N, C)).astype(np.float32)
    return dict(B=B, N=N, M=M, ns=ns, C=C, rng=rng, xyz=xyz, new_xyz=new_xyz, idx=idx, pts=pts,
                fidx=O.fps(xyz, M))


@on_gpu
def test_strided_sampling_ops(env):
    pkg, O, torch, dev, ops = env
    s, ts = small(env), env[0].tf_sampling
    M = s["M"]
    sw = lambda *a, **k: strided_sweep(torch, dev, *a, **k)  # noqa: E731
    sw(lambda x: ts.farthest_point_sample(M, x), [s["xyz"]], lambda x: O.fps(x, M))
    sw(lambda x: ts.farthest_point_sample_and_gather(M, x), [s["xyz"]],
       lambda x: (O.fps(x, M), O.gather_point(x, O.fps(x, M))))
    sw(ts.gather_point, [s["xyz"], s["fidx"]], O.gather_point)
    g = s["rng"].uniform(-1, 1, (s["B"], M, 3)).astype(np.float32)
    sw(ts.gather_point_grad, [s["xyz"], s["fidx"], g],
       lambda x, i, go: O.gather_point_grad(x.shape[1], i, go), exact=False, atomic=True)
    inp = s["rng"].uniform(0.1, 1, (s["B"], 40)).astype(np.float32)
    inpr = s["rng"].uniform(0, 1, (s["B"], 33)).astype(np.float32)
    sw(ts.prob_sample, [inp, inpr], O.prob_sample)


@on_gpu
def test_strided_grouping_ops(env):
    pkg, O, torch, dev, ops = env
    s, tg, pu = small(env), env[0].tf_grouping, env[0].pointnet_util
    ns = s["ns"]
    sw = lambda *a, **k: strided_sweep(torch, dev, *a, **k)  # noqa: E731
    sw(lambda a, b: tg.query_ball_point(0.5, ns, a, b), [s["xyz"], s["new_xyz"]],
       lambda a, b: O.ball_query(a, b, 0.5, ns))
    sw(tg.group_point, [s["pts"], s["idx"]], O.group_point)
    g = s["rng"].uniform(-1, 1, (s["B"], s["M"], ns, s["C"])).astype(np.float32)
    sw(tg.group_point_grad, [s["pts"], s["idx"], g],
       lambda p, i, go: O.group_point_grad(p.shape[1], i, go), exact=False, atomic=True)
    sw(lambda a, b: tg.knn_point(4, a, b), [s["xyz"], s["new_xyz"]],
       lambda a, b: O.knn_point(4, a, b), exact=False)
    dist = s["rng"].uniform(0, 1, (s["B"], s["M"], 20)).astype(np.float32)
    sw(lambda d: tg.select_top_k(4, d), [dist], lambda d: O.selection_sort(d, 4), exact=False)
    sw(lambda x, p, nx, i: pu.group_concat(x, p, nx, i), [s["xyz"], s["pts"], s["new_xyz"], s["idx"]],
       lambda x, p, nx, i: O.group_concat(x, p, nx, i))
    sw(lambda x, p, nx, i: ops.group_concat_train(x, p, nx, i, True, False),
       [s["xyz"], s["pts"], s["new_xyz"], s["idx"]], lambda x, p, nx, i: O.group_concat(x, p, nx, i)[0])
    gx = s["rng"].uniform(-0.3, 0.3, (s["B"], s["M"], ns, 3)).astype(np.float32)
    for mode in ("max", "avg", "weighted_avg", "max_and_avg"):
        sw(lambda x, gz: pu.group_pool(x, mode, gz), [g, gx],
           lambda x, gz: O.group_pool(x, gz, mode), exact=False)


@on_gpu
def test_strided_interpolation_ops(env):
    pkg, O, torch, dev, ops = env
    s, ti, pu = small(env), env[0].tf_interpolate, env[0].pointnet_util
    sw = lambda *a, **k: strided_sweep(torch, dev, *a, **k)  # noqa: E731
    x1, x2 = s["xyz"], s["new_xyz"]
    dist, idx = O.three_nn(x1, x2)
    w = O.idw_weights(dist)
    p2 = s["rng"].uniform(-1, 1, (s["B"], s["M"], s["C"])).astype(np.float32)
    sw(ti.three_nn, [x1, x2], O.three_nn)
    sw(ti.idw_weights, [dist], O.idw_weights)
    sw(ti.three_interpolate, [p2, idx, w], O.three_interpolate)
    g = s["rng"].uniform(-1, 1, (s["B"], s["N"], s["C"])).astype(np.float32)
    sw(ti.three_interpolate_grad, [p2, idx, w, g],
       lambda p, i, ww, go: O.three_interpolate_grad(p.shape[1], i, ww, go), exact=False, atomic=True)
    sw(ops.fp_fused, [x1, x2, s["pts"], p2], O.fp_fused)
    sw(lambda a, b, c, d: pu.fp_interpolate(a, b, c, d), [x1, x2, s["pts"], p2], O.fp_fused)
    sw(lambda d, i, a, b: pu.fp_apply((d, i), a, b), [dist, idx, s["pts"], p2], O_fp_apply(O))
    sw(ops.fp_apply_train, [dist, idx, s["pts"], p2], O_fp_apply(O))
    ga = s["rng"].uniform(-1, 1, (s["B"], s["N"], 2 * s["C"])).astype(np.float32)
    C = s["C"]
    sw(lambda go, d, i: ops.fp_apply_train_grad(go, d, i, s["M"], C, C), [ga, dist, idx],
       lambda go, d, i: (O.three_interpolate_grad(s["M"], i, O.idw_weights(d),
                                                  np.ascontiguousarray(go[:, :, :C])),
                         go[:, :, C:]), exact=False)


def pairs(torch, fn, *arrays):
    """[(float64, float32)] numpy pairs of fn's outputs on the arrays as CPU tensors."""
    outs = []
    for dt in (torch.float64, torch.float32):
        r = fn(*[None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(
            dt if a.dtype.kind == "f" else torch.int64) for a in arrays])
        outs.append([None if t is None else t.detach().numpy() for t in as_tuple(r)])
    return [None if a is None else (a, b) for a, b in zip(*outs)]


def attn_grads64(torch, Q, K, V, G):
    rs = [torch.from_numpy(a).double().requires_grad_(True) for a in (Q, K, V)]
    torch_attention(torch, *rs).backward(torch.from_numpy(G).double())
    return tuple(r.grad.numpy() for r in rs)


@on_gpu
def test_strided_attention_ops(env, attn_ref):
    pkg, O, torch, dev, ops = env
    import model_train_ref as MR
    al = pkg.attention_layer
    Q, K, V, G, _ = attn_ref
    sw = lambda *a, **k: strided_sweep(torch, dev, *a, **k)  # noqa: E731
    sw(al.attention_reduce, [Q, K, V], O.attn_reduce, exact=False)
    sw(al.attention_reduce_grad, [Q, K, V, G], lambda *a: attn_grads64(torch, *a), exact=False)
    sw(lambda q, k, v: al.attention_reduce_layers([(q, k, v)]), [Q, K, V], O.attn_reduce, exact=False)
    rng = np.random.default_rng(6)
    x = rng.uniform(-1, 1, (AT_B, AT_M, AT_NS, AT_C)).astype(np.float32)
    w = [rng.uniform(-0.5, 0.5, (AT_C, AT_C)).astype(np.float32) if i % 2 == 0
         else rng.uniform(-0.1, 0.1, AT_C).astype(np.float32) for i in range(6)]

    def fwd_ref(x, *w):   # (att, pmax, arg, q, kv): att, pmax and the query rows
        return pairs(torch, lambda X, wq, bq, *r: (MR.attention_core(X, wq, bq, *r),
                                                   X.max(dim=2).values, None,
                                                   X[:, :, 0] @ wq + bq, None), x, *w)
    sw(lambda *a: ops.attn_kv_train(*a, True), [x] + w, fwd_ref, exact="f32")
    # the gradient op on strided saved tensors
    T = lambda a: tdev(torch, dev, a)  # noqa: E731
    att, pmax, arg, q, kv = ops.attn_kv_train(T(x), *[T(a) for a in w], True)
    ga = rng.uniform(-1, 1, att.shape).astype(np.float32)
    gp = rng.uniform(-1, 1, att.shape).astype(np.float32)

    def bwd_ref(ga, gp, arg, x, wq, wk, wv, q, kv):
        t = torch.from_numpy
        ws = [t(wq), t(w[1]), t(wk), t(w[3]), t(wv), t(w[5])]
        r = [MR.attention_op_grads(t(x), ws, t(ga), t(gp), t(arg), dt)
             for dt in (torch.float64, torch.float32)]
        return [(a.numpy(), b.numpy()) for a, b in zip(*r)]
    sw(lambda ga, gp, arg, x, wq, wk, wv, q, kv: ops.attn_kv_train_grad(ga, gp, arg, x, wq, wk, wv,
                                                                       q, kv, True),
       [ga, gp, arg, x, w[0], w[2], w[4], q, kv], bwd_ref, exact="f32", ref_expand=False)


def layer_ref(torch, x, w, b, gamma, beta, pool=False):
    """mlp_train_ref.ref_layer on x (groups, ns, cin): (out, y, mean, var) pairs."""
    shape = x.shape[:-1] + (w.shape[1],)

    def fn(x, w, b, gamma, beta):
        p = {"x": x.reshape(-1, x.shape[-1]), "w": w, "b": b, "gamma": gamma, "beta": beta}
        out, y, mean, var = R.ref_layer(torch, p, x.dtype, True)[0]
        out = out.reshape(shape)
        return (out.max(dim=1).values if pool else out), y.reshape(shape), mean, var
    return pairs(torch, fn, x, w, b, gamma, beta)


@on_gpu
def test_strided_training_ops(env):
    pkg, O, torch, dev, ops = env
    import head_train_ref as HR
    from optim_cases import numpy_confusion, numpy_iou
    rng = np.random.default_rng(12)
    sw = lambda *a, **k: strided_sweep(torch, dev, *a, **k)  # noqa: E731
    T = lambda a: tdev(torch, dev, a)  # noqa: E731
    x = rng.uniform(-1, 1, (26, 5, 8)).astype(np.float32)
    w = rng.uniform(-0.4, 0.4, (8, 32)).astype(np.float32)
    b, gam, bet = (rng.uniform(0.5, 1.5, 32).astype(np.float32) for _ in range(3))
    sw(lambda *a: ops.mlp_layer_train(*a, 1e-3, True), [x, w, b, gam, bet],
       lambda *a: layer_ref(torch, *a), exact="f32")
    sw(lambda *a: ops.mlp_layer_train_pool(*a, 1e-3, True), [x, w, b, gam, bet],
       lambda *a: layer_ref(torch, *a, pool=True), exact="f32")   # (arg: the clone's bits)
    y = rng.uniform(-1, 1, (26, 5, 32)).astype(np.float32)

    def bn_ref(y, gamma, beta):
        def fn(y, gamma, beta):
            f = y.reshape(-1, y.shape[-1])
            mean, var = f.mean(dim=0), f.var(dim=0, unbiased=False)
            return torch.relu((y - mean) * (gamma / torch.sqrt(var + 1e-3)) + beta), mean, var
        return pairs(torch, fn, y, gamma, beta)
    sw(lambda *a: ops.bn_train(*a, 1e-3, True), [y, gam, bet], bn_ref, exact="f32")
    sw(lambda a: ops.dropout(a, 0.5, 1234), [y], lambda a: HR.dropout_ref(a, 0.5, 1234))
    logits = rng.uniform(-2, 2, (4, 30, 21)).astype(np.float32)
    labels = rng.integers(0, 21, (4, 30)).astype(np.int32)
    wts = rng.uniform(0.5, 2, (4, 30)).astype(np.float32)

    def xent_ref(z, lab, wt):   # (loss, lse, pred, num_present)
        def fn(z, lab, wt):
            loss, lse, _ = HR.xent_ref(torch, z.reshape(-1, 21), lab.reshape(-1), wt.reshape(-1),
                                       z.dtype)
            return loss, lse.reshape(lab.shape)
        return pairs(torch, fn, z, lab, wt) + [None, None]
    sw(ops.softmax_xent, [logits, labels, wts], xent_ref, exact="f32")

    def confusion(lab, pred):
        c = torch.zeros((21, 21), dtype=torch.int64, device=dev)
        n = torch.zeros(2, dtype=torch.int64, device=dev)
        ops.seg_confusion(lab, pred, c, n)
        return c, n
    pred = rng.integers(0, 21, (4, 30)).astype(np.int32)
    sw(confusion, [labels, pred], lambda a, b: numpy_confusion(a.reshape(-1), b.reshape(-1), 21))
    # mean_iou takes only a contiguous confusion (checked below); its values against numpy
    cm = confusion(T(labels), T(pred))[0]
    iou, per = ops.mean_iou(cm)
    want = numpy_iou(cm.cpu().numpy())
    assert np.float32(want[0]) == iou.cpu().numpy()   # (as tests/test_gpu_optim.py)
    assert np.array_equal(want[1].astype(np.float32), per.cpu().numpy())
    with pytest.raises(ValueError, match="contiguous"):
        ops.mean_iou(torch.zeros((21, 42), dtype=torch.int64, device=dev)[:, ::2])


@on_gpu
def test_strided_gradient_ops(env):
    """The *_grad ops with each saved tensor strided in turn (through autograd they only ever
    see a strided grad_out)."""
    pkg, O, torch, dev, ops = env
    import head_train_ref as HR
    rng = np.random.default_rng(14)
    sw = lambda *a, **k: strided_sweep(torch, dev, *a, ref_expand=False, **k)  # noqa: E731
    D = lambda d: {k: None if v is None else v.to(dev) for k, v in d.items()}  # noqa: E731
    both = (torch.float64, torch.float32)
    names = ("x", "w", "b", "gamma", "beta")
    # mlp_layer_train_grad
    p = R.make_params(torch, 130, 8, 32, True, seed=3)
    d = D(p)
    out, y, mean, var = ops.mlp_layer_train(d["x"], d["w"], d["b"], d["gamma"], d["beta"], R.EPS, True)
    r = [R.ref_grads(torch, p, dt, True, (out > 0).cpu()) for dt in both]
    ref = [(r[0][k].numpy(), r[1][k].numpy()) for k in names]
    sw(lambda go, x, w, y, m, v, g, bt: ops.mlp_layer_train_grad(go, x, w, y, m, v, g, bt, R.EPS,
                                                                 True, True),
       [d["go"], d["x"], d["w"], y, mean, var, d["gamma"], d["beta"]], lambda *a: ref, exact="f32")
    # mlp_layer_train_pool_grad
    p = R.pool_make_params(torch, 26, 5, 8, 32, True, seed=3)
    d = D(p)
    out, y, mean, var, arg = ops.mlp_layer_train_pool(d["x"], d["w"], d["b"], d["gamma"], d["beta"],
                                                      R.EPS, True)
    full = ops.mlp_layer_train(d["x"], d["w"], d["b"], d["gamma"], d["beta"], R.EPS, True)[0]
    r = [R.pool_ref_grads(torch, p, dt, True, (full > 0).cpu(), arg.cpu()) for dt in both]
    ref2 = [(r[0][k].numpy(), r[1][k].numpy()) for k in names]
    sw(lambda go, a, x, w, y, m, v, g, bt: ops.mlp_layer_train_pool_grad(go, a, x, w, y, m, v, g, bt,
                                                                         R.EPS, True, True),
       [d["go"], arg, d["x"], d["w"], y, mean, var, d["gamma"], d["beta"]], lambda *a: ref2,
       exact="f32")
    # bn_train_grad
    yb = torch.from_numpy(rng.uniform(-1, 1, (26, 5, 32)).astype(np.float32))
    gam = torch.from_numpy(rng.uniform(0.5, 1.5, 32).astype(np.float32))
    bet = torch.from_numpy(rng.uniform(-0.2, 0.2, 32).astype(np.float32))
    gob = torch.from_numpy(rng.uniform(-1, 1, (26, 5, 32)).astype(np.float32))
    o, mean, var = ops.bn_train(yb.to(dev), gam.to(dev), bet.to(dev), 1e-3, True)
    mask = (o > 0).cpu()
    r = []
    for dt in both:
        lv = [t.to(dt).clone().requires_grad_(True) for t in (yb, gam, bet)]
        f = lv[0].reshape(-1, 32)
        z = (lv[0] - f.mean(dim=0)) * (lv[1] / torch.sqrt(f.var(dim=0, unbiased=False) + 1e-3)) + lv[2]
        (z * mask.to(dt) * gob.to(dt)).sum().backward()
        r.append([t.grad.numpy() for t in lv])
    ref3 = list(zip(*r))
    sw(lambda go, x, m, v, g, bt: ops.bn_train_grad(go, x, m, v, g, bt, 1e-3, True),
       [gob.to(dev), yb.to(dev), mean, var, gam.to(dev), bet.to(dev)], lambda *a: ref3, exact="f32")
    # softmax_xent_grad
    logits = torch.from_numpy(rng.uniform(-2, 2, (4, 30, 21)).astype(np.float32))
    labels = torch.from_numpy(rng.integers(0, 21, (4, 30)).astype(np.int32))
    wts = torch.from_numpy(rng.uniform(0.5, 2, (4, 30)).astype(np.float32))
    loss, lse, pred, npres = ops.softmax_xent(logits.to(dev), labels.to(dev), wts.to(dev))
    r = []
    for dt in both:
        l, _, z = HR.xent_ref(torch, logits.reshape(-1, 21), labels.reshape(-1), wts.reshape(-1), dt)
        (l * 1.5).backward()
        r.append(z.grad.reshape(logits.shape).numpy())
    gl = torch.full((), 1.5, device=dev)
    sw(lambda z, lab, wt, ls: ops.softmax_xent_grad(gl, z, lab, wt, ls, npres),
       [logits.to(dev), labels.to(dev), wts.to(dev), lse], lambda *a: [(r[0], r[1])], exact="f32")
    # group_concat_train_grad (ordered sum: bit-reproducible)
    s = small(env)
    g = rng.uniform(-1, 1, (s["B"], s["M"], s["ns"], s["C"] + 3)).astype(np.float32)
    sw(lambda go, i: ops.group_concat_train_grad(go, i, s["N"], s["C"], 3), [g, s["idx"]],
       lambda go, i: O.group_point_grad(s["N"], i, np.ascontiguousarray(go[..., 3:])), exact=False)


@on_gpu
def test_strided_prediction_ops(env):
    """scene_vote, scene_labels, label_lut and map_back_rows on strided GPU tensors: the bits of
    the contiguous call and of the host twins (csrc/cpu_predict.cpp)."""
    pkg, O, torch, dev, ops = env
    rng = np.random.default_rng(15)
    sw = lambda *a, **k: strided_sweep(torch, dev, *a, **k)  # noqa: E731
    C = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    n, row0 = 50, 7
    logits = rng.integers(0, 6, (3, 40, 5)).astype(np.float32)
    mask = (rng.uniform(size=(3, 40)) < 0.7).astype(np.uint8)
    orig = rng.integers(-1, n + 1, (3, 40)).astype(np.int32)

    def vote(device):
        def run(lg, mk, og):
            keys = torch.zeros(n, dtype=torch.int64, device=device)
            return ops.scene_vote(lg, mk, og, row0, keys), keys
        return run
    host_vote = lambda lg, mk, og: vote("cpu")(C(lg), C(mk), C(og))  # noqa: E731
    sw(vote(dev), [logits, mask, orig], lambda *a: tuple(t.numpy() for t in host_vote(*a)))
    keys = host_vote(logits, mask, orig)[1]
    lut = rng.integers(0, 40, (2, 30)).astype(np.int32)   # (rows of a wider table as views)
    sw(lambda lt: ops.scene_labels(keys.to(dev), lt[0], -5), [lut],
       lambda lt: tuple(t.numpy() for t in ops.scene_labels(keys, C(lt[0]), -5)))
    inp = rng.integers(-3, 40, (3, 40)).astype(np.int32)
    sw(lambda a, lt: ops.label_lut(a, lt[0], -5), [inp, lut],
       lambda a, lt: ops.label_lut(C(a), C(lt[0]), -5).numpy())
    values = rng.uniform(-1, 1, (120, 4)).astype(np.float32)

    def back(device):
        def run(v):
            out = torch.full((n, 4), 9.0, device=device)
            ops.map_back_rows(v, row0, keys.to(device), out)
            return out
        return run
    sw(back(dev), [values], lambda v: back("cpu")(C(v)).numpy())


@on_gpu
def test_strided_leaves_receive_their_gradients(env, attn_ref):
    """Autograd through a channel slice: the leaf is the wide tensor; the gradient that arrives
    in it is the contiguous call's, scattered into the slice, zeros elsewhere. Every backward
    runs on a strided grad_out."""
    pkg, O, torch, dev, ops = env
    s = small(env)
    T = lambda a: tdev(torch, dev, a)  # noqa: E731
    dist, nidx = (T(a) for a in O.three_nn(s["xyz"], s["new_xyz"]))
    w = T(O.idw_weights(dist.cpu().numpy()))
    xyz, nx, idx, fidx = T(s["xyz"]), T(s["new_xyz"]), T(s["idx"]), T(s["fidx"])
    Q, K, V = (T(a) for a in attn_ref[:3])
    rng = s["rng"]
    p2 = T(rng.uniform(-1, 1, (s["B"], s["M"], s["C"])).astype(np.float32))
    pts = T(s["pts"])
    x4 = T(rng.uniform(-1, 1, (s["B"], s["M"], s["ns"], s["C"])).astype(np.float32))
    wm = T(rng.uniform(-0.4, 0.4, (8, 32)).astype(np.float32))
    gam = T(rng.uniform(0.5, 1.5, 32).astype(np.float32))
    g8 = T(rng.uniform(0.5, 1.5, 8).astype(np.float32))
    wq = [T(rng.uniform(-0.5, 0.5, (8, 8)).astype(np.float32)) if i % 2 == 0
          else T(rng.uniform(-0.1, 0.1, 8).astype(np.float32)) for i in range(6)]
    labels = T(rng.integers(0, 8, (s["B"], s["N"])).astype(np.int32))
    first = lambda o: o[0] if isinstance(o, (tuple, list)) else o  # noqa: E731
    wrappers = {
        "gather_point": (xyz, lambda t: pkg.tf_sampling.gather_point(t, fidx)),
        "group_point": (pts, lambda t: pkg.tf_grouping.group_point(t, idx)),
        "three_interpolate": (p2, lambda t: pkg.tf_interpolate.three_interpolate(t, nidx, w)),
        "attn_reduce Q": (Q, lambda t: pkg.attention_layer.attention_reduce(t, K, V)),
        "attn_reduce K": (K, lambda t: pkg.attention_layer.attention_reduce(Q, t, V)),
        "attn_reduce V": (V, lambda t: pkg.attention_layer.attention_reduce(Q, K, t)),
        "group_concat_train": (pts, lambda t: ops.group_concat_train(xyz, t, nx, idx, True, False)),
        "fp_apply_train p1": (pts, lambda t: ops.fp_apply_train(dist, nidx, t, p2)),
        "fp_apply_train p2": (p2, lambda t: ops.fp_apply_train(dist, nidx, pts, t)),
        "fp_interpolate": (p2, lambda t: pkg.pointnet_util.fp_interpolate(xyz, nx, pts, t)),
        "mlp_layer_train": (x4, lambda t: ops.mlp_layer_train(t, wm, gam, gam, gam, 1e-3, True)),
        "mlp_layer_train_pool": (x4, lambda t: ops.mlp_layer_train_pool(t, wm, gam, gam, gam, 1e-3, True)),
        "attn_kv_train": (x4, lambda t: ops.attn_kv_train(t, *wq, True)),
        "bn_train": (x4, lambda t: ops.bn_train(t, g8, g8, 1e-3, True)),
        "dropout": (x4, lambda t: ops.dropout(t, 0.5, 77)),
        "softmax_xent": (pts, lambda t: ops.softmax_xent(t, labels, None)),
    }
    for name, (t, fn) in wrappers.items():
        wide = torch.zeros(t.shape[:-1] + (t.shape[-1] + 3,), device=dev)
        wide[..., 3:] = t
        wide.requires_grad_(True)
        leaf = t.clone().requires_grad_(True)
        out_v, out_c = first(fn(wide[..., 3:])), first(fn(leaf))
        same_bits(out_v, out_c, name)
        if out_c.dim() == 0:
            gv = gc = torch.ones((), device=dev)
        else:
            gw = torch.rand(out_c.shape[:-1] + (out_c.shape[-1] + 2,), device=dev)
            gv = gw[..., 2:]
            assert not gv.is_contiguous() or gv.shape[-1] == 1
            gc = gv.contiguous()
        out_v.backward(gv)
        out_c.backward(gc)
        if name in ("gather_point", "group_point", "three_interpolate"):  # float atomics
            np.testing.assert_allclose(wide.grad[..., 3:].cpu().numpy(), leaf.grad.cpu().numpy(), **TOL)
        else:
            same_bits(wide.grad[..., 3:], leaf.grad, name + ": gradient in the slice")
        assert not wide.grad[..., :3].any(), name + ": gradient outside the slice"


@on_gpu
def test_in_place_arguments_reject_views(env):
    """confusion, counts, out, keys and the Adam lists are updated in place: a non-contiguous
    one is rejected (ValueError), never silently replaced by a temporary copy."""
    pkg, O, torch, dev, ops = env
    lab = torch.zeros(10, dtype=torch.int32, device=dev)
    conf = torch.zeros((4, 8), dtype=torch.int64, device=dev)
    cnt = torch.zeros(4, dtype=torch.int64, device=dev)
    ok_conf, ok_cnt = torch.zeros((4, 4), dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError, match="contiguous"):
        ops.seg_confusion(lab, lab, conf[:, ::2], ok_cnt)
    with pytest.raises(ValueError):
        ops.seg_confusion(lab, lab, ok_conf, cnt[::2])
    keys = torch.zeros((6, 2), dtype=torch.int64, device=dev)
    with pytest.raises(ValueError):
        ops.scene_vote(None, torch.ones(3, dtype=torch.uint8, device=dev),
                       torch.arange(3, dtype=torch.int32, device=dev), 0, keys[:, 0])
    out = torch.zeros((6, 6), device=dev)
    with pytest.raises(ValueError, match="contiguous"):
        ops.map_back_rows(torch.ones((3, 3), device=dev), 0, keys[:, 0].contiguous(), out[:, :3])
    p = torch.ones((4, 6), device=dev)
    for slot in range(4):
        lists = [[torch.ones((4, 3), device=dev)] for _ in range(4)]
        lists[slot] = [p[:, ::2]]
        with pytest.raises(ValueError, match="contiguous"):
            ops.adam_step(*lists, 1e-3, 0.9, 0.999, 1e-8)
    torch.cuda.synchronize()
    assert not conf.any() and not cnt.any() and not keys.any() and not out.any()
    assert torch.equal(p, torch.ones_like(p))
