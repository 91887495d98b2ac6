"""The opt-in bf16 matrix-core mode of the fused MLP kernels (csrc/mlp.hip, PN2_MLP_BF16) on the
GPU, against its written contract (include/pn2hip.h at pn2_mlp_pack_bf16). The evaluations E
(the contract, float64 sums), F (no rounding, float64) and E32 (the contract in numpy float32)
and the inputs are in tests/mlp_bf16_ref.py; tests/test_mlp_bf16_cpu.py shows on the same
inputs that a float32 evaluation stays within 1/64 of max|E - F| where these tests allow 1/16.

1. layout, exact: operands that every format holds exactly give the same bits on the bf16 and
   the fp32 path (and E's), in every entry point; no tolerance
2. rounding mode: an identity layer returns bf16(x) on ties and near-ties
3. single layers against E under the project's fp32 bar, with E32 as the yardstick
4. chains, and the fused grouping / interpolation / attention kernels, under |E - F| / 16
5. the Python level: ParamStore(precision=...) through the three modules and the model
"""
import importlib

import numpy as np
import pytest

import mlp_bf16_ref as R
from conftest import PKG_NAME
from support import gpu_marks, same_bits, tolerance

pytestmark = gpu_marks


@pytest.fixture(scope="module")
def env():
    import torch
    pkg = importlib.import_module(PKG_NAME)
    return pkg, torch, torch.device("cuda:0")


class RawLayer:
    """A layer of mlp_bf16_ref packed through the C ABI with its scale and shift as given (no
    bias, so the packed shift is the shift itself): what tf_util.SharedMLP needs of a layer."""

    def __init__(self, env, L):
        pkg, torch, dev = env
        lb, lib = pkg._lib, pkg._lib.lib()
        self.cin, self.cout = L["W"].shape
        self.w = torch.from_numpy(L["W"]).to(dev).contiguous()
        sc = None if L["scale"] is None else torch.from_numpy(L["scale"]).to(dev)
        sh = None if L["shift"] is None else torch.from_numpy(L["shift"]).to(dev)
        size, pack = ((lib.pn2_mlp_packed_size_bf16, lib.pn2_mlp_pack_bf16) if L["bf16"] else
                      (lib.pn2_mlp_packed_size, lib.pn2_mlp_pack))
        nbytes = int(size(self.cin, self.cout))
        self.buf = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=dev)
        lb.check(pack(lb.ptr(self.w), None, lb.ptr(sc), lb.ptr(sh), self.cin, self.cout,
                      lb.ptr(self.buf), nbytes, lb.stream_of(self.buf)), "pack")
        self.flags = (lb.PN2_MLP_RELU if L["relu"] else 0) | (lb.PN2_MLP_BF16 if L["bf16"] else 0)
        self.MlpLayer = lb.MlpLayer

    def struct(self):
        return self.MlpLayer(self.buf.data_ptr(), self.cin, self.cout, self.flags)


def fused(env, layers):
    return env[0].tf_util.SharedMLP([RawLayer(env, L) for L in layers])


def dev_(env, a):
    return None if a is None else env[1].from_numpy(np.ascontiguousarray(a)).to(env[2])


def run_rows(env, x, layers):
    return fused(env, layers)(dev_(env, x)).cpu().numpy()


def run_group(env, xyz, points, new_xyz, idx, layers, pool, xyz_last=False):
    return env[0].pointnet_util.group_mlp(
        dev_(env, xyz), dev_(env, points), dev_(env, new_xyz), dev_(env, idx),
        fused(env, layers), pool, xyz_last=xyz_last).cpu().numpy()


def run_fp(env, dist, nn, p1, p2, layers):
    return env[0].pointnet_util.fp_mlp(dev_(env, dist), dev_(env, nn), dev_(env, p1),
                                       dev_(env, p2), fused(env, layers)).cpu().numpy()


def run_attention(env, xyz, points, new_xyz, idx, layers, dense, sc, sh, add_max):
    pkg, torch, dev = env
    lb, lib = pkg._lib, pkg._lib.lib()
    mlp = fused(env, layers)
    qkv = [RawLayer(env, L) for L in dense]
    table = (lb.MlpLayer * 3)(*[d.struct() for d in qkv])
    t = [dev_(env, a) for a in (xyz, points, new_xyz, idx, sc, sh)]
    B, N = xyz.shape[:2]
    M, ns = idx.shape[1:]
    C = 0 if points is None else points.shape[2]
    out = torch.empty((B, M, mlp.cout), dtype=torch.float32, device=dev)
    tab, n = mlp.table()
    rc = lib.pn2_group_mlp_attention(lb.ptr(t[0]), lb.ptr(t[1]), lb.ptr(t[2]), lb.ptr(t[3]), B, N,
                                     C, M, ns, lb.PN2_USE_XYZ, n, tab, table, lb.ptr(t[4]),
                                     lb.ptr(t[5]), 1 if add_max else 0, lb.ptr(out),
                                     lb.stream_of(out))
    lb.check(rc, "group_mlp_attention")
    return out.cpu().numpy()


# ---------------------------------------------------------------- 1. layout, exact

@pytest.mark.parametrize("widths", R.SHAPE_WIDTHS + (R.BIG_SHAPE[2],), ids=str)
def test_layout_exact_shared_mlp(env, widths):
    big = widths == R.BIG_SHAPE[2]
    shapes = [R.BIG_SHAPE[:2]] if big else [(r, c) for r in R.SHAPE_ROWS for c in R.SHAPE_CINS]
    for rows, cin in shapes:
        x, layers = R.exact_chain(np.random.default_rng([rows, cin, len(widths)]), rows, cin,
                                  widths)
        got = run_rows(env, x, layers)
        what = f"rows {rows} cin {cin} widths {widths}"
        same_bits(got, run_rows(env, x, R.as_fp32(layers)), what + ": bf16 vs fp32 path")
        same_bits(got, R.chain_eval(x, layers, "E").astype(np.float32), what + ": vs E")


def _exact_geometry(rng, B, N, M, ns):
    xyz = (rng.integers(-2, 3, (B, N, 3)) / 8.0).astype(np.float32)
    new_xyz = np.zeros((B, M, 3), np.float32)  # xyz - 0: the centred xyz stays exact
    idx = rng.integers(0, N, (B, M, ns)).astype(np.int32)
    return xyz, new_xyz, idx


@pytest.mark.parametrize("ns,C,pool,xyz_last,widths", [
    (8, 0, "max", False, [32]), (32, 6, "max", False, [32, 32, 64]),
    (32, 5, None, True, [13, 40]), (64, 16, "max", False, [21]),
    (128, 6, None, False, [32, 32, 64]), (32, 0, "max", False, [64, 128, 256]),
], ids=str)
def test_layout_exact_group_mlp(env, ns, C, pool, xyz_last, widths):
    """The grouped source: the last layer runs with the points in the accumulator rows (the
    other lane map), with the weights in LDS and, for the widest chain, in global memory."""
    rng = np.random.default_rng([ns, C, len(widths)])
    xyz, new_xyz, idx = _exact_geometry(rng, 2, 256, 16, ns)
    points = (rng.integers(-2, 3, (2, 256, C)) / 8.0).astype(np.float32) if C else None
    _, layers = R.exact_chain(rng, 1, 3 + C, widths)
    got = run_group(env, xyz, points, new_xyz, idx, layers, pool, xyz_last)
    ref = run_group(env, xyz, points, new_xyz, idx, R.as_fp32(layers), pool, xyz_last)
    same_bits(got, ref, "group_mlp: bf16 vs fp32 path")
    E = R.pool_eval(R.chain_eval(R.group_rows(xyz, points, new_xyz, idx, xyz_last), layers, "E"),
                    pool)
    same_bits(got, E.astype(np.float32), "group_mlp vs E")


@pytest.mark.parametrize("C1,widths", [(0, [64, 32]), (6, [21]), (5, [32, 32, 64])], ids=str)
def test_layout_exact_fp_mlp(env, C1, widths):
    """IDW weights (1/4, 1/4, 1/2) from distances (1, 1, 1/2): the interpolated features are
    sums of integers over 32, exact in bf16."""
    rng = np.random.default_rng([C1, len(widths)])
    B, n, m, C2 = 2, 100, 20, 32
    dist = np.broadcast_to(np.array([1, 1, 0.5], np.float32), (B, n, 3)).copy()
    nn = rng.integers(0, m, (B, n, 3)).astype(np.int32)
    p1 = (rng.integers(-2, 3, (B, n, C1)) / 8.0).astype(np.float32) if C1 else None
    p2 = (rng.integers(-2, 3, (B, m, C2)) / 8.0).astype(np.float32)
    _, layers = R.exact_chain(rng, 1, C1 + C2, widths)
    x = R.fp_rows(dist, nn, p1, p2)
    assert np.array_equal(R.bf16_round(x), x)
    got = run_fp(env, dist, nn, p1, p2, layers)
    same_bits(got, run_fp(env, dist, nn, p1, p2, R.as_fp32(layers)), "fp_mlp: bf16 vs fp32 path")
    same_bits(got, R.chain_eval(x, layers, "E").astype(np.float32), "fp_mlp vs E")


@pytest.mark.parametrize("widths,ns,M,add_max", [([32, 64], 32, 16, True), ([512], 32, 4, False)],
                         ids=str)
def test_layout_exact_attention(env, widths, ns, M, add_max):
    """Key and value Dense as bf16 against fp32 on exact operands: the MLP output X is made of
    eighths and the Dense weights have one +-1 per output, so K and V are exact; everything
    after them is the same fp32 code on the same values."""
    rng = np.random.default_rng([ns, M, widths[-1]])
    B = 1 if widths[-1] == 512 else 2
    xyz, new_xyz, idx = _exact_geometry(rng, B, 256, M, ns)
    points = (rng.integers(-2, 3, (B, 256, 6)) / 8.0).astype(np.float32)
    _, layers = R.exact_chain(rng, 1, 9, widths)
    # X = the chain's last layer feeds the Dense layers: keep it bf16-exact (one weight per output)
    C, cprev = widths[-1], 9 if len(widths) == 1 else widths[-2]
    W = np.zeros((cprev, C), np.float32)
    W[rng.integers(0, cprev, C), np.arange(C)] = rng.choice([-1.0, 1.0], C)
    layers[-1] = dict(layers[-1], W=W, relu=True)
    dense = []
    for j in range(3):
        Wd = np.zeros((C, C), np.float32)
        Wd[rng.integers(0, C, C), np.arange(C)] = rng.choice([-1.0, 1.0], C)
        dense.append({"W": Wd, "scale": None, "shift": (rng.integers(-2, 3, C) / 8.0).astype(
            np.float32), "relu": False, "bf16": j > 0})
        dense[-1]["scale"] = np.ones(C, np.float32)
    sc = rng.uniform(0.5, 1.5, C).astype(np.float32)
    sh = rng.uniform(-0.5, 0.5, C).astype(np.float32)
    got = run_attention(env, xyz, points, new_xyz, idx, layers, dense, sc, sh, add_max)
    ref = run_attention(env, xyz, points, new_xyz, idx, R.as_fp32(layers), R.as_fp32(dense), sc,
                        sh, add_max)
    assert np.abs(got).max() > 0
    same_bits(got, ref, "group_mlp_attention: bf16 vs fp32 path")


# ---------------------------------------------------------------- 2. rounding mode

def _tie_values():
    t = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20, 1 + 2.0 ** -8 - 2.0 ** -20]
    v = np.array(t + [-a for a in t], np.float32)
    # nearest even: 1, 1 + 2^-6, 1 + 2^-7, 1 (truncation gives 1, 1 + 2^-7, 1 + 2^-7, 1; half-up
    # gives 1 + 2^-7, 1 + 2^-6, 1 + 2^-7, 1)
    want = np.array([1, 1 + 2.0 ** -6, 1 + 2.0 ** -7, 1], np.float32)
    assert np.array_equal(R.bf16_round(v), np.concatenate([want, -want]))
    return v


def test_rounding_is_nearest_even(env):
    v = _tie_values()
    rng = np.random.default_rng(8)
    ident = {"W": np.eye(32, dtype=np.float32), "scale": None, "shift": None, "relu": False,
             "bf16": True}
    x = rng.choice(v, (100, 32)).astype(np.float32)
    same_bits(run_rows(env, x, [ident]), R.bf16_round(x), "identity layer over rows")
    # the grouped source: the points in the accumulator rows; [xyz - 0, points] = 32 columns
    B, N, M, ns = 1, 64, 2, 32
    xyz = rng.choice(v, (B, N, 3)).astype(np.float32)
    points = rng.choice(v, (B, N, 29)).astype(np.float32)
    new_xyz = np.zeros((B, M, 3), np.float32)
    idx = np.arange(M * ns, dtype=np.int32).reshape(B, M, ns)
    got = run_group(env, xyz, points, new_xyz, idx, [ident], None)
    same_bits(got, R.bf16_round(R.group_rows(xyz, points, new_xyz, idx)), "identity, grouped")


# ---------------------------------------------------------------- 3. single layers vs E

def _single_layer_shapes(widths):
    if widths == R.BIG_SHAPE[2]:
        rows, cin = R.BIG_SHAPE[:2]
        return [(rows, cin, widths[0]), (rows, widths[0], widths[1])]
    out = [(r, c, widths[0]) for r in R.SHAPE_ROWS for c in R.SHAPE_CINS]
    return out + [(r, a, b) for r in R.SHAPE_ROWS for a, b in zip(widths, widths[1:])]


@pytest.mark.parametrize("widths", R.SHAPE_WIDTHS + (R.BIG_SHAPE[2],), ids=str)
def test_single_layer_vs_contract(env, widths):
    """Every layer of the shapes of test 1, alone, under the project's bar for fp32 work:
    max|gpu - E| <= max(4 max|E32 - E|, 1e-6 (1 + max|E|))."""
    for rows, cin, cout in _single_layer_shapes(widths):
        rng = np.random.default_rng([rows, cin, cout])
        L = R.make_layer(rng, cin, cout)
        x = rng.uniform(-1, 1, (rows, cin)).astype(np.float32)
        got = run_rows(env, x, [L]).astype(np.float64)
        E, E32 = R.layer_eval(x.astype(np.float64), L, "E"), R.layer_eval(x, L, "E32")
        err, (tol, err32) = np.abs(got - E).max(), tolerance(E, E32)
        print(f"rows {rows} {cin}->{cout}: max|gpu - E| = {err:.3g}, max|E32 - E| = {err32:.3g}")
        assert err <= tol, f"rows {rows} {cin}->{cout}: {err:.3g} > {tol:.3g}"


# ---------------------------------------------------------------- 4. chains vs E

def assert_chain_bound(got, evaluate, what):
    E, F = evaluate("E"), evaluate("F")
    assert got.shape == E.shape, (what, got.shape, E.shape)
    err, d = np.abs(got.astype(np.float64) - E).max(), np.abs(E - F).max()
    print(f"{what}: max|gpu - E| = {err:.3g}, max|E - F| = {d:.3g}, ratio {err / d:.3g}")
    assert np.isfinite(got).all(), what
    assert err <= d / 16, f"{what}: max|gpu - E| = {err:.3g} > max|E - F| / 16 = {d / 16:.3g}"


@pytest.mark.parametrize("name", sorted(R.CHAINS))
def test_chain_vs_contract(env, name):
    for seed in R.chain_seeds(name):
        x, layers = R.chain_case(name, seed)
        assert_chain_bound(run_rows(env, x, layers), R.chain_evaluate(name, seed),
                           f"{name}/{seed}")


@pytest.mark.parametrize("ns,C,pool,xyz_last", R.GROUP_CASES)
def test_group_mlp_vs_contract(env, ns, C, pool, xyz_last):
    seed = R.group_seed(ns, C, pool, xyz_last)
    xyz, points, new_xyz, idx, layers = R.group_case(ns, C, seed)
    got = run_group(env, xyz, points, new_xyz, idx, layers, pool, xyz_last)
    assert_chain_bound(got, R.group_evaluate(ns, C, pool, xyz_last, seed),
                       f"group_mlp ns={ns} C={C} {pool}")


@pytest.mark.parametrize("C1", [0, 6])
def test_fp_mlp_vs_contract(env, C1):
    seed = R.fp_seed(C1)
    dist, nn, p1, p2, layers = R.fp_case(C1, seed)
    assert_chain_bound(run_fp(env, dist, nn, p1, p2, layers), R.fp_evaluate(C1, seed),
                       f"fp_mlp C1={C1}")


@pytest.mark.parametrize("C_in,widths,ns,B,M,add_max", R.ATTN_CASES, ids=str)
def test_attention_vs_contract(env, C_in, widths, ns, B, M, add_max):
    seed = R.attn_seed(C_in, tuple(widths), ns, B, M, add_max)
    case = R.attn_case(C_in, widths, ns, B, M, seed)
    got = run_attention(env, *case, add_max)
    assert_chain_bound(got, R.attn_evaluate(C_in, widths, ns, B, M, add_max, seed),
                       f"group_mlp_attention C={widths[-1]} add_max={add_max}")


def test_bf16_query_is_invalid(env):
    pkg = env[0]
    case = list(R.attn_case(6, [32, 32, 64], 32, 2, 16, 0))
    case[5] = [dict(L, bf16=True) for L in case[5]]
    with pytest.raises(pkg.InvalidArgumentError):
        run_attention(env, *case, False)


def test_pack_bf16_rejects_an_undersized_buffer(env):
    pkg, torch, dev = env
    lb, lib = pkg._lib, pkg._lib.lib()
    w = torch.zeros((19, 40), device=dev)
    need = int(lib.pn2_mlp_packed_size_bf16(19, 40))
    buf = torch.empty(need // 4, dtype=torch.float32, device=dev)
    args = (lb.ptr(w), None, None, None, 19, 40, lb.ptr(buf))
    assert lib.pn2_mlp_pack_bf16(*args, need - 1, lb.stream_of(buf)) == lb.PN2_EINVAL
    assert lib.pn2_mlp_pack_bf16(*args, need, lb.stream_of(buf)) == lb.PN2_OK
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 5. the Python level

def _layer_terms(torch, p, eps):
    """scale and shift of a packed layer from its variables, in PackedLayer's arithmetic."""
    W = p["weights"].detach().cpu()
    b = p["biases"].detach().cpu()
    if p.get("gamma") is None:
        return W, torch.ones_like(b), b
    s64 = p["gamma"].detach().cpu().double() / torch.sqrt(
        p["moving_variance"].detach().cpu().double() + eps)
    sc = s64.float()
    sh = (p["beta"].detach().cpu().double() - p["moving_mean"].detach().cpu().double() * s64).float()
    return W, sc, b * sc + sh


def _compose(torch, x, layers, bf16, eps):
    """The layers in torch: .bfloat16().float() operands (when bf16) and a float64 matmul.
    layers: (variables, relu, rounded) with rounded = the layer is bf16 in the bf16 mode."""
    y = x.detach().cpu().double()
    for p, relu, rounded in layers:
        W, sc, sh = _layer_terms(torch, p, eps)
        if bf16 and rounded:
            y = y.float().bfloat16().float().double() @ W.bfloat16().float().double()
        else:
            y = y @ W.double()
        y = y * sc.double() + sh.double()
        y = torch.relu(y) if relu else y
    return y


def _ref_layers(torch, specs, eps):
    """The layers of _compose as mlp_bf16_ref dicts (for its float32 stand-ins)."""
    out = []
    for p, relu, rounded in specs:
        W, sc, sh = _layer_terms(torch, p, eps)
        out.append({"W": W.numpy(), "scale": sc.numpy(), "shift": sh.numpy(), "relu": relu,
                    "bf16": rounded})
    return out


def _first_seed(evaluate_of, start):
    """The first store seed from `start` at which every float32 stand-in of the module stays
    within 1/64 of max|E - F| (mlp_bf16_ref, 'Choice of inputs'): evaluated on the CPU from the
    geometry ops' outputs, before the kernel under test runs."""
    for seed in range(start, start + 32):
        if max(R.ratios(evaluate_of(seed))[0].values()) <= 1 / 64:
            return seed
    raise AssertionError("no usable seed")


def _randomise_bn(torch, store, scope, c, seed):
    g = np.random.default_rng(seed)
    for k, (lo, hi) in {"moving_mean": (-.1, .1), "moving_variance": (.5, 2), "gamma": (.5, 1.5),
                        "beta": (-.2, .2)}.items():
        store[f"{scope}/{k}"] = torch.from_numpy(g.uniform(lo, hi, c).astype(np.float32))


def _assert_bound_t(got, E, F, what):
    err, d = (got.cpu().double() - E).abs().max().item(), (E - F).abs().max().item()
    print(f"{what}: max|gpu - E| = {err:.3g}, max|E - F| = {d:.3g}, ratio {err / d:.3g}")
    assert err <= d / 16, f"{what}: {err:.3g} > {d / 16:.3g}"


@pytest.fixture(scope="module")
def clouds(env):
    pkg, torch, dev = env
    xyz, feats = pkg.synth.batch([0, 1], 512, "scannet", with_features=True)
    return torch.from_numpy(xyz).to(dev), torch.from_numpy(feats).to(dev)


def test_sa_module_on_a_bf16_store(env, clouds):
    pkg, torch, dev = env
    pu, tu = pkg.pointnet_util, pkg.tf_util
    xyz, feats = clouds
    widths = [32, 32, 64]

    def make(seed, **kw):
        store = tu.ParamStore(seed=seed, **kw)
        for i, w in enumerate(widths):
            _randomise_bn(torch, store, f"l1/conv{i}/bn", w, 10 + i)
        return store

    def specs(store):
        return [(store.conv(f"l1/conv{i}", c, w), True, True)
                for i, (c, w) in enumerate(zip([9] + widths, widths))]

    with torch.no_grad():
        _, new_xyz0 = pkg.tf_sampling.farthest_point_sample_and_gather(128, xyz)
        idx0, _ = pkg.tf_grouping.query_ball_point(0.2, 32, xyz, new_xyz0)
        x, _ = pu.group_concat(xyz, feats, new_xyz0, idx0)
    x_np = x.cpu().numpy()

    def evaluate_of(seed):
        ref = _ref_layers(torch, specs(make(seed)), tu.BN_EPSILON)
        return lambda mode: R.chain_eval(x_np, ref, mode).max(axis=2)

    seed = _first_seed(evaluate_of, 3)
    outs = {}
    for prec in ("default", "fp32", "bf16"):
        store = make(seed) if prec == "default" else make(seed, precision=prec)
        with torch.no_grad():
            new_xyz, outs[prec], idx = pu.pointnet_sa_module(
                xyz, feats, 128, 0.2, 32, widths, None, False, False, None, "l1", params=store)
    assert torch.equal(idx, idx0) and torch.equal(new_xyz, new_xyz0)
    assert torch.equal(outs["default"], outs["fp32"])
    assert not torch.equal(outs["bf16"], outs["fp32"])
    layers = specs(store)
    E, F = (_compose(torch, x, layers, b, tu.BN_EPSILON).max(dim=2).values for b in (True, False))
    _assert_bound_t(outs["bf16"], E, F, "pointnet_sa_module")
    # set_precision repacks: the same store now gives the fp32 bits, then the bf16 bits again
    with torch.no_grad():
        back = pu.pointnet_sa_module(xyz, feats, 128, 0.2, 32, widths, None, False, False, None,
                                     "l1", params=store.set_precision("fp32"))[1]
        again = pu.pointnet_sa_module(xyz, feats, 128, 0.2, 32, widths, None, False, False, None,
                                      "l1", params=store.set_precision("bf16"))[1]
    assert torch.equal(back, outs["fp32"]) and torch.equal(again, outs["bf16"])


def test_fp_module_on_a_bf16_store(env, clouds):
    pkg, torch, dev = env
    pu, tu = pkg.pointnet_util, pkg.tf_util
    xyz1, p1 = clouds
    g = torch.Generator().manual_seed(4)
    xyz2 = xyz1[:, torch.randperm(512, generator=g)[:128].to(dev)].contiguous()
    p2 = (torch.rand((2, 128, 64), generator=g) * 2 - 1).to(dev)
    widths = [64, 32]

    def make(seed, **kw):
        store = tu.ParamStore(seed=seed, **kw)
        for i, w in enumerate(widths):
            _randomise_bn(torch, store, f"fa/conv_{i}/bn", w, 20 + i)
        return store

    def specs(store):
        return [(store.conv(f"fa/conv_{i}", c, w), True, True)
                for i, (c, w) in enumerate(zip([70] + widths, widths))]

    with torch.no_grad():
        x = pu.fp_interpolate(xyz1, xyz2, p1, p2)
    x_np = x.cpu().numpy()

    def evaluate_of(seed):
        ref = _ref_layers(torch, specs(make(seed)), tu.BN_EPSILON)
        return lambda mode: R.chain_eval(x_np, ref, mode)

    seed = _first_seed(evaluate_of, 5)
    outs = {}
    for prec in ("fp32", "bf16"):
        store = make(seed, precision=prec)
        with torch.no_grad():
            outs[prec] = pu.pointnet_fp_module(xyz1, xyz2, p1, p2, widths, False, None, "fa",
                                               params=store)
    assert not torch.equal(outs["bf16"], outs["fp32"])
    layers = specs(store)
    E, F = (_compose(torch, x, layers, b, tu.BN_EPSILON) for b in (True, False))
    _assert_bound_t(outs["bf16"], E, F, "pointnet_fp_module")


@pytest.mark.parametrize("and_pooling", [False, True])
def test_attention_module_on_a_bf16_store(env, clouds, and_pooling):
    pkg, torch, dev = env
    al, pu, tu = pkg.attention_layer, pkg.pointnet_util, pkg.tf_util
    xyz, feats = clouds
    widths, C, ns, M = [32, 64], 64, 32, 128
    fn = al.pointnet_sa_module_attention_and_pooling if and_pooling else \
        al.pointnet_sa_module_attention
    qs, ks, vs = al._attention_scopes("att")

    def make(seed, **kw):
        store = tu.ParamStore(seed=seed, **kw)
        _randomise_bn(torch, store, "att/att", C, 2)
        g = np.random.default_rng(6)
        for d in (qs, ks, vs):
            store[f"{d}/bias"] = torch.from_numpy(g.uniform(-.1, .1, C).astype(np.float32))
        return store

    def specs(store):
        return [(store.conv(f"att/conv{i}", c, w), True, True)
                for i, (c, w) in enumerate(zip([9] + widths, widths))]

    with torch.no_grad():
        _, new_xyz0 = pkg.tf_sampling.farthest_point_sample_and_gather(M, xyz)
        idx0, _ = pkg.tf_grouping.query_ball_point(0.2, ns, xyz, new_xyz0)
        x, _ = pu.group_concat(xyz, feats, new_xyz0, idx0)
    x_np = x.cpu().numpy()

    def evaluate_of(seed):
        st = make(seed)
        ref = _ref_layers(torch, specs(st), tu.BN_EPSILON)
        dense = _ref_layers(torch, [(st.dense(s, C, C), False, j > 0)
                                    for j, s in enumerate((qs, ks, vs))], 0)
        sc, sh = (t.cpu().numpy() for t in tu.bn_affine(st, "att/att", C, "cpu"))
        return lambda mode: R.attention_eval(R.chain_eval(x_np, ref, mode), *dense, sc, sh,
                                             and_pooling, mode)

    seed = _first_seed(evaluate_of, 11)
    outs = {}
    for prec in ("fp32", "bf16"):
        store = make(seed, precision=prec)
        with torch.no_grad():
            new_xyz, outs[prec], idx = fn(xyz, feats, M, 0.2, ns, widths, None, False, False,
                                          None, "att", params=store)
    assert torch.equal(idx, idx0)
    assert not torch.equal(outs["bf16"], outs["fp32"])
    layers = specs(store)
    scale, shift = (t.cpu().double() for t in tu.bn_affine(store, "att/att", C, dev))
    res = []
    for b in (True, False):
        X = _compose(torch, x, layers, b, tu.BN_EPSILON)  # (B, M, ns, C) float64
        Q = _compose(torch, X[:, :, 0], [(store.dense(qs, C, C), False, False)], b, 0)
        K, V = (_compose(torch, X, [(store.dense(s, C, C), False, True)], b, 0).reshape(
            2, M, C // 4, ns, 4) for s in (ks, vs))
        a = torch.softmax(torch.einsum("bmhjd,bmhd->bmhj", K, Q.reshape(2, M, C // 4, 4)) / 2,
                          dim=-1)
        out = torch.einsum("bmhj,bmhjd->bmhd", a, V).reshape(2, M, C) * scale + shift
        res.append(out + X.max(dim=2).values if and_pooling else out)
    _assert_bound_t(outs["bf16"], res[0], res[1], f"attention module and_pooling={and_pooling}")


def test_model_keeps_fc2_and_the_query_fp32(env):
    pkg, torch, dev = env
    tu = pkg.tf_util
    xyz = torch.from_numpy(pkg.synth.batch([3], 2048, "scannet")[0]).to(dev)
    store = tu.ParamStore(seed=7, precision="bf16")
    model = importlib.import_module(PKG_NAME + ".pointnet2_sem_seg_attention")
    with torch.no_grad():
        logits = model.get_model(xyz, False, 21, params=store)[0]
    assert logits.shape == (1, 2048, 21) and torch.isfinite(logits).all()
    seen = {}
    for key, mlp in store._packed.items():
        if isinstance(mlp, tu.SharedMLP):
            name = key[1] if key[0] == "dense" else key[0][0]
            seen[name] = {L.precision for L in mlp.layers}
            flags = {bool(L.struct().flags & pkg._lib.PN2_MLP_BF16) for L in mlp.layers}
            assert flags == {p == "bf16" for p in seen[name]}
    assert seen["fc2"] == {"fp32"} and seen["fc1"] == {"bf16"}
    fp32 = sorted(n for n, p in seen.items() if p == {"fp32"})
    queries = sorted(n for n in seen if n.endswith("ScannetAttentionLayer/dense"))
    assert len(queries) == 4 and fp32 == sorted(queries + ["fc2"]), fp32
    for i in range(1, 5):  # key and value Dense
        assert seen[f"layer{i}/ScannetAttentionLayer/dense_1"] == {"bf16"}
        assert seen[f"layer{i}/ScannetAttentionLayer/dense_2"] == {"bf16"}
    assert seen["layer1/conv0"] == {"bf16"} and seen["fa_layer4/conv_0"] == {"bf16"}


def test_training_ignores_the_precision(env, clouds):
    pkg, torch, dev = env
    pu, tu = pkg.pointnet_util, pkg.tf_util
    xyz, feats = clouds
    outs = []
    for prec in ("fp32", "bf16"):
        store = tu.ParamStore(seed=9, precision=prec).trainable(dev)
        out = pu.pointnet_sa_module(xyz, feats, 64, 0.2, 16, [32, 64], None, False, True, None,
                                    "t1", params=store)[1]
        outs.append(out.detach())
    assert torch.equal(outs[0], outs[1])
