"""The culled samplers run over a cloud's distinct points only (csrc/fps_cull.h, DESIGN.md
§3.1 "Distinct points"): points with the same coordinate bits are merged into the one with the
smallest tie key before the sort, and the picks must stay the oracle's, index-exact and
new_xyz bit-exact. Clouds built around the copies, at the smallest N each instantiation takes
(SA1 kernel: just above 4,096; MSG kernel: just above 8,192), B = 2, M <= 256, through
pn2_fps_gather_sched with the schedules of tests/test_gpu_a_fullsize.py's SAMPLER_CASES; and
one cfg2 crop through the product path (pn2_fps_chain_grid)."""
import importlib

import numpy as np
import pytest

from conftest import PKG_NAME
from support import clouds, f32_bits, gpu_marks

pytestmark = gpu_marks

B = 2
SIZES = {"sa1": 4100, "msg": 8200}


@pytest.fixture(scope="module")
def env():
    import torch

    from oracle import oracle as O
    O.set_threads(16)
    pkg = importlib.import_module(PKG_NAME)
    return pkg, O, torch, torch.device("cuda:0")


def _key(k):
    return (k % 512) * 65536 + k // 512


def _uniform(rng, n):
    return rng.random((B, n, 3)).astype(np.float32)


def _twice_far(rng, N):
    """Every point twice, the copies shuffled over the second half: the index distance is
    ~N / 2 and which of the two has the smaller key (k mod 512, k div 512) is a coin toss."""
    u = _uniform(rng, N // 2)
    x = np.concatenate([u, np.stack([u[b][rng.permutation(N // 2)] for b in range(B)])], 1)
    return x


def _copies_of_0(rng, N):
    x = _uniform(rng, N)
    for b in range(B):
        x[b, rng.choice(np.arange(1, N), 60, replace=False)] = x[b, 0]
    return x


def _one_point_thousands(rng, N):
    x = _uniform(rng, N)
    for b in range(B):
        at = rng.choice(np.arange(1, N), 3000, replace=False)
        x[b, at] = x[b, at[0]]
    return x


def _all_identical(rng, N):
    return np.tile(np.array([[0.25, 0.5, 0.75]], np.float32), (B, N, 1)).reshape(B, N, 3)


def _few_distinct(rng, N):  # 100 distinct points: M = 256 is beyond them
    u = rng.random((100, 3)).astype(np.float32)
    return np.stack([u[rng.integers(0, 100, N)] for _ in range(B)])


def _zero_and_nan(rng, N):
    """(0.5, +0.0, 0.25) and (0.5, -0.0, 0.25): equal as floats, different bits, two groups
    (the reference's tie rule decides between them). Two points with the same NaN bits in x:
    one group; a NaN distance never lowers a running min (the reference's min and '>' ignore
    it), so once the NaN point is picked it holds the maximum for good and every later pick is
    the member with the smaller key."""
    x = _uniform(rng, N)
    nan = np.array([0x7FC00000], np.uint32).view(np.float32)[0]
    for b in range(B):
        x[b, 777] = x[b, 3000] = (0.5, 0.0, 0.25)
        x[b, 3000, 1] = np.float32(-0.0)
        x[b, 1500] = x[b, 2049] = (nan, 0.25, 0.5)  # key(2049) < key(1500)
    return x


CASES = {
    "twice_far": (_twice_far, 256), "copies_of_0": (_copies_of_0, 128),
    "one_point_thousands": (_one_point_thousands, 128), "all_identical": (_all_identical, 64),
    "few_distinct": (_few_distinct, 256), "zero_and_nan": (_zero_and_nan, 64),
    "uniform": (_uniform, 256),
}


def _sched(pkg, torch, x, M, sched):
    Bx, N = x.shape[0], x.shape[1]
    idx = torch.empty((Bx, M), dtype=torch.int32, device=x.device)
    nx = torch.empty((Bx, M, 3), dtype=torch.float32, device=x.device)
    rc = pkg._lib.lib().pn2_fps_gather_sched(x.data_ptr(), Bx, N, M, idx.data_ptr(),
                                             nx.data_ptr(), sched,
                                             torch.cuda.current_stream().cuda_stream)
    return rc, idx, nx


def _exact(name, got, want):
    assert got.shape == want.shape, (name, got.shape, want.shape)
    bad = got != want if want.dtype == np.int32 else f32_bits(got) != f32_bits(want)
    assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.size} values differ (bit-exact bar)"


@pytest.fixture(scope="module")
def cloud_and_ref(env):
    """Each (case, size)'s cloud and the oracle's picks, computed once."""
    _, O, _, _ = env
    made = {}

    def get(case, size):
        if (case, size) not in made:
            make, M = CASES[case]
            x = make(np.random.default_rng(17), SIZES[size])
            assert x.shape == (B, SIZES[size], 3) and x.dtype == np.float32
            ref = O.fps(x, M)
            made[case, size] = (x, M, ref, O.gather_point(x, ref))
        return made[case, size]
    return get


@pytest.mark.parametrize("sched", [0, 1])
@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("case", list(CASES))
def test_fps_over_distinct_points(env, cloud_and_ref, case, size, sched):
    pkg, O, torch, dev = env
    x, M, ref, ref_xyz = cloud_and_ref(case, size)
    if case == "twice_far":  # the key decides: many representatives are the later index
        _, inv = np.unique(x[0].view(np.uint32), axis=0, return_inverse=True)
        order = np.argsort(inv.reshape(-1), kind="stable").reshape(-1, 2)  # (first, copy) index
        assert (order[:, 1] - order[:, 0] >= 1).all() and order[:, 1].min() >= SIZES[size] // 2
        assert 0.2 < np.mean(_key(order[:, 1]) < _key(order[:, 0])) < 0.8
    rc, idx, new_xyz = _sched(pkg, torch, torch.from_numpy(x).to(dev), M, sched)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert pkg._lib.lib().pn2_fault_status(1) == 0, "the sampler stored a device fault"
    _exact(f"{case} {size} idx", idx.cpu().numpy(), ref)
    _exact(f"{case} {size} new_xyz", new_xyz.cpu().numpy(), ref_xyz)


# The search for copies is a hash table in LDS: two rounds, one atomic and one read per point
# and round, plus at most one compare with the slot's winner. Thousands of copies of one point
# all go to one slot, where a wave's 64 atomics run one after the other instead of at once.
# The whole pass is under 2 % of a launch at these sizes (2-5 us of ~100-130), its atomics a
# part of that: if all of it ran 64 times slower it would add 1.3 launches, while the sort and
# the sampling only get cheaper (fewer points). So 2.3 times the duplicate-free launch is
# the bound; 3 leaves room for the timer's noise on a shared GPU.
TIME_MULTIPLE = 3.0


@pytest.mark.parametrize("size", list(SIZES))
def test_many_copies_cost_no_more_than_the_bound(env, cloud_and_ref, size):
    pkg, O, torch, dev = env

    def best_of(x, M):
        xt = torch.from_numpy(x).to(dev)
        t = []
        for _ in range(4):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            assert _sched(pkg, torch, xt, M, 0)[0] == 0
            b.record()
            b.synchronize()
            t.append(a.elapsed_time(b))
        return min(t[1:])
    M = CASES["one_point_thousands"][1]
    heavy = best_of(cloud_and_ref("one_point_thousands", size)[0], M)
    free = best_of(cloud_and_ref("uniform", size)[0], M)
    print(f"{size}: {heavy * 1e3:.1f} us with 3,000 copies of one point, {free * 1e3:.1f} us "
          f"duplicate-free")
    assert heavy <= TIME_MULTIPLE * free, (heavy, free)


def test_cfg2_crop_product_path(env):
    """One cfg2 batch straight from synth.batch through pn2_fps_chain_grid (the SA1 sampler
    that grids its picks, then SA2-4): every stage against the oracle's samplers."""
    pkg, O, torch, dev = env
    x = clouds(pkg, "scannet", B, 8192, seed=21)
    bits = x.view(np.uint32).reshape(B, 8192, 3)
    assert len(np.unique(bits[0], axis=0)) < 0.8 * 8192, "the crops are drawn with replacement"
    npoints = [1024, 256, 64, 16]
    out = [(torch.empty((B, m), dtype=torch.int32, device=dev),
            torch.empty((B, m, 3), dtype=torch.float32, device=dev)) for m in npoints]
    kgrid = pkg.grid.PointGrid(out[0][1], 0.0, build=False)
    pkg.tf_sampling.farthest_point_sample_chain(npoints, torch.from_numpy(x).to(dev), out=out,
                                                grid0=kgrid)
    torch.cuda.synchronize()
    assert pkg._lib.lib().pn2_fault_status(1) == 0
    cur = x
    for k, ((i, n), m) in enumerate(zip(out, npoints)):
        r = O.fps(cur, m)
        _exact(f"SA{k + 1} idx", i.cpu().numpy(), r)
        cur = O.gather_point(cur, r)
        _exact(f"SA{k + 1} new_xyz", n.cpu().numpy(), cur)
