"""The sampler chain over an earlier sampler's picks in one launch (fps_chain_prefix_kernel,
csrc/fps.hip): per cloud, the prefix check over every point, then either the copies (idx =
0 .. m - 1, new_xyz = the input's first m points) or the stages run as block-scan samplers
inside the same workgroup.

Every idx and new_xyz of every stage is compared bit for bit with the oracle's sampler
(tf_sampling_g.cu:105-181) applied stage by stage. The inputs are the picks of a real sampler
(pn2_fps_gather, 2048 -> 1024: the v9 block scan) over small ScanNet-like clouds, whole or cut
to ragged sizes, and then edited so that the check must fail.
"""
import ctypes
import importlib

import numpy as np
import pytest

from conftest import PKG_NAME
from support import gpu_marks

pytestmark = gpu_marks


@pytest.fixture(scope="module")
def env():
    import torch

    from oracle import oracle as O
    O.set_threads(16)
    pkg = importlib.import_module(PKG_NAME)
    return pkg, O, torch, torch.device("cuda:0")


@pytest.fixture(scope="module")
def picks(env):
    """(4, 1024, 3): four clouds' first 1024 picks in pick order. Read-only."""
    pkg, O, torch, dev = env
    x = pkg.synth.batch(range(21, 25), 2048, "scannet")[0]
    _, nx = pkg.tf_sampling.farthest_point_sample_and_gather(1024, torch.from_numpy(x).to(dev))
    p = nx.cpu().numpy()
    p.setflags(write=False)
    return p


def _chain(pkg, O, torch, dev, p, npoints, what):
    """pn2_fps_chain over p (B, n, 3): every stage equal to the oracle's, every idx an index of
    its stage's input, no fault. Returns the oracle's idx per stage."""
    h = pkg._lib.lib()
    p = np.array(p, np.float32, order="C")  # (a writable copy)
    B, n = p.shape[:2]
    x = torch.from_numpy(p).to(dev)
    # (rows start as -1: a word the kernel left unwritten cannot pass for an index)
    outs = [(torch.full((B, m), -1, dtype=torch.int32, device=dev),
             torch.full((B, m, 3), np.nan, dtype=torch.float32, device=dev)) for m in npoints]
    npt = (ctypes.c_int * len(npoints))(*npoints)
    ib = (ctypes.c_void_p * len(npoints))(*[o[0].data_ptr() for o in outs])
    nb = (ctypes.c_void_p * len(npoints))(*[o[1].data_ptr() for o in outs])
    rc = h.pn2_fps_chain(x.data_ptr(), B, n, len(npoints), ctypes.addressof(npt),
                         ctypes.addressof(ib), ctypes.addressof(nb),
                         torch.cuda.current_stream().cuda_stream)
    assert rc == 0, (what, rc)
    torch.cuda.synchronize()
    cur, refs, n_in = p, [], n
    for k, ((i, nx), m) in enumerate(zip(outs, npoints)):
        i, nx = i.cpu().numpy(), nx.cpu().numpy()
        assert ((i >= 0) & (i < n_in)).all(), f"{what}: stage {k} idx holds a non-index"
        r = O.fps(cur, m)
        assert np.array_equal(i, r), f"{what}: stage {k} idx, {int((i != r).sum())} differ"
        cur = O.gather_point(cur, r)
        assert np.array_equal(nx.view(np.int32), cur.view(np.int32)), f"{what}: stage {k} new_xyz"
        refs.append(r)
        n_in = m
    assert h.pn2_fault_status(0) == 0, what
    return refs


def _is_prefix(refs, b=slice(None)):
    return all(bool((r[b] == np.arange(r.shape[1])).all()) for r in refs)


@pytest.mark.parametrize("B", [1, 3])
def test_prefix_holds(env, picks, B):
    """n = 1024 -> 256 -> 64 -> 16 over sampler output: the check holds and the stages are
    copies (and the oracle's stages really are prefixes)."""
    refs = _chain(*env, picks[:B], [256, 64, 16], f"prefix B={B}")
    assert _is_prefix(refs)


@pytest.mark.parametrize("n,stages", [(1000, [250, 60, 7]), (130, [65, 2]), (200, [200, 50]),
                                      (257, [256]), (1024, [1024, 1024])],
                         ids=lambda v: str(v).replace(" ", ""))
def test_ragged_sizes(env, picks, n, stages):
    """Sizes that are no multiple of the workgroup, of a wave or of the check's packed pairs,
    odd and even m, a stage that takes its whole input (n = m), m = 2, a 257th point that only
    the second point slot of thread 0 covers. The first n picks of a sampling are a sampling."""
    refs = _chain(*env, picks[:2, :n], stages, f"ragged n={n} {stages}")
    assert _is_prefix(refs)


def _edited(picks, B=2):
    c = {}
    for pos in (1, 200):
        p = picks[:B].copy(); p[:, [pos, pos + 1]] = p[:, [pos + 1, pos]]; c[f"swap at {pos}"] = p
    p = picks[:B].copy(); p[:, [254, 255]] = p[:, [255, 254]]; c["swap at 255"] = p
    p = picks[:B].copy(); p[:, 100] = p[:, 50]; c["duplicate inside the prefix"] = p
    # (a copy of pick 200 at 700: a tie at step 200 that the reference's tie order gives to
    # point 700 -- only a check over every point of the cloud, not the prefix alone, sees it)
    p = picks[:B].copy(); p[:, 700] = p[:, 200]; c["duplicate beyond the prefix"] = p
    return c


@pytest.mark.parametrize("what", ["swap at 1", "swap at 200", "swap at 255",
                                  "duplicate inside the prefix", "duplicate beyond the prefix"])
def test_check_fails_fallback_samples(env, picks, what):
    """Edited sampler output: the check must fail and the stages run as samplers; the
    oracle's stage 0 is really not a prefix."""
    refs = _chain(*env, _edited(picks)[what], [256, 64, 16], what)
    assert not _is_prefix(refs[:1]), what


def test_non_finite_coordinate(env, picks):
    """A NaN coordinate: the check's finiteness test rejects the cloud, and the samplers keep
    the point's running min at 1e38 (a NaN distance never lowers it: the reference's
    min(d, temp), tf_sampling_g.cu:140, and the samplers' integer min over a NaN's positive
    bit pattern agree), so it is picked at every step from 1 on.
    (An infinite coordinate is a different matter and not this kernel's: once that point is
    the centre its own distance is inf - inf, a NaN the hardware generates with the sign bit
    set, which the integer min of every sampler of this library -- fps_v9_body and the hot-set
    stages alike, before and after this kernel -- takes for the smallest value, where the
    reference keeps 1e38. Measured on the one-launch and the two-launch build: both give
    0, 300, 1, 2, ... where the oracle gives 0, 300, 300, ...)"""
    p = picks[:2].copy()
    p[:, 300, 0] = np.nan
    refs = _chain(*env, p, [256, 64, 16], "NaN coordinate")
    assert (refs[0][:, 1:] == 300).all()


def test_all_points_equal(env):
    p = np.tile(np.array([[0.25, 0.5, 0.75]], np.float32), (2, 1024, 1)).reshape(2, 1024, 3)
    _chain(*env, p, [256, 64, 16], "all equal")


def test_lattice_ties(env):
    """Points of an integer lattice drawn with replacement: exact ties and duplicates at
    every step, at a full and at a ragged size (the fallback's wave-0 and four-wave bodies)."""
    g = np.stack(np.meshgrid(*[np.arange(8)] * 3, indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(3)
    p = np.stack([g[rng.integers(0, len(g), 1024)] for _ in range(2)]).astype(np.float32)
    _chain(*env, p, [256, 64, 16], "lattice 1024")
    _chain(*env, p[:, :700], [400, 100, 30], "lattice 700")  # (400 picks: past the LDS hand-over)
    _chain(*env, p[:, :100], [64, 20], "lattice 100")


def test_mixed_launch_verdicts_are_per_cloud(env, picks):
    """B = 4, clouds 1 and 3 fail the check, clouds 0 and 2 hold."""
    p = picks.copy()
    p[1, [10, 11]] = p[1, [11, 10]]
    p[3, 700] = p[3, 200]
    refs = _chain(*env, p, [256, 64, 16], "mixed")
    assert [_is_prefix(refs[:1], b) for b in range(4)] == [True, False, True, False]


def test_other_chain_paths_unchanged(env):
    """A chain whose first stage samples a raw cloud (2048 points: its own sampler launch, then
    the tail over its picks), and the single-stage 1024 -> 256 sampler (the hot-set stage)."""
    pkg, O, torch, dev = env
    x = pkg.synth.batch(range(31, 33), 2048, "scannet")[0]
    _chain(pkg, O, torch, dev, x, [1024, 256, 64], "raw 2048 chain")
    x = pkg.synth.batch(range(33, 35), 1024, "scannet")[0]
    idx, nx = pkg.tf_sampling.farthest_point_sample_and_gather(256, torch.from_numpy(x).to(dev))
    r = O.fps(x, 256)
    assert np.array_equal(idx.cpu().numpy(), r)
    assert np.array_equal(nx.cpu().numpy().view(np.int32), O.gather_point(x, r).view(np.int32))
    assert pkg._lib.lib().pn2_fault_status(0) == 0
