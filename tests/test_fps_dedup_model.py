"""The distinct-points rule of the culled sampler ("Distinct points") on the
CPU model: sampling over the representatives only -- of the points with the same coordinate
bits, the one with the smallest tie key (k mod 512, k div 512) -- gives the picks of the
brute-force sampler over the whole cloud (tools/model_fps_cull.py: fps_exact, the reference's
fp32 arithmetic and tie order). Duplicate-heavy clouds, N about 1,024, M = 128."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "tools"))
import model_fps_cull as model  # noqa: E402

N, M = 1024, 128
FRACS = [0.5, 0.7, 0.8, 0.85, 0.9, 0.93, 0.95, 0.97, 0.98, 0.99, 0.995]


def _with_replacement(seed, n=N, distinct=None):
    rng = np.random.default_rng(seed)
    u = rng.random((distinct or n, 3)).astype(np.float32)
    return u[rng.integers(0, len(u), n)]


def _key_decides():
    """Every point twice, the copy 600 indices later: the copy of k in [424, 512) sits at
    k' = k + 600 in [1024, 1112) with k' mod 512 < k mod 512, so there the later index is the
    representative and the reference picks it."""
    rng = np.random.default_rng(7)
    u = rng.random((600, 3)).astype(np.float32)
    return np.concatenate([u, u])


def _signed_zero():
    x = _with_replacement(11)
    x[5] = x[700] = (np.float32(0.5), np.float32(0.0), np.float32(0.25))
    x[700, 1] = np.float32(-0.0)  # equal as floats, different bits: two groups
    return x


CLOUDS = {
    "with_replacement": lambda: _with_replacement(1),
    "few_distinct": lambda: _with_replacement(2, distinct=100),  # M > the distinct points
    "key_decides": _key_decides,
    "copies_of_point_0": lambda: np.concatenate([_with_replacement(3)[:1]] * 40
                                                + [_with_replacement(3)[:N - 40]]),
    "all_identical": lambda: np.tile(np.array([[0.25, 0.5, 0.75]], np.float32), (N, 1)),
    "signed_zero": _signed_zero,
}


@pytest.fixture(scope="module")
def exact():
    return {name: model.fps_exact(make(), M) for name, make in CLOUDS.items()}


def test_representatives_are_the_smallest_keys():
    x = _key_decides()
    rep = model.representatives(x)
    assert len(rep) == 600 and rep[0] == 0
    # copies at k and k + 600: the later index stands for the group where its key is smaller
    late = rep[rep >= 600] - 600
    assert len(late) > 0 and (model.key(late + 600) < model.key(late)).all()
    assert set(late) == {k for k in range(600) if model.key(k + 600) < model.key(k)}
    z = _signed_zero()
    nan = np.array([0x7FC00001], np.uint32).view(np.float32)[0]
    z[9] = z[600] = (nan, np.float32(0.1), np.float32(0.2))  # the same NaN bits: one group
    z[601] = (-nan, np.float32(0.1), np.float32(0.2))        # another NaN: its own group
    rz = set(model.representatives(z).tolist())
    assert {5, 700} <= rz, "+0.0 and -0.0 differ in bits: not merged"
    assert 9 in rz and 600 not in rz and 601 in rz, "NaNs merge only when bit-identical"


@pytest.mark.parametrize("name", list(CLOUDS))
def test_argmax_over_representatives_is_the_reference(name, exact):
    """Brute force over the representatives alone, with their own indices' keys."""
    x = CLOUDS[name]()
    rep = model.representatives(x)
    keys = model.key(rep)
    t = np.full(len(rep), model.INIT, np.float32)
    out = [0]
    for _ in range(M - 1):
        t = np.minimum(t, model.d2(x[rep], x[out[-1]]))
        cand = np.flatnonzero(t == t.max())
        out.append(int(rep[cand[np.argmin(keys[cand])]]))
    assert np.array_equal(np.array(out), exact[name]), name


@pytest.mark.parametrize("name", list(CLOUDS))
def test_schedule_over_representatives_is_exact(name, exact):
    x = CLOUDS[name]()
    picks, st = model.simulate(x, M, 64, 64, FRACS, dedup=True)
    assert st["points"] == len(model.representatives(x))
    assert np.array_equal(picks, exact[name]), name
