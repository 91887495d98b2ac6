"""GPU: the bits of the training layers' outputs, pinned.

The other GPU tests compare against float64 within a tolerance and check that two runs of one
build agree; neither notices a summation order that changes between two builds. This one does:
seeded float32 inputs (numpy.random.default_rng, nothing from torch's generators), every output
of the torch.ops.pn2 training ops below, and the SHA-256 of each output's bytes against
tests/golden/train_bits.json. The kernels have fixed grids and fixed orders, so the digests are
a function of the inputs alone.

The JSON names the commit it was recorded at. It is regenerated only by running this file as a
script on the GPU, at a commit whose results are the ones to keep:

    python tests/test_gpu_train_bits.py --record --commit <hash> [--out FILE]

Each case is the smallest shape at which its code path can go wrong (SLAB = PN2_BN_BLOCK_ROWS
rows per stage-1 partial, PG = PN2_BN_POOL_BLOCK_GROUPS groups per pooled partial).
"""
import hashlib
import importlib
import json
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import PKG_NAME  # noqa: E402
from support import gpu_marks  # noqa: E402

pytestmark = gpu_marks

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_bits.json")
EPS = 1e-3
SLAB = 1024
PG = 128
T, F = True, False

# (kind, shape, flags): see run_case
CASES = (
    # 10 stats blocks (stage 2's lanes 0 and 1 stride), two channel tiles with the second
    # partial, a 37-row tail that is no multiple of 8; (F, F) is the path that does not read y
    [("mlp", (9 * SLAB + 37, 16, 40), (bn, relu)) for bn, relu in ((T, T), (T, F), (F, T), (F, F))]
    + [("mlp", (1, 16, 32), (T, T))]
    # groups layout: 9 pool-backward blocks; gpt clamped to 1 with ns no multiple of 8
    + [("pool", (g, ns, 8, 40), f) for g, ns in ((8 * PG + 13, 16), (5, 33))
       for f in ((T, T), (F, F))]
    # split layout: just over kPoolSplit; two apply chunks, the second partial
    + [("pool", (3, ns, 8, 40), f) for ns in (65, 300) for f in ((T, T), (F, T))]
    + [("bn", (9 * SLAB + 37, 40), (relu,)) for relu in (T, F)]
    # col_sum over 9,600 rows in 10 blocks; then the generic reduction and the scatter with a
    # pooled gradient
    + [("attn", (600, 16, 8), (T,)), ("attn", (600, 16, 8), (F,)), ("attn", (37, 5, 8), (T,))]
)


def case_id(case):
    kind, shape, flags = case
    return kind + "-" + "x".join(map(str, shape)) + "-" + "".join("FT"[f] for f in flags)


def _inputs(case):
    """Seeded float32 arrays of one case; the seed is the case's position in CASES."""
    kind, shape, flags = case
    rng = np.random.default_rng(1000 + CASES.index(case))
    u = lambda lo, hi, *s: rng.uniform(lo, hi, s).astype(np.float32)  # noqa: E731

    def gamma_beta(c):  # gamma of either sign: bn may be decreasing in y
        mag, sign = u(0.5, 1.5, c), u(-1, 1, c)
        return np.where(sign < 0, -mag, mag).astype(np.float32), u(-0.2, 0.2, c)

    if kind in ("mlp", "pool"):
        *lead, cin, cout = shape
        lim = float(np.sqrt(6.0 / (cin + cout)))
        p = {"x": u(-1, 1, *lead, cin), "w": u(-lim, lim, cin, cout), "b": u(-0.1, 0.1, cout)}
        p["gamma"], p["beta"] = gamma_beta(cout) if flags[0] else (None, None)
        p["go"] = u(-1, 1, *lead[:1], cout)
    elif kind == "bn":
        rows, c = shape
        p = {"x": u(-1, 1, rows, c), "go": u(-1, 1, rows, c)}
        p["gamma"], p["beta"] = gamma_beta(c)
    else:
        g, ns, c = shape
        lim = float(np.sqrt(3.0 / c))
        p = {"x": u(-1, 1, g, ns, c), "go": u(-1, 1, g, c), "gp": u(-1, 1, g, c)}
        for n in "qkv":
            p["w" + n], p["b" + n] = u(-lim, lim, c, c), u(-0.1, 0.1, c)
    return p


def run_case(ops, torch, dev, case):
    """{output name: SHA-256 of its bytes} for the forward op and its gradient op."""
    kind, shape, flags = case
    p = {k: None if v is None else torch.from_numpy(v).to(dev) for k, v in _inputs(case).items()}
    if kind in ("mlp", "pool"):
        bn, relu = flags
        pooled = kind == "pool"
        fwd = ops.mlp_layer_train_pool if pooled else ops.mlp_layer_train
        res = fwd(p["x"], p["w"], p["b"], p["gamma"], p["beta"], EPS, relu)
        names = ("out", "y", "mean", "var") + (("arg",) if pooled else ())
        outs = dict(zip(names, res))
        stats = (outs["mean"], outs["var"]) if bn else (None, None)
        tail = (p["x"], p["w"], outs["y"], *stats, p["gamma"], p["beta"], EPS, relu, True)
        grads = (ops.mlp_layer_train_pool_grad(p["go"], outs["arg"], *tail) if pooled
                 else ops.mlp_layer_train_grad(p["go"], *tail))
        outs.update(zip(("grad_x", "grad_w", "grad_b", "grad_gamma", "grad_beta"), grads))
    elif kind == "bn":
        (relu,) = flags
        outs = dict(zip(("out", "mean", "var"),
                        ops.bn_train(p["x"], p["gamma"], p["beta"], EPS, relu)))
        grads = ops.bn_train_grad(p["go"], p["x"], outs["mean"], outs["var"], p["gamma"], p["beta"],
                                  EPS, relu)
        outs.update(zip(("grad_x", "grad_gamma", "grad_beta"), grads))
    else:
        (add_max,) = flags
        res = ops.attn_kv_train(p["x"], p["wq"], p["bq"], p["wk"], p["bk"], p["wv"], p["bv"],
                                add_max)
        outs = dict(zip(("att", "pmax", "arg", "q", "kv"), res))
        grads = ops.attn_kv_train_grad(p["go"], p["gp"] if add_max else None, outs["arg"], p["x"],
                                       p["wq"], p["wk"], p["wv"], outs["q"], outs["kv"], True)
        outs.update(zip(("grad_x", "grad_wq", "grad_bq", "grad_wk", "grad_bk", "grad_wv",
                         "grad_bv"), grads))
    return {k: hashlib.sha256(np.ascontiguousarray(v.cpu().numpy()).tobytes()).hexdigest()
            for k, v in outs.items()}


@pytest.fixture(scope="module")
def env():
    import torch
    pkg = importlib.import_module(PKG_NAME)
    return pkg._torch_ops.ops(), torch, torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_covers_the_cases(golden):
    assert len(golden["commit"]) == 40
    assert sorted(golden["digests"]) == sorted(map(case_id, CASES))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_bits(env, golden, case):
    got = run_case(*env, case)
    want = golden["digests"][case_id(case)]
    assert sorted(got) == sorted(want)
    changed = [k for k in got if got[k] != want[k]]
    assert not changed, (f"{case_id(case)}: bits differ from commit {golden['commit'][:12]} "
                         f"in {changed}")


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", action="store_true", required=True)
    ap.add_argument("--commit", required=True, help="the commit whose build is being recorded")
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args()
    import torch
    the_ops = importlib.import_module(PKG_NAME)._torch_ops.ops()
    digests = {case_id(c): run_case(the_ops, torch, torch.device("cuda:0"), c) for c in CASES}
    with open(a.out, "w") as f:
        json.dump({"commit": a.commit, "digests": digests}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded", len(digests), "cases at", a.commit, "->", a.out)
