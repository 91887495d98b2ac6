"""CPU: the reference of tests/test_gpu_model_train.py (tests/model_train_ref.py) checked without
a GPU, so that the yardstick the whole-model gradient test leans on is itself pinned.

  decisions from the float64 forward   `plain` below is the straightforward training-mode model
                                       (torch.relu, .max(dim), torch.nn.functional.batch_norm with
                                       training=True, F.cross_entropy, the oracle's fps / ball
                                       query / three_nn) and writes down the choices it made. Fed
                                       that record, the frozen reference is the same function:
                                       outputs and gradients agree in float64 to rounding.
  gradcheck                            torch.autograd.gradcheck of the frozen reference on a tiny
                                       instance: nothing in it is detached by accident, and with
                                       the decisions frozen it is smooth.
  the yardstick is meaningful          float32 against float64 on the full-size cases: finite, and
                                       an error above 0 for every tensor but the gradient of a
                                       conv bias under batch norm (the batch mean absorbs it).
                                       `pytest -s` prints the table that the GPU test's docstring
                                       quotes.
"""
import importlib

import numpy as np
import pytest
import torch

import model_train_ref as R
from conftest import PKG_NAME

F = torch.nn.functional


def plain(spec, P, xyz, feats, labels, smpw, seed, O, dt=torch.float64):
    """The straightforward model in dtype dt on leaves P; returns (outputs as R.run returns them,
    without "inter", and the record of its own discrete choices)."""
    B = xyz.shape[0]
    rec = {"centres": [], "group_idx": [], "nn": [], "layers": [], "attn_arg": [], "seed": seed,
           "keep_prob": spec["keep_prob"]}
    stats = {}
    bsel = torch.arange(B)[:, None, None]

    def batch_norm(y, scope):
        y2 = y.reshape(-1, y.shape[-1])
        stats[scope] = (y2.mean(0).detach(), y2.var(0, unbiased=False).detach())
        return F.batch_norm(y2, None, None, P[f"{scope}/gamma"], P[f"{scope}/beta"], True, 0.0,
                            R.EPS).reshape(y.shape)

    def mlp(a, scopes, pool=False):
        for s in scopes:
            a = torch.einsum("...i,io->...o", a, P[f"{s}/weights"][0, 0]) + P[f"{s}/biases"]
            a = torch.relu(batch_norm(a, f"{s}/bn"))
            arg = None
            if pool and s == scopes[-1]:
                a, arg = a.max(dim=2)
            rec["layers"].append({"mask": a.detach() > 0, "arg": arg})
        return a

    coords, pts = [xyz.numpy()], [feats]
    for L in spec["sa"]:
        cur = coords[-1]
        centres = O.gather_point(cur, O.fps(cur, L["npoint"]))
        idx = torch.from_numpy(O.ball_query(cur, centres, L["radius"], L["nsample"])[0]).long()
        rec["centres"].append(torch.from_numpy(centres))
        rec["group_idx"].append(idx)
        rel = torch.from_numpy(cur).to(dt)[bsel, idx] - torch.from_numpy(centres).to(dt)[:, :, None]
        grouped = rel if pts[-1] is None else torch.cat([rel, pts[-1][bsel, idx]], -1)
        scopes = [f"{L['scope']}/conv{i}" for i in range(len(L["mlp"]))]
        X = mlp(grouped, scopes, pool=L["kind"] == "max")
        if L["kind"] != "max":
            base = f"{L['scope']}/ScannetAttentionLayer"
            def lin(d, x):
                return F.linear(x, P[f"{base}/{d}/kernel"].T, P[f"{base}/{d}/bias"])
            Bm, M, ns, C = X.shape
            q = lin("dense", X[:, :, 0, :]).reshape(Bm, M, C // 4, 4)
            k = lin("dense_1", X).reshape(Bm, M, C // 4, ns, 4)
            v = lin("dense_2", X).reshape(Bm, M, C // 4, ns, 4)
            a = torch.softmax(torch.einsum("bmhd,bmhnd->bmhn", q, k) * 0.5, dim=-1)
            out = batch_norm(torch.einsum("bmhn,bmhnd->bmhd", a, v).reshape(Bm, M, C),
                             f"{L['scope']}/{L['scope']}")
            mx, arg = X.max(dim=2)
            rec["attn_arg"].append(arg)
            X = out + mx if L["kind"] == "attn_pool" else out
        coords.append(centres)
        pts.append(X)
    for j, L in enumerate(spec["fp"]):
        k = len(spec["sa"]) - 1 - j
        dist, nidx = O.three_nn(coords[k], coords[k + 1])
        dist, nidx = torch.from_numpy(dist), torch.from_numpy(nidx).long()
        rec["nn"].append((dist, nidx))
        inv = 1.0 / torch.clamp(dist.to(dt), min=1e-10)
        w = inv / inv.sum(-1, keepdim=True)
        near = pts[k + 1][bsel, nidx]  # (B, n, 3, C)
        interp = (w[..., 0:1] * near[:, :, 0] + w[..., 1:2] * near[:, :, 1]
                  + w[..., 2:3] * near[:, :, 2])
        a = interp if pts[k] is None else torch.cat([interp, pts[k]], -1)
        pts[k] = mlp(a, [f"{L['scope']}/conv_{i}" for i in range(len(L["mlp"]))])
    fc1 = mlp(pts[0], ["fc1"])
    keep = torch.from_numpy(R.dropout_keep(fc1.numel(), spec["keep_prob"], seed)).reshape(fc1.shape)
    net = torch.where(keep, fc1 / spec["keep_prob"], torch.zeros((), dtype=dt))
    logits = net @ P["fc2/weights"][0, 0] + P["fc2/biases"]
    rec["layers"].append({"mask": logits.detach() > 0, "arg": None})
    C = logits.shape[-1]
    ce = F.cross_entropy(logits.reshape(-1, C), labels.reshape(-1).long(), reduction="none")
    w = smpw.reshape(-1).to(dt)
    loss = (w * ce).sum() / int((w != 0).sum())
    return {"logits": logits, "feats": fc1, "loss": loss, "stats": stats}, rec


def plain_run(spec, init, xyz, feats, labels, smpw, seed, O):
    P = R.leaves_of(spec, init, torch.float64)
    f = None if feats is None else feats.double().requires_grad_(True)
    out, rec = plain(spec, P, xyz, f, labels, smpw, seed, O)
    out["loss"].backward()
    out["grads"] = {n: torch.zeros_like(p) if p.grad is None else p.grad for n, p in P.items()}
    out["grad_feats"] = None if f is None else f.grad
    return {k: v.detach() if isinstance(v, torch.Tensor) else v for k, v in out.items()}, rec


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module(PKG_NAME)


_full = {}


def full_case(pkg, orc, name):
    """The full-size case: the plain model's float64 run, and the frozen reference on the plain
    model's record in float64 and float32. Computed once per case."""
    if name not in _full:
        orc.set_threads(16)
        spec, xyz, feats, labels, smpw = R.case_inputs(pkg, name)
        init = R.store_init(pkg, spec)
        p64, rec = plain_run(spec, init, xyz, feats, labels, smpw, R.DROPOUT_SEED, orc)
        r64 = R.run(spec, init, xyz, feats, labels, smpw, rec, torch.float64)
        r32 = R.run(spec, init, xyz, feats, labels, smpw, rec, torch.float32)
        _full[name] = (spec, p64, r64, r32)
    return _full[name]


def compared(spec, out):
    """name -> tensor of everything the GPU test compares."""
    d = {"logits": out["logits"], "feats": out["feats"], "loss": out["loss"]}
    if out["grad_feats"] is not None:
        d["grad input features"] = out["grad_feats"]
    for s in R.bn_scopes(spec):
        d[f"{s} batch mean"], d[f"{s} batch variance"] = out["stats"][s]
    for n in R.leaf_names(spec):
        d[f"grad {n}"] = out["grads"][n]
    return d


NEAR_ZERO = 1e-11  # of a tensor's largest magnitude: see same()


def same(a, b, what):
    """Equal in float64 to rounding: rtol 1e-12 per element, plus NEAR_ZERO of the tensor's
    largest magnitude, because rtol alone cannot hold the elements that cancellation leaves near
    0. The two models add in different orders (einsum and F.batch_norm against matmul and
    explicit means) through up to 31 layers with a batch norm each. Measured, largest
    |frozen - plain| / max |plain| over all compared tensors: 1.6e-12 (case a, feats), 1.5e-13
    (case b), 1.6e-14 (case c), 1.6e-14 (the tiny instances); NEAR_ZERO = 1e-11 leaves a factor 6."""
    torch.testing.assert_close(a, b, rtol=1e-12, atol=NEAR_ZERO * float(b.abs().max()),
                               msg=lambda m: f"{what}: {m}")


def check_frozen_equals_plain(spec, p64, r64):
    got, want = compared(spec, r64), compared(spec, p64)
    assert sorted(got) == sorted(want)
    noise = {f"grad {n}": f"grad {m}" for n, m in R.absorbed(spec).items()}
    for k in want:
        assert torch.isfinite(want[k]).all(), k
        if k in noise:
            # mathematically 0 (a batch mean absorbs it): both are rounding noise, held against
            # the gradient of the same layer's weights or gamma. Measured, largest noise / scale:
            # 2.2e-12 (case a, layer1/conv0/biases: sums over 65,536 rows), below 1e-14 elsewhere
            scale = float(want[noise[k]].abs().max())
            assert scale > 0 and float(got[k].abs().max()) <= NEAR_ZERO * scale, k
            assert float(want[k].abs().max()) <= NEAR_ZERO * scale, k
        else:
            same(got[k], want[k], k)
    assert sorted(r64["grads"]) == sorted(R.leaf_names(spec))


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_frozen_reference_is_the_plain_model(pkg, orc, name):
    spec, p64, r64, _ = full_case(pkg, orc, name)
    check_frozen_equals_plain(spec, p64, r64)
    # the plain model really took its max and its ReLU: something is masked, something is not
    assert float(r64["loss"]) > 0
    assert float(r64["grads"]["fc2/biases"].abs().max()) > 0


TINY = R.make_spec(3, [("s1", 16, 0.45, 4, (6, 8), "max"), ("s2", 4, 0.9, 4, (8, 8), "attn_pool")],
                   [("f1", (8, 6)), ("f2", (8, 5))], 6, 3)
TINY_PLAIN = R.make_spec(0, [("s1", 16, 0.45, 4, (6, 8), "max"), ("s2", 4, 0.9, 4, (8, 8), "attn")],
                         [("f1", (8, 6)), ("f2", (8, 5))], 6, 3)


def tiny_inputs(spec):
    # 64 points as two clouds of 32, so that the batch index is part of what is checked
    g = torch.Generator().manual_seed(64)
    xyz = torch.rand(2, 32, 3, generator=g)
    feats = torch.rand(2, 32, spec["cin"], generator=g) * 2 - 1 if spec["cin"] else None
    labels, smpw = R.targets(2, 32, spec["num_class"], seed=3)
    return xyz, feats, labels, smpw


@pytest.mark.parametrize("spec", [TINY, TINY_PLAIN], ids=["features", "no-features"])
def test_tiny_instance_frozen_equals_plain_and_gradcheck(orc, spec):
    """Two SA and two FP levels, widths <= 8, 64 points, nsample 4, variables away from their
    initialisers (random_init): the frozen reference equals the plain model, and gradcheck passes
    on it with the decisions frozen (logits and the fc1 output as functions of every leaf and of
    the input features)."""
    xyz, feats, labels, smpw = tiny_inputs(spec)
    init = R.random_init(spec, seed=8)
    p64, rec = plain_run(spec, init, xyz, feats, labels, smpw, 99, orc)
    r64 = R.run(spec, init, xyz, feats, labels, smpw, rec, torch.float64)
    check_frozen_equals_plain(spec, p64, r64)
    names = R.leaf_names(spec)
    P = R.leaves_of(spec, init, torch.float64)
    f = None if feats is None else feats.double().requires_grad_(True)

    def fn(*leaves):
        Q = dict(zip(names, leaves))
        out = R.forward(spec, Q, xyz, leaves[len(names)] if f is not None else None, rec,
                        torch.float64)
        return out["logits"], out["feats"]

    args = tuple(P[n] for n in names) + ((f,) if f is not None else ())
    # the instance with input features and the attention + pooling level gets the full
    # gradcheck (every entry of the Jacobian: 576 backward passes); the other one the fast
    # mode, one random projection of the Jacobian per side
    assert torch.autograd.gradcheck(fn, args, eps=1e-6, atol=1e-6, rtol=1e-4,
                                    fast_mode=spec is not TINY)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_fp32_yardstick_is_meaningful(pkg, orc, name):
    spec, _, r64, r32 = full_case(pkg, orc, name)
    c64, c32 = compared(spec, r64), compared(spec, r32)
    exact_zero = {f"grad {n}" for n in R.bias_under_bn(spec)}
    assert exact_zero and "grad fc2/biases" not in exact_zero
    print(f"\ncase ({name}): max |fp32 - f64|  /  max |f64|")
    for k in c64:
        assert torch.isfinite(c32[k]).all() and torch.isfinite(c64[k]).all(), k
        err = float((c32[k].double() - c64[k]).abs().max())
        print(f"  {k:58s} {err:9.3g}  {float(c64[k].abs().max()):9.3g}")
        if k in exact_zero:
            # the float64 gradient is rounding noise around 0, far below any other gradient
            assert float(c64[k].abs().max()) < 1e-9, k
        else:
            assert err > 0, k
            assert float(c64[k].abs().max()) > 0, k
