#!/usr/bin/env python3
"""Time the training-mode attention tail of the attention SA modules, forward plus backward with
gradients for x and all six Dense variables: the query / key / value projections, the reduction
and the max pool over nsample. New path: torch.ops.pn2.attn_kv_train (csrc/attn_train.hip: K and
V projected together, the reduction and its gradient on the interleaved rows, grad_x written
once and patched). Baseline: what the HIP ops offered before it, composed under autograd:

    q    = mlp_layer_train(x[..., 0, :], wq, bq, None, None, eps, False)
    k, v = mlp_layer_train(x, wk, bk, ...), mlp_layer_train(x, wv, bv, ...)
    att  = attn_reduce(q, k, v)                 (autograd: attn_reduce_grad)
    pmax = x.max(-2).values

at cfg3's four attention layers with B = 16:

    SA1   16,384 groups x 32 x  64
    SA2    4,096 groups x 32 x 128
    SA3    1,024 groups x 32 x 256
    SA4      256 groups x 32 x 512

    python tools/bench_attn_train.py [--repeats 7] [--iters 10] [--out summary.json]

Each shape runs in a child process of its own under `timeout`; a shape that fails stops the
run. Per shape: warm-up, then `repeats` timed windows of `iters` forward+backward passes per
side, the two sides alternating, timed with events on the stream; the median window and the
min-max of the windows are reported. `ranges_overlap` says whether the two sides' min-max ranges
overlap: where they do, the medians' order is not a measured gain. `new_calls_us` is the per-call
breakdown of the new path (each op alone, median of the same windows).

Peak allocated memory per side is torch.cuda.max_memory_allocated over one forward+backward
pass, after reset_peak_memory_stats, less the memory held before the pass (the inputs).

`out_equal` and `max_rel_grad_diff` compare the two sides: att and pmax must be bit-equal; the
gradients differ in the last bits of reordered fp32 sums.
"""
import json
import os
import statistics
import sys

from _timing import main, windows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = {"SA1": (16384, 32, 64), "SA2": (4096, 32, 128), "SA3": (1024, 32, 256),
          "SA4": (256, 32, 512)}
EPS = 1e-3
NAMES = ("x", "wq", "bq", "wk", "bk", "wv", "bv")


def one(name, repeats, iters):
    import torch
    import pn2hip
    ops = pn2hip.ops
    assert torch.cuda.is_available(), "bench_attn_train needs the MI355X"
    dev = torch.device("cuda:0")
    G, ns, C = SHAPES[name]
    g = torch.Generator().manual_seed(G + C)
    lim = (6.0 / (C + C)) ** 0.5
    leaf = lambda t: t.to(dev).requires_grad_(True)  # noqa: E731
    L = {"x": leaf(torch.rand(G, ns, C, generator=g) * 2 - 1)}
    for n in "qkv":
        L["w" + n] = leaf((torch.rand(C, C, generator=g) * 2 - 1) * lim)
        L["b" + n] = leaf(torch.rand(C, generator=g) * 0.2 - 0.1)
    leaves = [L[k] for k in NAMES]
    go = (torch.rand(G, C, generator=g) * 2 - 1).to(dev)
    gp = (torch.rand(G, C, generator=g) * 2 - 1).to(dev)

    def clear():
        for t in leaves:
            t.grad = None

    def new():
        clear()
        att, pmax = ops.attn_kv_train(*leaves, True)[:2]
        torch.autograd.backward([att, pmax], [go, gp])
        return att, pmax

    def parent():
        clear()
        x = L["x"]
        lin = lambda t, n: ops.mlp_layer_train(t, L["w" + n], L["b" + n], None, None, EPS, False)[0]  # noqa: E731
        att = ops.attn_reduce(lin(x[:, 0], "q")[None], lin(x, "k")[None], lin(x, "v")[None])[0]
        pmax = x.max(-2).values
        torch.autograd.backward([att, pmax], [go, gp])
        return att, pmax

    on = [t.detach().clone() for t in new()]
    gn = [t.grad.clone() for t in leaves]
    op = [t.detach().clone() for t in parent()]
    diffs = {}
    for nm, a, t in zip(NAMES, gn, leaves):
        scale = max(float(t.grad.abs().max()), 1e-6)
        diffs[nm] = float((a - t.grad).abs().max()) / scale
    del gn

    def peak(fn):
        clear()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    mem_n, mem_p = peak(new), peak(parent)
    tn, tp = windows(torch, [new, parent], repeats, iters)
    mn, mp = statistics.median(tn), statistics.median(tp)

    # the new path's two ops alone
    with torch.no_grad():
        d = [t.detach() for t in leaves]
        att, pmax, arg, q, kv = ops.attn_kv_train(*d, True)
        calls = {
            "attn_kv_train": lambda: ops.attn_kv_train(*d, True),
            "attn_kv_train_grad": lambda: ops.attn_kv_train_grad(go, gp, arg, d[0], d[1], d[3],
                                                                 d[5], q, kv, True)}
        per_call = {k: round(statistics.median(windows(torch, [fn], repeats, iters)[0]), 1)
                    for k, fn in calls.items()}

    print(json.dumps({
        "shape": name, "groups": G, "ns": ns, "C": C, "repeats": repeats, "iters": iters,
        "new_fwd_bwd_us": round(mn, 1), "parent_fwd_bwd_us": round(mp, 1),
        "new_min_max_us": [round(min(tn), 1), round(max(tn), 1)],
        "parent_min_max_us": [round(min(tp), 1), round(max(tp), 1)],
        "parent_over_new": round(mp / mn, 2), "lower_median": bool(mn < mp),
        "ranges_overlap": bool(max(tn) >= min(tp) and max(tp) >= min(tn)),
        "new_peak_MB": round(mem_n / 1e6, 1), "parent_peak_MB": round(mem_p / 1e6, 1),
        "new_calls_us": per_call,
        "out_equal": bool(torch.equal(on[0], op[0]) and torch.equal(on[1], op[1])),
        "max_rel_grad_diff": {k: float(f"{v:.3g}") for k, v in diffs.items()}}))


if __name__ == "__main__":
    main(__file__, SHAPES, one)
