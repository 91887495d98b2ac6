#!/usr/bin/env python3
"""Time the last layer of a set-abstraction MLP in training mode together with its max pool
over nsample, forward plus backward: the fused op (torch.ops.pn2.mlp_layer_train_pool,
pn2_bn_act_pool_fwd / _bwd in csrc/mlp_train.hip) against the path it replaces
(torch.ops.pn2.mlp_layer_train followed by .max(dim=-2).values under autograd), at the last SA
layers of cfg2 with B = 16:

    SA1 conv2   16,384 groups x 32    32 ->  64
    SA2 conv2    4,096 groups x 32    64 -> 128
    SA4 conv2      256 groups x 32   256 -> 512

    python tools/bench_mlp_train_pool.py [--repeats 7] [--iters 10] [--out summary.json]

Each shape runs in a child process of its own under `timeout`; a shape that fails stops the
run. Per shape: warm-up, then `repeats` timed windows of `iters` forward+backward passes per
side, the two sides alternating, timed with events on the stream; the median window and the
min-max of the windows are reported. Both sides run batch norm and ReLU and compute gradients
for the input, weight, gamma and beta. `ranges_overlap` says whether the two sides' min-max
ranges overlap: where they do, the medians' order is not a measured gain.

Peak allocated memory per side is torch.cuda.max_memory_allocated over one forward+backward
pass, after reset_peak_memory_stats, less the memory held before the pass (the inputs).

`out_equal` and `max_rel_grad_diff` compare the two sides: the pooled outputs must be bit-equal;
the gradients differ in the last bits of reordered fp32 sums.
"""
import importlib
import json
import os
import statistics
import sys

from _timing import main, windows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = {"SA1_conv2": (16384, 32, 32, 64), "SA2_conv2": (4096, 32, 64, 128),
          "SA4_conv2": (256, 32, 256, 512)}
EPS = 1e-3


def one(name, repeats, iters):
    import torch
    import pn2hip
    ops = pn2hip.ops
    assert torch.cuda.is_available(), "bench_mlp_train_pool needs the MI355X"
    dev = torch.device("cuda:0")
    groups, ns, cin, cout = SHAPES[name]
    g = torch.Generator().manual_seed(groups + cin)
    lim = (6.0 / (cin + cout)) ** 0.5
    leaf = lambda t: t.to(dev).requires_grad_(True)  # noqa: E731
    x = leaf(torch.rand(groups, ns, cin, generator=g) * 2 - 1)
    w = leaf((torch.rand(cin, cout, generator=g) * 2 - 1) * lim)
    gamma = leaf(torch.rand(cout, generator=g) + 0.5)
    beta = leaf(torch.rand(cout, generator=g) * 0.4 - 0.2)
    go = (torch.rand(groups, cout, generator=g) * 2 - 1).to(dev)
    leaves = (x, w, gamma, beta)

    def clear():
        for t in leaves:
            t.grad = None

    def fused():
        clear()
        out = ops.mlp_layer_train_pool(x, w, None, gamma, beta, EPS, True)[0]
        out.backward(go)
        return out

    def parent():
        clear()
        out = ops.mlp_layer_train(x, w, None, gamma, beta, EPS, True)[0].max(dim=-2).values
        out.backward(go)
        return out

    of = fused().detach().clone()
    gf = [t.grad.clone() for t in leaves]
    op = parent().detach().clone()
    diffs = {}
    for nm, a, t in zip(("x", "w", "gamma", "beta"), gf, leaves):
        scale = max(float(t.grad.abs().max()), 1e-6)
        diffs[nm] = float((a - t.grad).abs().max()) / scale
    del gf

    def peak(fn):
        clear()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    mem_f, mem_p = peak(fused), peak(parent)
    tf_, tp = windows(torch, [fused, parent], repeats, iters)
    mf, mp = statistics.median(tf_), statistics.median(tp)
    print(json.dumps({
        "shape": name, "groups": groups, "ns": ns, "cin": cin, "cout": cout, "repeats": repeats,
        "iters": iters, "fused_fwd_bwd_us": round(mf, 1), "parent_fwd_bwd_us": round(mp, 1),
        "fused_min_max_us": [round(min(tf_), 1), round(max(tf_), 1)],
        "parent_min_max_us": [round(min(tp), 1), round(max(tp), 1)],
        "parent_over_fused": round(mp / mf, 2), "no_slower": bool(mf <= mp),
        "ranges_overlap": bool(max(tf_) >= min(tp) and max(tp) >= min(tf_)),
        "fused_peak_MB": round(mem_f / 1e6, 1), "parent_peak_MB": round(mem_p / 1e6, 1),
        "out_equal": bool(torch.equal(of, op)),
        "max_rel_grad_diff": {k: float(f"{v:.3g}") for k, v in diffs.items()}}))


if __name__ == "__main__":
    main(__file__, SHAPES, one)
