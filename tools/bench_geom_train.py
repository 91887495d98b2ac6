#!/usr/bin/env python3
"""Time the training-mode geometry of the SA and FP modules, forward plus backward, on the fused
kernels with ordered-gather gradients (csrc/geom_train.hip: torch.ops.pn2.group_concat_train,
fp_apply_train) against the composition of the reference's ops that pointnet_util ran before
them, at the cfg2 SSG levels with B = 16:

    SA2..SA4   group_concat_train                     vs  group_point x 2, the subtraction and
                                                          torch.cat, with autograd (the grouping
                                                          gradient a float-atomic scatter)
    FP4..FP1   fp_apply_train                         vs  idw_weights, three_interpolate and
                                                          torch.cat, with autograd
    SA2_ns128  N 1024, C 32, M 256 with nsample 128

    python tools/bench_geom_train.py [--repeats 7] [--iters 10] [--out summary.json]

three_nn and the ball query are outside both sides: the clouds are synthetic ScanNet-like rooms
sampled down the SSG levels (8192 -> 1024 -> 256 -> 64 -> 16 points) with the product's own
sampler, and every level's idx comes from query_ball_point / three_nn on them, so the lists per
destination have the skew real layers have. The new side includes its inverse-index build, which
is also timed alone (the C entry point, events). Each shape runs in a child process of its own
under `timeout`; a shape that fails stops the run. Per shape: warm-up, then `repeats` timed
windows of `iters` forward+backward passes per side, the two sides alternating, timed with events
on the stream; the median window, the range and the peak of torch.cuda.max_memory_allocated over
one pass above the memory held before it are reported. The bar, on SA2 and FP4 (the two levels
with the most bytes): the new side's median window is no higher than the composition's, measured
in the same run. The small levels are bound by launches and are reported without a bar.
"""
import importlib
import json
import os
import statistics
import sys

from _timing import main, peak_delta, windows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B = 16
LEVELS = (8192, 1024, 256, 64, 16)  # points per cloud at l0 .. l4
# name -> ("sa", source level, C, nsample, radius) | ("fp", unknown level, C2, C1)
SHAPES = {
    "SA2": ("sa", 1, 64, 32, 0.2),
    "SA3": ("sa", 2, 128, 32, 0.4),
    "SA4": ("sa", 3, 256, 32, 0.8),
    "FP4": ("fp", 0, 128, 0),
    "FP3": ("fp", 1, 256, 64),
    "FP2": ("fp", 2, 256, 128),
    "FP1": ("fp", 3, 512, 256),
    "SA2_ns128": ("sa", 1, 32, 128, 0.4),
}
BARRED = ("SA2", "FP4")


def one(name, repeats, iters):
    import torch
    pkg = importlib.import_module("pointcloud-segmentation-attention_amd")
    import pn2hip
    ops = pn2hip.ops
    assert torch.cuda.is_available(), "bench_geom_train needs the MI355X"
    dev = torch.device("cuda:0")
    pu, tg, ti, ts = pkg.pointnet_util, pkg.tf_grouping, pkg.tf_interpolate, pkg.tf_sampling
    g = torch.Generator().manual_seed(7)
    rand = lambda *s: (torch.rand(*s, generator=g) * 2 - 1).to(dev)  # noqa: E731
    xyz = [torch.from_numpy(pkg.synth.batch(list(range(B)), LEVELS[0], "scannet")[0]).to(dev)]
    for n in LEVELS[1:]:
        xyz.append(ts.farthest_point_sample_and_gather(n, xyz[-1])[1])
    spec = SHAPES[name]
    res = {"shape": name, "B": B, "repeats": repeats, "iters": iters}
    if spec[0] == "sa":
        _, lvl, C, ns, radius = spec
        src, new_xyz = xyz[lvl], xyz[lvl + 1]
        N, M = LEVELS[lvl], LEVELS[lvl + 1]
        idx, _ = tg.query_ball_point(radius, ns, src, new_xyz)
        points = rand(B, N, C).requires_grad_(True)
        go = rand(B, M, ns, C + 3)
        keys, K, S = idx, N, M * ns
        res.update({"N": N, "C": C, "M": M, "nsample": ns})

        def new():
            points.grad = None
            ops.group_concat_train(src, points, new_xyz, idx, True, False).backward(go)

        def old():
            points.grad = None
            pu.group_concat(src, points, new_xyz, idx, ordered_grad=False)[0].backward(go)
        leaves = (points,)
    else:
        _, lvl, C2, C1 = spec
        n, m = LEVELS[lvl], LEVELS[lvl + 1]
        dist, idx = ti.three_nn(xyz[lvl], xyz[lvl + 1])
        p2 = rand(B, m, C2).requires_grad_(True)
        p1 = rand(B, n, C1).requires_grad_(True) if C1 else None
        go = rand(B, n, C2 + C1)
        keys, K, S = idx, m, 3 * n
        res.update({"n": n, "m": m, "C2": C2, "C1": C1})

        def clear():
            p2.grad = None
            if p1 is not None:
                p1.grad = None

        def new():
            clear()
            ops.fp_apply_train(dist, idx, p1, p2).backward(go)

        def old():
            clear()
            interp = ti.three_interpolate(p2, idx, ti.idw_weights(dist))
            (interp if p1 is None else torch.cat([interp, p1], dim=2)).backward(go)
        leaves = (p2,) if p1 is None else (p2, p1)

    # the two sides compute the same gradients (the order of the sums aside)
    new()
    got = [t.grad.clone() for t in leaves]
    old()
    diff = max(float((a - t.grad).abs().max()) for a, t in zip(got, leaves))
    counts = torch.bincount(keys.reshape(B, -1)[0].long(), minlength=K)
    res.update({"max_abs_grad_diff": diff, "slots_per_key_median_max": [
        int(counts.median()), int(counts.max())]})

    t_new, t_old = windows(torch, [new, old], repeats, iters)
    m_new, m_old = statistics.median(t_new), statistics.median(t_old)
    res.update({"new_fwd_bwd_us": round(m_new, 1), "old_fwd_bwd_us": round(m_old, 1),
                "new_min_max_us": [round(min(t_new), 1), round(max(t_new), 1)],
                "old_min_max_us": [round(min(t_old), 1), round(max(t_old), 1)],
                "old_over_new": round(m_old / m_new, 2),
                "new_peak_alloc_bytes": peak_delta(torch, new),
                "old_peak_alloc_bytes": peak_delta(torch, old)})
    if name in BARRED:
        res["no_slower"] = bool(m_new <= m_old)

    # the inverse-index build alone (the C entry point)
    L = importlib.import_module("pointcloud-segmentation-attention_amd._lib")
    lib, ptr = L.lib(), L.ptr
    size = int(lib.pn2_inverse_index_size(B, S, K))
    inv = torch.empty(size // 4, dtype=torch.int32, device=dev)
    kflat = keys.reshape(B, S).contiguous()

    def build():
        L.check(lib.pn2_inverse_index_build(ptr(kflat), B, S, K, ptr(inv), size,
                                            L.stream_of(kflat)), "inverse_index_build")
    (t_build,) = windows(torch, [build], repeats, iters)
    res["index_build_us"] = round(statistics.median(t_build), 1)
    res["index_bytes"] = size
    print(json.dumps(res))


if __name__ == "__main__":
    main(__file__, SHAPES, one)
