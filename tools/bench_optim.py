#!/usr/bin/env python3
"""Time what a training step runs after the gradients exist (csrc/optim.hip, train.py):

    adam      one optimiser step over the full pointnet2_sem_seg variable set (the 90 variables of
              a trainable store after one forward, random gradients): train.AdamOptimizer.step
              (torch.ops.pn2.adam_step, ceil(90 / 64) = 2 launches) next to
              torch.optim.Adam(foreach=True) and torch.optim.Adam(fused=True) on copies of the
              same variables and gradients
    metrics   torch.ops.pn2.seg_confusion + torch.ops.pn2.mean_iou on 16 x 8192 rows, C = 21

    python tools/bench_optim.py [--repeats 7] [--iters 20] [--out summary.json]

The three optimisers do not compute the same update (TF's epsilon-hat form against torch's), so
this compares cost, not results; no bar is set. Each shape runs in a child process of its own
under `timeout`; a shape that fails stops the run. Per shape: warm-up, then `repeats` timed
windows of `iters` calls per candidate, the candidates alternating, timed with events on the
stream (so a candidate bound by its host-side launches is charged for them); the median window
and the range are reported. For `adam` the C entry point alone is timed too, with the bytes the
update has to move (16 read and 12 written per element) over that time.
"""
import importlib
import json
import os
import statistics
import sys

from _timing import main, summary, windows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS, NCLASS = 16 * 8192, 21
SHAPES = ("adam", "metrics")


def one(name, repeats, iters):
    import torch
    pkg = importlib.import_module("pointcloud-segmentation-attention_amd")
    import pn2hip
    ops = pn2hip.ops
    assert torch.cuda.is_available(), "bench_optim needs the MI355X"
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(7)
    res = {"shape": name, "repeats": repeats, "iters": iters}
    if name == "adam":
        store = pkg.tf_util.ParamStore(seed=0).trainable(dev)
        xyz = torch.from_numpy(pkg.synth.batch([0, 1], 1024, "scannet")[0]).to(dev)
        pkg.pointnet2_sem_seg.get_model(xyz, True, NCLASS, params=store)
        params = list(store.parameters())
        grads = [(torch.rand(p.shape, generator=g) * 2e-2 - 1e-2).to(dev) for p in params]
        for p, gr in zip(params, grads):
            p.grad = gr

        def copies():
            out = [p.detach().clone().requires_grad_(True) for p in params]
            for c, gr in zip(out, grads):
                c.grad = gr
            return out

        ours = pkg.train.AdamOptimizer(store)
        foreach = torch.optim.Adam(copies(), lr=1e-3, foreach=True)
        fused = torch.optim.Adam(copies(), lr=1e-3, fused=True)
        fns = {"pn2_adam_optimizer": ours.step, "torch_adam_foreach": foreach.step,
               "torch_adam_fused": fused.step}
        times = windows(torch, list(fns.values()), repeats, iters)
        n = sum(p.numel() for p in params)
        L = importlib.import_module("pointcloud-segmentation-attention_amd._lib")
        res.update({"variables": len(params), "elements": n,
                    "launches": -(-len(params) // L.PN2_ADAM_SLOTS)})
        for k, t in zip(fns, times):
            res[k] = summary(t)
        med = {k: res[k]["us"] for k in fns}
        res["fused_over_ours"] = round(med["torch_adam_fused"] / med["pn2_adam_optimizer"], 2)
        res["foreach_over_ours"] = round(med["torch_adam_foreach"] / med["pn2_adam_optimizer"], 2)
        # the C entry point alone
        ms = [torch.zeros_like(p) for p in params]
        vs = [torch.zeros_like(p) for p in params]
        tab = (L.AdamSlot * len(params))(*[
            L.AdamSlot(p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel())
            for p, gr, m, v in zip(params, grads, ms, vs)])
        st = L.stream_of(params[0])

        def entry():
            L.check(L.lib().pn2_adam_step(tab, len(params), 1e-3, 0.9, 0.999, 1e-8, st),
                    "adam_step")

        (t,) = windows(torch, [entry], repeats, iters)
        us = statistics.median(t)
        res["entry_point"] = {"us": round(us, 1), "bytes": 28 * n,
                              "GBps": round(28 * n / us / 1e3, 1)}
    else:
        labels = torch.randint(0, NCLASS, (ROWS,), generator=g, dtype=torch.int32).to(dev)
        pred = torch.randint(0, NCLASS, (ROWS,), generator=g, dtype=torch.int32).to(dev)
        cm = torch.zeros(NCLASS, NCLASS, dtype=torch.int64, device=dev)
        counts = torch.zeros(2, dtype=torch.int64, device=dev)
        metrics = pkg.train.SegMetrics(NCLASS, device=dev)

        def both():
            ops.seg_confusion(labels, pred, cm, counts)
            ops.mean_iou(cm)

        def confusion():
            ops.seg_confusion(labels, pred, cm, counts)

        def through_metrics():  # update() zeroes a fresh counts tensor: one more small launch
            metrics.update(labels, pred)
            metrics.iou()

        names = ("seg_confusion_mean_iou", "seg_confusion", "SegMetrics_update_iou")
        times = windows(torch, [both, confusion, through_metrics], repeats, iters)
        res.update({"rows": ROWS, "classes": NCLASS})
        for k, t in zip(names, times):
            res[k] = summary(t)
    print(json.dumps(res))


if __name__ == "__main__":
    main(__file__, SHAPES, one, iters=20)
