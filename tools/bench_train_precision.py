#!/usr/bin/env python3
"""Time train.train_step of pointnet2_sem_seg at both train precisions of the store
(tf_util.ParamStore(train_precision=...): the fp32 HIP training layers, and their opt-in bf16
matrix-core mode), at B = 16 clouds of 8,192 points:

    python tools/bench_train_precision.py [--repeats 7] [--iters 5] [--out summary.json]

One child process under `timeout`; in it the two stores (equal seeds, so equal initial values)
each take five warm-up steps, then alternate in `repeats` windows of `iters` steps on one fixed
batch with a fixed dropout seed, timed with events on the stream. A step is zero_grad, the model
with is_training=True, the weighted loss, backward, Adam and the metrics update. Reported: the
median window per step with its spread, clouds per second, and the two losses after the timed
steps (not a statement about accuracy: one synthetic batch, random labels)."""
import importlib
import json
import os
import sys

from _timing import main, summary, windows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = {"sem_seg_B16": (16, 8192)}
NCLASS = 21


def one(name, repeats, iters):
    import numpy as np
    import torch
    pkg = importlib.import_module("pointcloud-segmentation-attention_amd")
    assert torch.cuda.is_available(), "bench_train_precision needs the MI355X"
    dev = torch.device("cuda:0")
    B, N = SHAPES[name]
    xyz = torch.from_numpy(pkg.synth.batch(range(B), N, "scannet")[0]).to(dev)
    rng = np.random.default_rng(B * N)
    labels_np = rng.integers(0, NCLASS, (B, N)).astype(np.int32)
    smpw_np = (rng.uniform(0.5, 5.0, (B, N)) * (labels_np > 0)).astype(np.float32)
    labels, smpw = torch.from_numpy(labels_np).to(dev), torch.from_numpy(smpw_np).to(dev)
    last = {}

    def stepper(prec):
        store = pkg.tf_util.ParamStore(seed=1, train_precision=prec).trainable(dev)
        opt, metrics = pkg.train.AdamOptimizer(store), pkg.train.SegMetrics(NCLASS, dev)

        def step():
            last[prec] = pkg.train.train_step(store, opt, metrics, xyz, labels, smpw, NCLASS,
                                              bn_decay=0.5, seed=1)[0]
        return step

    steps = [stepper("fp32"), stepper("bf16")]
    for fn in steps:
        for _ in range(5):
            fn()
    t32, t16 = windows(torch, steps, repeats, iters)
    s32, s16 = summary(t32), summary(t16)
    print(json.dumps({
        "shape": name, "model": "pointnet2_sem_seg", "batch": B, "points": N, "repeats": repeats,
        "iters": iters, "fp32_step": s32, "bf16_step": s16,
        "fp32_clouds_per_s": round(B / s32["us"] * 1e6, 1),
        "bf16_clouds_per_s": round(B / s16["us"] * 1e6, 1),
        "fp32_over_bf16": round(s32["us"] / s16["us"], 3),
        "loss_after": {k: round(float(v), 4) for k, v in last.items()}}))


if __name__ == "__main__":
    main(__file__, SHAPES, one, iters=5, timeout=240)
