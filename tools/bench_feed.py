#!/usr/bin/env python3
"""Time the training feed on the HIP kernels of csrc/feed.hip and pn2_val_select against what
they replace:

    feed_batch   torch.ops.pn2.feed_batch at B = 16, N = 8192 with colours and normals (one
                 launch) against the torch composition of the same expressions on the same device
                 (train.py:94-108: cast, divide, concatenate, gather, not_equal, cast, multiply)
    val_chunks   data_transformation.scene_val_chunks on golden cases 1 and 2 (20,000 and 45,000
                 points, npoints = 8192, scene already on the device) against the same work
                 in numpy on the host (box tests, np.random.choice, gathers, per column)

    python tools/bench_feed.py [--repeats 15] [--iters 20] [--out summary.json]

Per figure: 3 warm-up windows, then `repeats` windows of `iters` calls, the two sides alternating,
a host clock around work that ends in a device synchronise; the median window and the range are
reported per call. No pass/fail threshold. The outputs of the two sides are compared before the
timed windows (feed_batch: xyz and smpw equal bits, the colours within one ulp, see below).
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, N = 16, 8192


def windows(sync, fns, repeats, iters):
    """Per fn the time per call (us) of `repeats` windows of `iters` calls, alternating."""
    times = [[] for _ in fns]
    for w in range(3 + repeats):
        for k, fn in enumerate(fns):
            sync()
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            sync()
            if w >= 3:
                times[k].append((time.perf_counter() - t0) / iters * 1e6)
    return times


def stats(ts):
    return {"median_us": round(statistics.median(ts), 2), "min_us": round(min(ts), 2),
            "max_us": round(max(ts), 2)}


def numpy_val_chunks(np, bounds, points, labels, colors, normals, npoints):
    """The chunker's work in numpy on the host, column by column: float64 box tests over the
    whole scene, np.random.choice, fancy-index gathers, the 1 % keep test, one concatenate per
    output. `bounds`: data_transformation._val_bounds (the columns both routes share)."""
    p64 = points.astype(np.float64)
    weights = np.ones(21)
    weights[0] = 0
    kept = []
    for box in bounds:
        lo, hi = box[:3], box[3:]
        idx = np.flatnonzero(np.all((p64 >= lo - 0.2) & (p64 <= hi + 0.2), axis=1))
        if idx.size == 0:
            continue
        draw = idx[np.random.choice(idx.size, npoints, replace=True)]
        inside = np.all((p64[draw] >= lo - 0.001) & (p64[draw] <= hi + 0.001), axis=1)
        if inside.mean() < 0.01:
            continue
        kept.append((points[draw], labels[draw], colors[draw], normals[draw],
                     weights[labels[draw]] * inside))
    return tuple(np.stack(col) for col in zip(*kept))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    pkg = importlib.import_module("pointcloud-segmentation-attention_amd")
    import pn2hip
    ops = pn2hip.ops
    assert torch.cuda.is_available(), "bench_feed needs the MI355X"
    dev = torch.device("cuda:0")
    sync = lambda: torch.cuda.synchronize(dev)  # noqa: E731
    out = {}

    g = torch.Generator().manual_seed(7)
    pts = torch.randn(B, N, 3, generator=g).to(dev)
    lab = torch.randint(0, 21, (B, N), generator=g, dtype=torch.int32).to(dev)
    col = torch.randint(0, 256, (B, N, 3), generator=g, dtype=torch.int32).to(dev)
    nrm = torch.randn(B, N, 3, generator=g).to(dev)
    sw = (torch.rand(B, N, generator=g) < 0.8).to(torch.float32).to(dev)
    cw = torch.tensor(pkg.CLASS_WEIGHTS, dtype=torch.float32, device=dev)
    lab64 = lab.to(torch.int64)

    def hip():
        return ops.feed_batch(pts, lab, col, nrm, sw, None, cw, True, True)

    def composed():
        colors = col.to(torch.float32) / 255.0
        features = torch.cat([colors, nrm], 2)
        mask = (sw != 0.0).to(torch.float32)
        return pts, features, cw[lab64] * mask
    (hx, hf, hw), (tx, tf, tw) = hip(), composed()
    assert torch.equal(hx, tx) and torch.equal(hw, tw)
    # torch divides by a scalar as a multiplication by its reciprocal: one ulp from the kernel's
    # correctly rounded quotient (which the tests pin to numpy's division)
    assert torch.allclose(hf, tf, rtol=2.0 ** -22, atol=0)
    th, tt = windows(sync, (hip, composed), a.repeats, a.iters)
    out["feed_batch"] = {"rows": B * N, "hip": stats(th), "torch_composition": stats(tt)}

    for case, sid, n in (("golden1", 1, 20000), ("golden2", 2, 45000)):
        scene = pkg.synth.scannet_scene(sid, n)
        dscene = [torch.from_numpy(x).to(dev) for x in scene]
        gen = torch.Generator(dev).manual_seed(1)

        def device_route():
            return pkg.scene_val_chunks(*dscene, 8192, generator=gen)

        bounds = pkg.data_transformation._val_bounds(torch.from_numpy(scene[0]))

        def host_route():
            return numpy_val_chunks(np, bounds, *scene, 8192)
        assert device_route()[0].shape == host_route()[0].shape
        td, tn = windows(sync, (device_route, host_route), a.repeats, max(1, a.iters // 4))
        out[f"val_chunks_{case}"] = {"points": n, "chunks": int(device_route()[0].shape[0]),
                                     "device": stats(td), "numpy_host": stats(tn)}
    print(json.dumps(out, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
