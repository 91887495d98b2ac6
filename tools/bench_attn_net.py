#!/usr/bin/env python3
"""Micro-benchmark of the attention networks' reductions (csrc/attn_net.hip): torch.ops.pn2.
attn_reduce_kd and its gradient, head_mix and its gradient, each beside what a user would
otherwise run: the torch composition (reshape, matmul, scale, softmax, matmul; autograd for the
backward) on the same tensors in the same process.

Shapes: the reduction at the net layers' own shapes (B = 16, ns = 32, 16 heads; M x kd = 1024 x 8,
256 x 16, 64 x 32, 16 x 64) and at the pooling model's first layer (M = 1024, kd = 64); head_mix
at the row counts of the same net layers (B * M * ns rows, 5 heads, the same kd).

Back-to-back launches between HIP events, median of `--reps` windows. Bytes are what the
algorithm needs: forward 2 G ns C 4 read (K and V) plus Q and the output; backward the same read
plus grad_K and grad_V written (plus Q, grad_out, grad_Q); head_mix one read of qkv and one write
of the output, its backward qkv and grad_out read and grad_qkv written. Writes one JSON document
(--out, default profiles/attn_net/summary.json) and prints it."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NET_SHAPES = (("l1", 1024, 8), ("l2", 256, 16), ("l3", 64, 32), ("l4", 16, 64))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_net", "summary.json"))
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    args = ap.parse_args()
    import torch
    import pn2hip
    ops = pn2hip.ops
    assert torch.cuda.is_available(), "bench_attn_net.py measures on the MI355X only"
    dev = torch.device("cuda:0")

    def timeit(fn):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.inner):
                fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3 / args.inner)
        return statistics.median(ts)

    def entry(hip_us, torch_us, nbytes):
        return {"hip_us": round(hip_us, 1), "torch_us": round(torch_us, 1),
                "hip_GBps": round(nbytes / hip_us / 1e3), "bytes": nbytes,
                "torch_over_hip": round(torch_us / hip_us, 2)}

    def reduce_torch(Q, K, V, kd):
        B, M, ns, C = K.shape
        H = C // kd
        Kh, Vh = K.reshape(B, M, H, ns, kd), V.reshape(B, M, H, ns, kd)
        s = torch.matmul(Q.reshape(B, M, H, 1, kd), Kh.transpose(-1, -2)) / math.sqrt(kd)
        return torch.matmul(torch.softmax(s, dim=-1), Vh).reshape(B, M, C)

    def mix_torch(qkv, H, kd):
        q, k, v = qkv.reshape(-1, 3, H, kd).unbind(1)
        a = torch.softmax(torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(kd), dim=-1)
        return torch.matmul(a, v).reshape(-1, H * kd)

    def bench_reduce(B, M, ns, H, kd):
        C = H * kd
        Q = torch.rand((B, M, C), device=dev) - 0.5
        K = torch.rand((B, M, ns, C), device=dev) - 0.5
        V = torch.rand((B, M, ns, C), device=dev) - 0.5
        go = torch.rand((B, M, C), device=dev) - 0.5
        with torch.no_grad():
            fwd = timeit(lambda: ops.attn_reduce_kd(Q, K, V, kd))
            bwd = timeit(lambda: ops.attn_reduce_kd_grad(Q, K, V, go, kd))
            t_fwd = timeit(lambda: reduce_torch(Q, K, V, kd))
        L = [t.clone().requires_grad_(True) for t in (Q, K, V)]

        def torch_step():
            torch.autograd.grad(reduce_torch(*L, kd), L, go)
        t_step = timeit(torch_step)
        kv = 2 * B * M * ns * C * 4
        small = B * M * C * 4
        return {"shape": {"B": B, "M": M, "ns": ns, "H": H, "kd": kd},
                "forward": entry(fwd, t_fwd, kv + 2 * small),
                # the torch column is forward + backward (autograd needs its own forward); the
                # HIP column beside it is forward + gradient too
                "forward_backward": entry(fwd + bwd, t_step, 3 * kv + 5 * small),
                "backward_hip_us": round(bwd, 1),
                "backward_hip_GBps": round((2 * kv + 3 * small) / bwd / 1e3)}

    def bench_mix(rows, H, kd):
        W = H * kd
        qkv = torch.rand((rows, 3 * W), device=dev) * 2 - 1
        go = torch.rand((rows, W), device=dev) - 0.5
        with torch.no_grad():
            fwd = timeit(lambda: ops.head_mix(qkv, H, kd))
            bwd = timeit(lambda: ops.head_mix_grad(qkv, go, H, kd))
            t_fwd = timeit(lambda: mix_torch(qkv, H, kd))
        leaf = qkv.clone().requires_grad_(True)

        def torch_step():
            torch.autograd.grad(mix_torch(leaf, H, kd), leaf, go)
        t_step = timeit(torch_step)
        return {"shape": {"rows": rows, "H": H, "kd": kd},
                "forward": entry(fwd, t_fwd, rows * 4 * W * 4),
                "forward_backward": entry(fwd + bwd, t_step, rows * 11 * W * 4),
                "backward_hip_us": round(bwd, 1),
                "backward_hip_GBps": round(rows * 7 * W * 4 / bwd / 1e3)}

    B = args.batch
    res = {"device": torch.cuda.get_device_name(0), "batch": B, "reps": args.reps,
           "inner": args.inner, "attn_reduce_kd": {}, "head_mix": {}}
    for name, M, kd in NET_SHAPES:
        res["attn_reduce_kd"][name] = bench_reduce(B, M, 32, 16, kd)
    res["attn_reduce_kd"]["pooling_l1"] = bench_reduce(B, 1024, 32, 16, 64)
    for name, M, kd in NET_SHAPES:
        res["head_mix"][name] = bench_mix(B * M * 32, 5, kd)
    slower = [f"{op}/{name}/{what}" for op in ("attn_reduce_kd", "head_mix")
              for name, r in res[op].items() for what in ("forward", "forward_backward")
              if r[what]["torch_over_hip"] < 1.0]
    res["slower_than_torch"] = slower
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
