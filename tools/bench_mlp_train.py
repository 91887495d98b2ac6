#!/usr/bin/env python3
"""Time one training-mode shared-MLP layer, forward plus backward, on the HIP kernels
(torch.ops.pn2.mlp_layer_train, csrc/mlp_train.hip) against the torch composition it replaces
(tf_util.mlp_torch with is_training=True plus autograd), at three layer shapes of cfg2:

    SA1 conv1   524,288 rows   32 -> 32
    FP4 conv0   131,072 rows  128 -> 128
    SA4 conv1     8,192 rows  256 -> 512

    python tools/bench_mlp_train.py [--repeats 7] [--iters 10] [--out summary.json]
                                    [--precision bf16]

Each shape runs in a child process of its own under `timeout`; a shape that fails stops the
run. Per shape: warm-up, then `repeats` timed windows of `iters` forward+backward passes per
side, the two sides alternating, timed with events on the stream; the median window is
reported. Both sides compute gradients for the input, weight, bias, gamma and beta. The torch
side keeps its moving averages on the CPU (as tf_util.mlp_torch does: one device-to-host copy
per layer) and gets its weights as device tensors.

`max_rel_grad_diff` is the largest difference between the two sides' gradients over the
largest gradient: last-bit differences of reordered fp32 sums, except that a pre-activation
within rounding of zero can fall on either side of the ReLU (a discrete difference of up to
one grad_out element), and that the bias gradient under batch norm is exactly 0 on the HIP
side and rounding noise on the torch side (shown as 1.0).

Then, per C entry point of the layer, the time of the call alone (events, median of `repeats`
windows) and the bytes its algorithm has to move (computed from the shape) over that time,
against the measured copy peak of 6.03 TB/s. The two GEMMs through pn2_shared_mlp
include their pn2_mlp_pack.

--precision bf16 adds the layer's opt-in bf16 matrix-core mode (torch.ops.pn2.mlp_layer_train_bf16)
as a third side in the same alternating windows of the same child process, and
pn2_mlp_wgrad_bf16 and the two bf16 GEMMs (pn2_mlp_pack_bf16 included) to the entry-point table.
`bf16_checks` holds what the issue of that mode asks of the times: the bf16 layer's median window
below the fp32 layer's fastest one (FP4 conv0, SA4 conv1: matrix-core bound in fp32), not above
its slowest one (SA1 conv1: load bound), and pn2_mlp_wgrad_bf16 no slower than pn2_mlp_wgrad.
"""
import importlib
import json
import os
import statistics
import sys

from _timing import main, windows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_PEAK_TBS = 6.03
SHAPES = {"SA1_conv1": (524288, 32, 32), "FP4_conv0": (131072, 128, 128),
          "SA4_conv1": (8192, 256, 512)}
EPS = 1e-3


def one(name, repeats, iters, precision="fp32"):
    import torch
    pkg = importlib.import_module("pointcloud-segmentation-attention_amd")
    import pn2hip
    L, tu, ops = importlib.import_module(pkg.__name__ + "._lib"), pkg.tf_util, pn2hip.ops
    assert torch.cuda.is_available(), "bench_mlp_train needs the MI355X"
    dev = torch.device("cuda:0")
    rows, cin, cout = SHAPES[name]
    g = torch.Generator().manual_seed(rows + cin)
    lim = (6.0 / (cin + cout)) ** 0.5
    leaf = lambda t: t.to(dev).requires_grad_(True)  # noqa: E731
    x = leaf(torch.rand(rows, cin, generator=g) * 2 - 1)
    w = leaf((torch.rand(cin, cout, generator=g) * 2 - 1) * lim)
    b = leaf(torch.rand(cout, generator=g) * 0.2 - 0.1)
    gamma = leaf(torch.rand(cout, generator=g) + 0.5)
    beta = leaf(torch.rand(cout, generator=g) * 0.4 - 0.2)
    go = (torch.rand(rows, cout, generator=g) * 2 - 1).to(dev)
    leaves = (x, w, b, gamma, beta)
    layer = tu.TorchLayer({"weights": w, "biases": b, "gamma": gamma, "beta": beta,
                           "moving_mean": torch.zeros(cout), "moving_variance": torch.ones(cout)})

    def clear():
        for t in leaves:
            t.grad = None

    def hip():
        clear()
        ops.mlp_layer_train(x, w, b, gamma, beta, EPS, True)[0].backward(go)

    def parent():
        clear()
        tu.mlp_torch(x, [layer], True, None).backward(go)

    def hip_bf16():
        clear()
        ops.mlp_layer_train_bf16(x, w, b, gamma, beta, EPS, True)[0].backward(go)

    bf16 = precision == "bf16"

    # same gradients on both sides (reordered fp32 sums differ in the last bits)
    hip()
    gh = [t.grad.clone() for t in leaves]
    parent()
    diffs = {}
    for nm, a, t in zip(("x", "w", "b", "gamma", "beta"), gh, leaves):
        scale = max(float(t.grad.abs().max()), 1e-6)
        diffs[nm] = float((a - t.grad).abs().max()) / scale
    bf16_diffs = {}
    if bf16:  # against the fp32 HIP layer: the rounding of the operands, about 2^-8 relative
        hip_bf16()
        for nm, a, t in zip(("x", "w", "b", "gamma", "beta"), gh, leaves):
            scale = max(float(a.abs().max()), 1e-6)
            bf16_diffs[nm] = float((a - t.grad).abs().max()) / scale
    times = windows(torch, [hip, parent] + ([hip_bf16] if bf16 else []), repeats, iters)
    t_hip, t_par = (statistics.median(t) for t in times[:2])
    spread = [(min(t), max(t)) for t in times]

    # the C entry points alone
    xd, wd, bd, gd, btd = (t.detach() for t in leaves)
    lib, ptr, st = L.lib(), L.ptr, L.stream_of(xd)
    f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)  # noqa: E731
    y, out, gy, gx, gw = f32(rows, cout), f32(rows, cout), f32(rows, cout), f32(rows, cin), f32(cin, cout)
    mean, var, gg, gb = f32(cout), f32(cout), f32(cout), f32(cout)
    ws_bn = int(lib.pn2_bn_workspace_size(rows, cout))
    ws_wg = int(lib.pn2_mlp_wgrad_workspace_size(rows, cin, cout))
    wsb, wsw = f32(max(ws_bn // 4, 4)), f32(max(ws_wg // 4, 4))
    wt = wd.t().contiguous()

    def gemm(inp, weight, bias, ci, co, dst, bf=False):
        size, pack = ((lib.pn2_mlp_packed_size_bf16, lib.pn2_mlp_pack_bf16) if bf else
                      (lib.pn2_mlp_packed_size, lib.pn2_mlp_pack))
        nb = int(size(ci, co))
        packed = f32((nb + 3) // 4)
        L.check(pack(ptr(weight), ptr(bias), None, None, ci, co, ptr(packed), nb, st), "mlp_pack")
        tab = (L.MlpLayer * 1)(L.MlpLayer(packed.data_ptr(), ci, co, L.PN2_MLP_BF16 if bf else 0))
        L.check(lib.pn2_shared_mlp(ptr(inp), rows, ci, 1, tab, ptr(dst), st), "shared_mlp")

    R, F = rows * 4, 4
    calls = {
        "pn2_shared_mlp y=xW+b": (lambda: gemm(xd, wd, bd, cin, cout, y), R * (cin + cout)),
        "pn2_bn_stats": (lambda: L.check(lib.pn2_bn_stats(
            ptr(y), rows, cout, ptr(mean), ptr(var), ptr(wsb), ws_bn, st), "bn_stats"), R * cout),
        "pn2_bn_act_fwd": (lambda: L.check(lib.pn2_bn_act_fwd(
            ptr(y), rows, cout, ptr(mean), ptr(var), ptr(gd), ptr(btd), EPS, 1, ptr(out), st),
            "bn_act_fwd"), 2 * R * cout),
        "pn2_bn_act_bwd": (lambda: L.check(lib.pn2_bn_act_bwd(
            ptr(go), ptr(y), rows, cout, ptr(mean), ptr(var), ptr(gd), ptr(btd), EPS, 1, ptr(gy),
            ptr(gg), ptr(gb), ptr(wsb), ws_bn, st), "bn_act_bwd"), 5 * R * cout),
        "pn2_mlp_wgrad": (lambda: L.check(lib.pn2_mlp_wgrad(
            ptr(xd), ptr(gy), rows, cin, cout, ptr(gw), ptr(wsw), ws_wg, st), "mlp_wgrad"),
            R * (cin + cout) + ws_wg * 2 + F * cin * cout),
        "pn2_shared_mlp grad_x=grad_y W^T": (lambda: gemm(gy, wt, None, cout, cin, gx),
                                             R * (cin + cout)),
    }
    if bf16:
        calls.update({
            "pn2_shared_mlp y=xW+b bf16": (lambda: gemm(xd, wd, bd, cin, cout, y, True),
                                           R * (cin + cout)),
            "pn2_mlp_wgrad_bf16": (lambda: L.check(lib.pn2_mlp_wgrad_bf16(
                ptr(xd), ptr(gy), rows, cin, cout, ptr(gw), ptr(wsw), ws_wg, st), "mlp_wgrad_bf16"),
                R * (cin + cout) + ws_wg * 2 + F * cin * cout),
            "pn2_shared_mlp grad_x=grad_y W^T bf16": (lambda: gemm(gy, wt, None, cout, cin, gx, True),
                                                      R * (cin + cout)),
        })
    for fn, _ in calls.values():  # in order: each call's inputs exist
        fn()
    kern = {}
    # a bf16 entry point alternates with its fp32 twin in the same windows
    twins = {nm: nm[:-5] for nm in calls if nm.endswith("bf16")}  # " bf16" / "_bf16"
    timed = {}
    for nm, (fn, nbytes) in calls.items():
        if nm in twins:
            continue
        pair = [nm] + [b for b, a in twins.items() if a == nm]
        for k, t in zip(pair, windows(torch, [calls[k][0] for k in pair], repeats, iters)):
            timed[k] = t
    for nm, (fn, nbytes) in calls.items():
        t = timed[nm]
        us = statistics.median(t)
        kern[nm] = {"us": round(us, 1), "min_max_us": [round(min(t), 1), round(max(t), 1)],
                    "bytes": nbytes, "GBps": round(nbytes / us / 1e3, 1),
                    "frac_copy_peak": round(nbytes / us / 1e6 / COPY_PEAK_TBS, 3)}
    extra = {}
    if bf16:
        t_bf = statistics.median(times[2])
        extra = {"bf16_fwd_bwd_us": round(t_bf, 1),
                 "bf16_min_max_us": [round(min(times[2]), 1), round(max(times[2]), 1)],
                 "hip_over_bf16": round(t_hip / t_bf, 2),
                 "bf16_max_rel_grad_diff_vs_hip": {k: float(f"{v:.3g}")
                                                   for k, v in bf16_diffs.items()},
                 "bf16_checks": {
                     "layer_median_below_fp32_fastest": bool(t_bf < min(times[0])),
                     "layer_median_not_above_fp32_slowest": bool(t_bf <= max(times[0])),
                     "wgrad_bf16_no_slower": bool(kern["pn2_mlp_wgrad_bf16"]["us"]
                                                  <= kern["pn2_mlp_wgrad"]["us"])}}
    print(json.dumps({
        "shape": name, "rows": rows, "cin": cin, "cout": cout, "repeats": repeats, "iters": iters,
        "hip_fwd_bwd_us": round(t_hip, 1), "parent_fwd_bwd_us": round(t_par, 1),
        "hip_min_max_us": [round(v, 1) for v in spread[0]],
        "parent_min_max_us": [round(v, 1) for v in spread[1]],
        "parent_over_hip": round(t_par / t_hip, 2), "no_slower": bool(t_hip <= t_par),
        "max_rel_grad_diff": {k: float(f"{v:.3g}") for k, v in diffs.items()}, **extra,
        "entry_points": kern}))


if __name__ == "__main__":
    main(__file__, SHAPES, one, timeout=150, header={"copy_peak_TBps": COPY_PEAK_TBS},
         options=[("--precision", {"choices": ("fp32", "bf16"), "default": None,
                                   "help": "bf16: time the layer's bf16 mode as a further side"})])
