#!/usr/bin/env python3
"""Benchmark of the K-streamed layer kernel (csrc/mlp_wide.hip) on the layers of the attention
networks that the fused MLP kernel refuses, at B = 16, each beside what ran them before: the torch
composition attention_layer._layer_torch (a matmul and a hand-written batch norm) on the same
tensors in the same process, the two alternating window by window (tools/_timing.py).

Layers, rows x cin -> cout: inference (tf_util.WideLayer over pn2_dense_wide against
_layer_torch with the moving statistics) and training forward + backward (tf_util.mlp_train, whose
forward and input gradient run on the kernel, against _layer_torch on the batch statistics, both
through autograd for x and every variable). dense_512_8192 is the pooling layers' key / value
Dense: its forward fits the fused kernel, its input gradient (8,192 -> 512 over W^T) does not.

Models: the whole PoolingAttentionNetModel and AttentionNetModel, forward (inference) and training
step (forward + backward of every variable), on a store with wide_layers="hip" against one with
wide_layers="torch", which runs what the parent commit ran.

One child process per shape; --out writes profiles/dense_wide/summary.json."""
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _timing  # noqa: E402

PKG = "pointcloud-segmentation-attention_amd"
# name: (rows, cin, cout, batch norm + ReLU)
LAYERS = {
    "pool_l3_conv0": (32768, 2051, 128, True),
    "pool_l4_conv0": (8192, 4099, 256, True),
    "pool_fa_layer1": (1024, 12288, 256, True),
    "pool_fa_layer2": (4096, 2304, 256, True),
    "net_fa_layer1": (1024, 1536, 256, True),
    "dense_512_8192": (8192, 512, 8192, False),
}
MODELS = {"PoolingAttentionNetModel": "pooling_attention_model",
          "AttentionNetModel": "attention_models"}
BATCH, NPOINT, NUM_CLASS = 16, 8192, 21


def _entry(hip, torch_):
    h, t = _timing.summary(hip), _timing.summary(torch_)
    return {"hip": h, "torch": t, "torch_over_hip": round(t["us"] / h["us"], 2),
            # slower than torch by more than torch's own run-to-run spread
            "hip_slower_beyond_spread": h["us"] - t["us"] > t["min_max_us"][1] - t["min_max_us"][0]}


def one_layer(name, repeats, iters):
    import torch
    pkg = importlib.import_module(PKG)
    tu, A = pkg.tf_util, pkg.attention_layer
    dev = torch.device("cuda:0")
    rows, cin, cout, bn = LAYERS[name]
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.rand(rows, cin, device=dev, generator=g) * 2 - 1
    go = torch.rand(rows, cout, device=dev, generator=g) * 2 - 1
    res = {"shape": name, "rows": rows, "cin": cin, "cout": cout,
           "plan": dict(zip(("row_tiles", "k_slab", "out_tiles_per_wg"), _plan(pkg, rows, cin, cout)))}

    def layer_of(store):
        if bn:
            return tu.torch_layers(store, ["l"], cin, [cout], bn=True)[0]
        return tu.TorchLayer(store.dense("l", cin, cout), relu=False)

    if A.plan_accepts(cin, (cout,)):
        res["inference"] = "the fused kernel takes this layer"
    else:
        store = tu.ParamStore(seed=3)
        L = layer_of(store)
        wide = A._packed_wide(store, L, "l")
        Ld = A._device_layer(store, L, "l")
        with torch.no_grad():
            hip, tor = _timing.windows(torch, [lambda: wide(x),
                                               lambda: A._layer_torch(x, Ld, False, None)],
                                       repeats, iters)
        res["inference"] = _entry(hip, tor)
    tstore = tu.ParamStore(seed=3).trainable(dev)
    Lt = layer_of(tstore)
    leaf = x.clone().requires_grad_(True)
    params = [leaf] + [v for v in Lt.params.values() if v is not None and v.requires_grad]

    def step(fwd):
        def run():
            torch.autograd.grad(fwd(), params, go)
        return run

    hip, tor = _timing.windows(
        torch, [step(lambda: tu.mlp_train(leaf, [Lt], None, precision="fp32")),
                step(lambda: A._layer_torch(leaf, Lt, True, None))], repeats, iters)
    res["training_forward_backward"] = _entry(hip, tor)
    print(json.dumps(res), flush=True)


def _plan(pkg, rows, cin, cout):
    import ctypes
    L = importlib.import_module(PKG + "._lib")
    tab = (L.MlpLayer * 1)(L.MlpLayer(1 << 20, cin, cout, 0))
    out = [ctypes.c_int(0) for _ in range(3)]
    L.check(L.lib().pn2_dense_wide_plan(rows, cin, tab, *(ctypes.addressof(o) for o in out)),
            "dense_wide_plan")
    return [o.value for o in out]


def one_model(name, repeats, iters):
    import torch
    pkg = importlib.import_module(PKG)
    tu = pkg.tf_util
    dev = torch.device("cuda:0")
    xyz = torch.from_numpy(pkg.synth.batch(range(BATCH), NPOINT, "scannet")[0]).to(dev)
    mod = getattr(pkg, MODELS[name])
    res = {"shape": name, "batch": BATCH, "points": NPOINT}

    def model_of(mode, training):
        store = tu.ParamStore(seed=2, wide_layers=mode)
        if training:
            store = store.trainable(dev)
        model = getattr(mod, name)(training, None, NUM_CLASS, params=store, seed=9)
        with torch.no_grad():   # creates every variable
            model.body(xyz, None, False, NUM_CLASS, None, store)
        return model, store

    fns = []
    for mode in ("hip", "torch"):
        model, store = model_of(mode, False)
        fns.append(lambda model=model: model(xyz))
    with torch.no_grad():
        hip, tor = _timing.windows(torch, fns, repeats, iters)
    res["forward"] = _entry(hip, tor)
    del fns
    torch.cuda.empty_cache()
    steps = []
    for mode in ("hip", "torch"):
        model, store = model_of(mode, True)
        params = list(store.parameters())

        def step(model=model, store=store, params=params):
            out = model.body(xyz, None, True, NUM_CLASS, None, store)
            logits = out[0] if isinstance(out, (tuple, list)) else out
            torch.autograd.grad(logits.square().mean(), params, allow_unused=True)
        steps.append(step)
    hip, tor = _timing.windows(torch, steps, repeats, iters)
    res["training_step"] = _entry(hip, tor)
    print(json.dumps(res), flush=True)


def one(name, repeats, iters):
    assert importlib.import_module("torch").cuda.is_available(), \
        "bench_dense_wide.py measures on the MI355X only"
    (one_layer if name in LAYERS else one_model)(name, repeats, iters)


if __name__ == "__main__":
    _timing.main(__file__, tuple(LAYERS) + tuple(MODELS), one, iters=5, timeout=300,
                 header={"batch": BATCH, "what": "us per call, median of the windows; torch = "
                         "attention_layer._layer_torch (layers) or wide_layers='torch' (models), "
                         "what the parent commit ran"})
