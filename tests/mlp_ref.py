"""Shared by the GPU tests of the fused inference MLP kernels (csrc/mlp.hip): random layers, their
packing for the kernels and the numpy float32 evaluation that is the yardstick of
support.tolerance (the float64 one is oracle.mlp_f64). Not a test module."""
import numpy as np


def make_layers(rng, cin, widths, bn=True, relu=True, last_relu=None, last_bn=None):
    layers, c = [], cin
    for i, w in enumerate(widths):
        last = i == len(widths) - 1
        use_bn = bn if not (last and last_bn is not None) else last_bn
        use_relu = relu if not (last and last_relu is not None) else last_relu
        lim = np.sqrt(6.0 / (c + w))
        L = {"weights": rng.uniform(-lim, lim, (c, w)).astype(np.float32),
             "biases": rng.uniform(-0.1, 0.1, w).astype(np.float32), "relu": use_relu}
        if use_bn:
            L.update(gamma=rng.uniform(0.5, 1.5, w).astype(np.float32),
                     beta=rng.uniform(-0.2, 0.2, w).astype(np.float32),
                     moving_mean=rng.uniform(-0.1, 0.1, w).astype(np.float32),
                     moving_variance=rng.uniform(0.5, 2.0, w).astype(np.float32))
        layers.append(L)
        c = w
    return layers


def fused(pkg, layers):
    tu = pkg.tf_util
    return tu.SharedMLP([tu.PackedLayer(L["weights"], L["biases"], L.get("gamma"), L.get("beta"),
                                        L.get("moving_mean"), L.get("moving_variance"),
                                        relu=L["relu"]) for L in layers])


def mlp_f32(x, layers):
    """The same layers in numpy float32 (the error yardstick of the tolerance)."""
    y = np.asarray(x, np.float32)
    for L in layers:
        y = y @ L["weights"] + L["biases"]
        if L.get("gamma") is not None:
            s = (L["gamma"].astype(np.float64) / np.sqrt(L["moving_variance"].astype(np.float64)
                                                         + 1e-3))
            t = L["beta"] - L["moving_mean"] * s
            y = (y * s.astype(np.float32) + t.astype(np.float32)).astype(np.float32)
        if L["relu"]:
            y = np.maximum(y, 0)
    return y
