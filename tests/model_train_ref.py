"""The training-mode segmentation model (pointnet2_sem_seg / pointnet2_sem_seg_features with
is_training=True, get_loss, and the attention SA modules) restated in plain torch on the CPU,
shared by tests/test_model_train_ref_cpu.py and tests/test_gpu_model_train.py (no tests here).

The reference is a function of the dtype (float64: the truth; float32: the yardstick of the
project's tolerance) and of a *record* of the discrete choices of one forward, following
tests/test_gpu_mlp_train_scale.py::test_module_gradients_vs_f64: the choices are validated bit
for bit elsewhere, and a flip between two equally good candidates is not an error.

  taken from the record      the sampled centres (coordinates), the ball-query / kNN indices,
                             the three_nn indices and fp32 squared distances, every ReLU mask
                             (out > 0), every max pool's argmax, the dropout seed
  restated here, in dtype    grouping and centring, conv + bias, batch norm on batch statistics
                             (every axis but the channel, biased variance, eps 1e-3), the ReLU
                             as a product with the mask, the max pool as a gather at the argmax
                             followed by the mask of the pooled output, the attention layer
                             (heads of 4 channels, logits / 2, softmax over nsample, its batch
                             norm, + the max for _and_pooling), the IDW weights from the recorded
                             distances, interpolation and concat [interpolated, points1], dropout
                             (head_train_ref.dropout_keep, scaled by 1 / keep_prob) and the loss
                             (head_train_ref.xent_ref)

A record is a dict:
    centres    [new_xyz (B, M, 3) float32]              per SA level
    group_idx  [idx (B, M, ns) int64]                   per SA level
    nn         [(dist (B, n, 3) float32, idx int64)]    per FP level, in call order
    layers     [{"mask": out > 0, "arg": int64 or None}] per conv layer, in call order
    attn_arg   [arg (B, M, C) int64]                    per attention SA level
    seed, keep_prob                                     of the dropout
`decisions(entries)` builds it from the (name, args, outputs) triples a spy around
_torch_ops.call collected.

A model is described by a spec (ssg_spec, attention_spec, or one a test writes):
    cin         channels of the input features (0: none)
    sa          [{"scope", "npoint", "radius", "nsample", "mlp", "kind"}], kind "max" (the SSG
                module), "attn" or "attn_pool" (the attention modules)
    fp          [{"scope", "mlp"}]: FP module j writes level len(sa) - 1 - j
    fc1, num_class, keep_prob
"""
import numpy as np
import torch

from head_train_ref import dropout_keep, xent_ref

EPS = 1e-3  # tf.contrib.layers.batch_norm's epsilon

# pointnet2_sem_seg.py:29-50
SSG_SA = (("layer1", 1024, 0.1, 32, (32, 32, 64)), ("layer2", 256, 0.2, 32, (64, 64, 128)),
          ("layer3", 64, 0.4, 32, (128, 128, 256)), ("layer4", 16, 0.8, 32, (256, 256, 512)))
SSG_FP = (("fa_layer1", (256, 256)), ("fa_layer2", (256, 256)), ("fa_layer3", (256, 128)),
          ("fa_layer4", (128, 128, 128)))


def make_spec(cin, sa, fp, fc1, num_class, keep_prob=0.5):
    return {"cin": cin, "fc1": fc1, "num_class": num_class, "keep_prob": keep_prob,
            "sa": [dict(scope=s, npoint=m, radius=r, nsample=ns, mlp=list(w), kind=kind)
                   for s, m, r, ns, w, kind in sa],
            "fp": [dict(scope=s, mlp=list(w)) for s, w in fp]}


def ssg_spec(num_class, cin):
    """pointnet2_sem_seg (cin 0) / pointnet2_sem_seg_features (cin feature channels)."""
    return make_spec(cin, [l + ("max",) for l in SSG_SA], SSG_FP, 128, num_class)


def attention_spec(num_class, cin):
    """The attention stack of tests/test_gpu_model_train.py case (c)."""
    return make_spec(cin, [("layer1", 256, 0.2, 16, (32, 32, 64), "attn"),
                           ("layer2", 64, 0.4, 16, (64, 64, 128), "attn_pool")],
                     [("fa_layer1", (128, 128)), ("fa_layer2", (128, 128))], 128, num_class)


def variables(spec):
    """[(TF variable name, TF shape, initialiser, trainable)] in creation order."""
    out = []

    def conv(scope, cin, cout, bn=True):
        out.append((f"{scope}/weights", (1, 1, cin, cout), "xavier", True))
        out.append((f"{scope}/biases", (cout,), "zeros", True))
        if bn:
            batch_norm(f"{scope}/bn", cout)

    def batch_norm(scope, c):
        out.extend([(f"{scope}/gamma", (c,), "ones", True), (f"{scope}/beta", (c,), "zeros", True),
                    (f"{scope}/moving_mean", (c,), "zeros", False),
                    (f"{scope}/moving_variance", (c,), "ones", False)])

    c = [spec["cin"]]
    for L in spec["sa"]:
        ci = c[-1] + 3
        for i, w in enumerate(L["mlp"]):
            conv(f"{L['scope']}/conv{i}", ci, w)
            ci = w
        if L["kind"] != "max":
            for d in ("dense", "dense_1", "dense_2"):
                base = f"{L['scope']}/ScannetAttentionLayer/{d}"
                out.append((f"{base}/kernel", (ci, ci), "xavier", True))
                out.append((f"{base}/bias", (ci,), "zeros", True))
            batch_norm(f"{L['scope']}/{L['scope']}", ci)
        c.append(ci)
    K = len(spec["sa"])
    for j, L in enumerate(spec["fp"]):
        k = K - 1 - j
        ci = c[k] + c[k + 1]
        for i, w in enumerate(L["mlp"]):
            conv(f"{L['scope']}/conv_{i}", ci, w)
            ci = w
        c[k] = ci
    conv("fc1", c[0], spec["fc1"])
    conv("fc2", spec["fc1"], spec["num_class"], bn=False)
    return out


def attention_names(scope):
    """(wq, bq, wk, bk, wv, bv) of the attention layer under `scope`."""
    base = f"{scope}/ScannetAttentionLayer"
    return [f"{base}/{d}/{v}" for d in ("dense", "dense_1", "dense_2") for v in ("kernel", "bias")]


def leaf_names(spec):
    return [n for n, _, _, tr in variables(spec) if tr]


def bn_scopes(spec):
    """The prefixes '<...>' of every '<...>/moving_mean'."""
    return [n[:-len("/moving_mean")] for n, _, _, _ in variables(spec)
            if n.endswith("/moving_mean")]


def bias_under_bn(spec):
    """The conv biases a batch norm follows: the batch mean absorbs them, their gradient is 0."""
    scopes = set(bn_scopes(spec))
    return [n for n in leaf_names(spec)
            if n.endswith("/biases") and n[:-len("/biases")] + "/bn" in scopes]


def absorbed(spec):
    """leaf with a mathematically zero gradient -> a leaf of the same layer to measure rounding
    noise against. These are the conv biases under batch norm and the beta of an attention
    module's batch norm: no ReLU follows that one, and a constant per channel passes through the
    next grouping, through an interpolation (its weights sum to 1) and through an FP concat into
    a conv whose batch norm subtracts it again."""
    out = {n: n[:-len("biases")] + "weights" for n in bias_under_bn(spec)}
    for L in spec["sa"]:
        if L["kind"] != "max":
            out[f"{L['scope']}/{L['scope']}/beta"] = f"{L['scope']}/{L['scope']}/gamma"
    return out


def random_init(spec, seed):
    """Every variable with values away from the initialisers' special ones (gamma 1, beta 0,
    bias 0), as float32 CPU tensors."""
    g = torch.Generator().manual_seed(seed)
    def u(lo, hi, s):
        return (torch.rand(s, generator=g, dtype=torch.float64) * (hi - lo) + lo).float()
    init = {}
    for name, shape, kind, _ in variables(spec):
        if kind == "xavier":
            lim = float(np.sqrt(6.0 / (shape[-2] + shape[-1])))
            init[name] = u(-lim, lim, shape)
        elif name.endswith(("gamma", "moving_variance")):
            init[name] = u(0.5, 1.5, shape)
        else:
            init[name] = u(-0.3, 0.3, shape)
    return init


def decisions(entries):
    """The record of one forward from a spy's (name, args, outputs) triples, in call order."""
    cpu = lambda t: t.detach().cpu()  # noqa: E731
    rec = {"centres": [], "group_idx": [], "nn": [], "layers": [], "attn_arg": [], "seed": None,
           "keep_prob": None, "dropout_out": None}
    for name, args, out in entries:
        if name == "farthest_point_sample_and_gather":
            rec["centres"].append(cpu(out[1]))
        elif name == "query_ball_point":
            rec["group_idx"].append(cpu(out[0]).long())
        elif name == "knn_point":
            rec["group_idx"].append(cpu(out[1]).long())
        elif name == "three_nn":
            rec["nn"].append((cpu(out[0]), cpu(out[1]).long()))
        elif name in ("mlp_layer_train", "mlp_layer_train_pool"):
            o = cpu(out[0])
            arg = cpu(out[4]).long().reshape(o.shape) if name.endswith("_pool") else None
            rec["layers"].append({"mask": o > 0, "arg": arg})
        elif name == "attn_kv_train":
            rec["attn_arg"].append(cpu(out[2]).long().reshape(out[1].shape))
        elif name == "dropout":
            rec["keep_prob"], rec["seed"] = float(args[1]), int(args[2])
            rec["dropout_out"] = cpu(out)
    return rec


def _gather_ns(z, arg):
    """z (B, M, ns, C) at arg (B, M, C) along ns; an arg outside [0, ns) selects nothing."""
    ok = (arg >= 0) & (arg < z.shape[2])
    picked = torch.gather(z, 2, arg.clamp(0, z.shape[2] - 1).unsqueeze(2)).squeeze(2)
    return picked * ok.to(z.dtype)


def attention_core(X, wq, bq, wk, bk, wv, bv):
    """attention_layer.py:24-42 on the per-point features X (B, M, ns, C): the Dense query of
    each group's first row, Dense keys and values, heads of 4 channels cut from the reference's
    reshape of the (ns, C) matrices, logits / 2, softmax over nsample -> (B, M, C)."""
    Bm, M, ns, C = X.shape
    H = C // 4
    Q = (X[:, :, 0] @ wq + bq).reshape(Bm, M, H, 1, 4)
    Kh = (X @ wk + bk).reshape(Bm, M, H, ns, 4)
    Vh = (X @ wv + bv).reshape(Bm, M, H, ns, 4)
    w = torch.softmax((Q @ Kh.transpose(-1, -2)) / 2, dim=-1)
    return (w @ Vh).reshape(Bm, M, C)


def attention_op_grads(x, weights, grad_att, grad_pmax, arg, dt):
    """The attention op on its own, for localising an error: x (B, M, ns, C) and `weights` =
    (wq, bq, wk, bk, wv, bv) as float32 values, the incoming gradients grad_att (B, M, C) and
    grad_pmax (B, M, C) or None with the max pool's arg. Returns the gradients of x and of the
    six variables in dtype dt, in the order of attn_kv_train_grad's outputs."""
    X = x.detach().cpu().to(dt).requires_grad_(True)
    wq, bq, wk, bk, wv, bv = (w.detach().cpu().to(dt).requires_grad_(True) for w in weights)
    out = (attention_core(X, wq, bq, wk, bk, wv, bv) * grad_att.detach().cpu().to(dt)).sum()
    if grad_pmax is not None:
        a = arg.detach().cpu().long().reshape(grad_pmax.shape)
        out = out + (_gather_ns(X, a) * grad_pmax.detach().cpu().to(dt)).sum()
    out.backward()
    return [t.grad for t in (X, wq, bq, wk, bk, wv, bv)]


def forward(spec, P, xyz, feats, rec, dt):
    """The model up to the logits in dtype dt: P name -> leaf (dt), xyz (B, N, 3) float32, feats
    (B, N, cin) in dt or None. Returns {"logits", "feats", "stats": bn scope -> (mean, var),
    "inter": [(label, activation)] in the order the layers run}."""
    B, K = xyz.shape[0], len(spec["sa"])
    b = torch.arange(B).reshape(B, 1, 1)
    stats, inter = {}, []
    layers, attn_args = iter(rec["layers"]), iter(rec["attn_arg"])

    def bn(y, scope):
        y2 = y.reshape(-1, y.shape[-1])
        mean = y2.mean(0)
        var = ((y2 - mean) ** 2).mean(0)  # biased
        stats[scope] = (mean.detach(), var.detach())
        return (y - mean) * (P[f"{scope}/gamma"] / torch.sqrt(var + EPS)) + P[f"{scope}/beta"]

    def conv(a, scope, batch_norm=True, relu=True, pool=False):
        L = next(layers)
        w = P[f"{scope}/weights"]
        z = a @ w.reshape(w.shape[-2], w.shape[-1]) + P[f"{scope}/biases"]
        if batch_norm:
            z = bn(z, f"{scope}/bn")
        if pool:
            z = _gather_ns(z, L["arg"])
        if relu:
            assert L["mask"].shape == z.shape, (scope, L["mask"].shape, z.shape)
            z = z * L["mask"].to(dt)
        inter.append((scope, z))
        return z

    def attention(X, L):
        sc = L["scope"]
        out = bn(attention_core(X, *(P[n] for n in attention_names(sc))), f"{sc}/{sc}")
        arg = next(attn_args)
        if L["kind"] == "attn_pool":
            out = out + _gather_ns(X, arg)
        inter.append((f"{sc}/attention", out))
        return out

    lv = [xyz.to(dt)] + [c.to(dt) for c in rec["centres"]]
    pts = [feats]
    for i, L in enumerate(spec["sa"]):
        idx = rec["group_idx"][i]
        g = lv[i][b, idx] - lv[i + 1].unsqueeze(2)
        if pts[i] is not None:
            g = torch.cat([g, pts[i][b, idx]], dim=-1)
        last = len(L["mlp"]) - 1
        for j in range(last + 1):
            g = conv(g, f"{L['scope']}/conv{j}", pool=L["kind"] == "max" and j == last)
        pts.append(g if L["kind"] == "max" else attention(g, L))
    for j, L in enumerate(spec["fp"]):
        k = K - 1 - j
        dist, nidx = rec["nn"][j]
        r = 1 / torch.clamp(dist.to(dt), min=1e-10)
        w = r / r.sum(dim=2, keepdim=True)
        a = (pts[k + 1][b, nidx] * w.unsqueeze(-1)).sum(dim=2)
        if pts[k] is not None:
            a = torch.cat([a, pts[k]], dim=-1)
        for i in range(len(L["mlp"])):
            a = conv(a, f"{L['scope']}/conv_{i}")
        pts[k] = a
    net = conv(pts[0], "fc1")
    keep = dropout_keep(net.numel(), rec["keep_prob"], rec["seed"]).reshape(tuple(net.shape))
    dropped = net * torch.from_numpy(keep).to(dt) / rec["keep_prob"]
    inter.append(("dp1", dropped))
    logits = conv(dropped, "fc2", batch_norm=False, relu=False)
    return {"logits": logits, "feats": net, "stats": stats, "inter": inter, "keep": keep}


def leaves_of(spec, init, dt):
    return {n: init[n].detach().cpu().to(dt).clone().requires_grad_(True)
            for n in leaf_names(spec)}


def run(spec, init, xyz, feats, labels, smpw, rec, dt):
    """Forward, loss and backward in dtype dt. Returns {"logits", "feats", "loss", "stats",
    "grads": name -> gradient of every leaf, "grad_feats" (None without input features),
    "inter", "keep"}, all detached."""
    P = leaves_of(spec, init, dt)
    f = None if feats is None else feats.detach().cpu().to(dt).clone().requires_grad_(True)
    out = forward(spec, P, xyz.detach().cpu(), f, rec, dt)
    logits = out["logits"]
    C = logits.shape[-1]
    loss, _, z = xent_ref(torch, logits.reshape(-1, C), labels.cpu().reshape(-1),
                          smpw.cpu().reshape(-1), dt)
    loss.backward()
    logits.backward(z.grad.reshape(logits.shape))
    out.update(logits=logits.detach(), feats=out["feats"].detach(), loss=loss.detach(),
               grads={n: (torch.zeros_like(p) if p.grad is None else p.grad) for n, p in P.items()},
               grad_feats=None if f is None else f.grad,
               inter=[(k, v.detach()) for k, v in out["inter"]])
    return out


def moving_after(stats, init, decay, dt):
    """bn scope -> (moving_mean, moving_variance) after one update from `init`'s values:
    decay * initial + (1 - decay) * batch statistic, in dtype dt."""
    return {s: (decay * init[f"{s}/moving_mean"].to(dt) + (1 - decay) * m.to(dt),
                decay * init[f"{s}/moving_variance"].to(dt) + (1 - decay) * v.to(dt))
            for s, (m, v) in stats.items()}


# The full-size cases of tests/test_gpu_model_train.py: name -> (spec, input features?)
B, N, DECAY, STORE_SEED, DROPOUT_SEED = 2, 2048, 0.8, 11, (5 << 32) + 20240
CASES = {"a": (ssg_spec(21, 0), False), "b": (ssg_spec(4, 6), True),
         "c": (attention_spec(5, 6), True)}


def case_inputs(pkg, name):
    """(spec, xyz (B, N, 3) float32, feats (B, N, 6) float32 or None, labels, smpw) on the CPU.
    2048 points and not the other model tests' 1024: SA1's sampler then picks a real subset and
    FP4 interpolates between distinct points instead of copying at distance 0."""
    spec, with_feats = CASES[name]
    xyz, feats = pkg.synth.batch([0, 1], N, "scannet", with_features=True)
    labels, smpw = targets(B, N, spec["num_class"], seed=ord(name))
    return (spec, torch.from_numpy(xyz), torch.from_numpy(feats) if with_feats else None, labels,
            smpw)


def store_init(pkg, spec, seed=STORE_SEED):
    """The values a fresh ParamStore(seed=seed) gives the spec's variables (the reference's
    initialisers), as float32 CPU tensors in their TF shapes."""
    store = pkg.tf_util.ParamStore(seed=seed)
    return {n: store.get(n, shape, kind).clone() for n, shape, kind, _ in variables(spec)}


def targets(B, N, num_class, seed):
    """labels (B, N) int32 in [0, num_class) with about a fifth equal to 0; smpw (B, N) float32:
    0 where the label is 0 and on a further 10 % of the rows, in [0.5, 5) elsewhere."""
    g = np.random.default_rng(seed)
    labels = g.integers(1, num_class, (B, N)).astype(np.int32)
    labels[g.random((B, N)) < 0.2] = 0
    smpw = g.uniform(0.5, 5.0, (B, N)).astype(np.float32)
    smpw[(labels == 0) | (g.random((B, N)) < 0.1)] = 0
    return torch.from_numpy(labels), torch.from_numpy(smpw)
