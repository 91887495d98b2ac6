"""Plain torch restatements of what the attention networks compute (attention_points/
attention_scannet: attention_layer.py:10-210, pooling_attention_layer.py), for the tests of
csrc/attn_net.hip and of the layers above it. Every function takes tensors of one dtype and
works in it, so the same code gives the float64 reference and the float32 one that sets the
tolerance (tests/support.py). Not a test module.

Variables come in a dict `w`: name -> tensor, the layer's store under its hierarchical names
(INTEGRATION.md lists them).
"""
import math

import torch


def attn_reduce(Q, K, V, kd):
    """AttentionLayer.call's reduction (:35-42) for key_dim = output_dim = kd: Q (..., C),
    K, V (..., ns, C), C = H * kd. tf.reshape of (ns, C) to (H, ns, kd) is a reinterpretation of
    the group's ns * C values: head h is the contiguous run [h*ns*kd, (h+1)*ns*kd)."""
    lead, (ns, C) = K.shape[:-2], K.shape[-2:]
    H = C // kd
    Kh, Vh = K.reshape(*lead, H, ns, kd), V.reshape(*lead, H, ns, kd)
    q = Q.reshape(*lead, H, 1, kd)
    s = (Kh * q).sum(-1) / math.sqrt(kd)
    a = torch.softmax(s, dim=-1)
    return (a[..., None] * Vh).sum(-2).reshape(*lead, C)


def head_mix(qkv, H, kd):
    """InnerAttentionLayer.call between its Dense layers (:66-76): qkv (..., 3*H*kd) = [Q | K | V]
    of ONE point, attention among that point's H heads."""
    lead = qkv.shape[:-1]
    q, k, v = qkv.reshape(*lead, 3, H, kd).unbind(-3)
    a = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(kd), dim=-1)
    return (a @ v).reshape(*lead, H * kd)


def dense(w, scope, x):
    return x @ w[f"{scope}/kernel"] + w[f"{scope}/bias"]


def feed_forward(w, scope, x):
    """FeedForwardLayer (:81-105): Dense + ReLU three times, then a Dense (dropout rate 0)."""
    for i in (1, 2, 3):
        x = torch.relu(dense(w, f"{scope}/layer_{i}", x))
    return dense(w, f"{scope}/layer_4", x)


def inner_attention(w, scope, x, kd, H=5):
    """InnerAttentionLayer (:48-78): Dense q, k, v of width H*kd, head mixing, Dense out."""
    qkv = torch.cat([dense(w, f"{scope}/{n}", x) for n in ("query", "key", "value")], -1)
    return dense(w, f"{scope}/out", head_mix(qkv, H, kd))


def inner_block(w, scope, x, kd):
    """InnerAttentionBlock (:108-125)."""
    p = feed_forward(w, f"{scope}/pre_feed_forward", x)
    p = inner_attention(w, f"{scope}/inner_attention", p, kd)
    return feed_forward(w, f"{scope}/feed_forward", p) + p


def attention(w, scope, x, query, kd):
    """AttentionLayer (:10-45) with output_dim = key_dim = kd: x (B,M,ns,cin), query (B,M,cq)."""
    return attn_reduce(dense(w, f"{scope}/query", query), dense(w, f"{scope}/key", x),
                       dense(w, f"{scope}/value", x), kd)


def group(xyz, points, new_xyz, idx):
    """sample_and_group's new_points for use_xyz=True (pointnet_util.py:38-50) at the given
    centres and indices: [grouped_xyz - new_xyz, grouped points], (B,M,ns,3+C)."""
    B = xyz.shape[0]
    b = torch.arange(B)[:, None, None]
    g = xyz[b, idx.long()] - new_xyz[:, :, None]
    return g if points is None else torch.cat([g, points[b, idx.long()]], -1)


def attention_net_layer(w, scope, grouped, out_dim, nblocks):
    """AttentionNetLayer.call after sample_and_group (:158-167): grouped (B,M,ns,3+C)."""
    x = grouped
    for i in range(nblocks):
        x = inner_block(w, f"{scope}/block_{i}", x, out_dim)
    return attention(w, f"{scope}/attention", x, x[:, :, 0], out_dim)


def attention_net_mlp_layer(w, scope, grouped, out_dim, nblocks):
    """AttentionNetMLPLayer.call after sample_and_group (:200-209): ReLU between the feed-forward
    blocks, none after the last."""
    x = grouped
    for i in range(nblocks):
        x = feed_forward(w, f"{scope}/feed_forward_{i}", x)
        if i + 1 < nblocks:
            x = torch.relu(x)
    return attention(w, f"{scope}/attention", x, x[:, :, 0], out_dim)


def conv_bn_relu(w, scope, x, training, eps=1e-3):
    """tf_util.conv2d 1x1 with batch norm and ReLU: on the batch statistics (biased variance) when
    training, else on the moving ones."""
    y = x @ w[f"{scope}/weights"].reshape(x.shape[-1], -1) + w[f"{scope}/biases"]
    if training:
        dims = tuple(range(y.dim() - 1))
        mean, var = y.mean(dims), y.var(dims, unbiased=False)
    else:
        mean, var = w[f"{scope}/bn/moving_mean"], w[f"{scope}/bn/moving_variance"]
    return torch.relu((y - mean) * (w[f"{scope}/bn/gamma"] / torch.sqrt(var + eps)) +
                      w[f"{scope}/bn/beta"])


def pooling_attention_net_layer(w, scope, grouped, new_xyz, out_dim, nmlp, training):
    """PoolingAttentionNetLayer.call after sample_and_group (pooling_attention_layer.py:33-41):
    the conv2d MLP with batch norm, then attention with the Dense of new_xyz as the query."""
    x = grouped
    for i in range(nmlp):
        x = conv_bn_relu(w, f"{scope}/conv{i}", x, training)
    return attention(w, f"{scope}/attention", x, new_xyz, out_dim)
