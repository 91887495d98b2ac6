"""torch.ops.pn2.* — the C ABI registered as PyTorch operators (csrc/torch_ops.cpp, built into
libpn2torch.so next to libpn2hip.so): TORCH_LIBRARY schemas with the reference's op names and
argument order, one body per op that launches on the current HIP stream and, registered under
Meta as well, gives fake tensors / torch.compile the same checks and output shapes. This module loads the library and registers autograd for the ops the
reference registers gradients for, w.r.t. the points only (tf_sampling.py:44-48 GatherPoint,
tf_grouping.py:42-46 GroupPoint, tf_interpolate.py:29-34 ThreeInterpolate), plus the attention
reduction (TF autodiff through attention_layer.py:35-42, all of Q, K, V; attn_reduce_kd for any
key_dim, and head_mix, the attention among one point's heads of :61-78: csrc/attn_net.hip) and the training-mode
shared-MLP layer (mlp_layer_train, and mlp_layer_train_pool for the layer fused with the max
pool over nsample: x, weight, bias, gamma, beta; csrc/mlp_train.hip; their _bf16 namesakes, the
layer's opt-in bf16 matrix-core mode, use the _bf16 grad ops), the training-mode attention
layer (attn_kv_train: x and the three Dense layers' variables; csrc/attn_train.hip) and the
stand-alone batch-statistics batch norm (bn_train: x, gamma, beta). The training head's ops
(csrc/head_train.hip: dropout, the same op on the gradient with the same seed; softmax_xent,
the logits only) and the training-mode geometry ops (csrc/geom_train.hip: group_concat_train,
the points only; fp_apply_train, points1 and points2) carry their autograd in libpn2torch.so
itself (csrc/torch_ops.cpp). The optimiser and metrics ops (csrc/optim.hip: adam_step,
seg_confusion, mean_iou) mutate their arguments in place and are not differentiable. The
prediction ops (csrc/predict.hip: scene_vote, scene_labels, map_back_rows, label_lut) are
integers and copied bytes; they also have CPU kernels (the host twins, equal bits), and so have
the training feed's ops (csrc/feed.hip, pn2_val_select in csrc/scene.hip: feed_batch, val_select,
val_chunks; host twins in csrc/cpu_feed.cpp), whose arithmetic is fixed operation by operation,
and the rendering ops (csrc/render.hip: render_ball, render_project; host twins in
csrc/cpu_render.cpp), which carry no autograd.

The mirror modules (tf_sampling, tf_grouping, tf_interpolate, attention_layer) call these ops
for every reference-signature call; the pn2hip alias package re-exports them as pn2hip.ops.
"""
import os

import torch

from ._lib import _HERE, InvalidArgumentError

TORCH_LIB_PATH = os.environ.get("PN2TORCH_LIB") or os.path.join(_HERE, "libpn2torch.so")
_loaded = False


def ops():
    """torch.ops.pn2, loading libpn2torch.so on first use (raises if it was not built)."""
    global _loaded
    if not _loaded:
        if not os.path.exists(TORCH_LIB_PATH):
            raise RuntimeError(
                f"{TORCH_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ "
                "as g; g.build()'`. pn2hip has no CPU fallback.")
        torch.ops.load_library(TORCH_LIB_PATH)
        _register_autograd()
        _loaded = True
    return torch.ops.pn2


def call(name, *args):
    """torch.ops.pn2.<name>(*args) for the mirror modules: the op's reference-text ValueError
    (TORCH_CHECK_VALUE, or PN2_EINVAL from the C ABI) surfaces as InvalidArgumentError, the
    mirror's stand-in for tf.errors.InvalidArgumentError (a ValueError too)."""
    try:
        return getattr(ops(), name)(*args)
    except InvalidArgumentError:
        raise
    except ValueError as e:
        raise InvalidArgumentError(str(e).splitlines()[0]) from e


def _register_autograd():
    reg = torch.library.register_autograd

    def save_all(ctx, inputs, output):
        ctx.save_for_backward(*inputs)

    def gather_bwd(ctx, grad):
        inp, idx = ctx.saved_tensors
        return torch.ops.pn2.gather_point_grad(inp, idx, grad.contiguous()), None

    def group_bwd(ctx, grad):
        points, idx = ctx.saved_tensors
        return torch.ops.pn2.group_point_grad(points, idx, grad.contiguous()), None

    def interp_bwd(ctx, grad):
        points, idx, weight = ctx.saved_tensors
        return torch.ops.pn2.three_interpolate_grad(points, idx, weight, grad.contiguous()), \
            None, None

    def attn_bwd(ctx, grad):
        Q, K, V = ctx.saved_tensors
        return tuple(torch.ops.pn2.attn_reduce_grad(Q, K, V, grad.contiguous()))

    def attn_kd_setup(ctx, inputs, output):
        *qkv, ctx.key_dim = inputs
        ctx.save_for_backward(*qkv)

    def attn_kd_bwd(ctx, grad):
        Q, K, V = ctx.saved_tensors
        return tuple(torch.ops.pn2.attn_reduce_kd_grad(Q, K, V, grad.contiguous(),
                                                       ctx.key_dim)) + (None,)

    def head_mix_setup(ctx, inputs, output):
        qkv, ctx.heads, ctx.key_dim = inputs
        ctx.save_for_backward(qkv)

    def head_mix_bwd(ctx, grad):
        qkv, = ctx.saved_tensors
        return torch.ops.pn2.head_mix_grad(qkv, grad.contiguous(), ctx.heads,
                                           ctx.key_dim), None, None

    def mlp_setup(ctx, inputs, output, bf16=False):
        # mlp_layer_train returns (out, y, mean, var), mlp_layer_train_pool the pool's arg too
        x, weight, bias, gamma, beta, eps, relu = inputs
        out, y, mean, var, *arg = output
        ctx.mark_non_differentiable(y, mean, var, *arg)
        ctx.save_for_backward(x, weight, y, mean, var, gamma, beta, *arg)
        ctx.eps, ctx.relu, ctx.has_bias, ctx.bf16 = eps, relu, bias is not None, bf16

    def mlp_setup_bf16(ctx, inputs, output):
        mlp_setup(ctx, inputs, output, bf16=True)

    def mlp_bwd(ctx, grad_out, *_):
        x, weight, y, mean, var, gamma, beta, *arg = ctx.saved_tensors
        # pooled, grad_out is (..., cout): the (..., ns, cout) gradient of the activation never
        # exists. The input gradient is one more GEMM: skipped when nothing upstream needs it
        # (SA1's first layer reads coordinates). A _bf16 forward gets the _bf16 grad op: its two
        # GEMMs run on the bf16 matrix cores too (the rounding is straight-through)
        pn2 = torch.ops.pn2
        if ctx.bf16:
            grad = pn2.mlp_layer_train_pool_bf16_grad if arg else pn2.mlp_layer_train_bf16_grad
        else:
            grad = pn2.mlp_layer_train_pool_grad if arg else pn2.mlp_layer_train_grad
        gx, gw, gb, gg, gbeta = grad(grad_out.contiguous(), *arg, x, weight, y, mean, var, gamma,
                                     beta, ctx.eps, ctx.relu, ctx.needs_input_grad[0])
        bn = gamma is not None
        return (gx if ctx.needs_input_grad[0] else None, gw, gb if ctx.has_bias else None,
                gg if bn else None, gbeta if bn else None, None, None)

    def attn_kv_setup(ctx, inputs, output):
        x, wq, bq, wk, bk, wv, bv, add_max = inputs
        att, pmax, arg, q, kv = output
        ctx.mark_non_differentiable(arg, q, kv)
        ctx.save_for_backward(x, wq, wk, wv, q, kv, arg)
        ctx.add_max = add_max

    def attn_kv_bwd(ctx, grad_att, grad_pmax, *_):
        # grad_x is written once by the (2C -> C) GEMM and patched at 2 G C elements: the query
        # row's and the max pool's gradients never exist as (..., ns, C) tensors
        x, wq, wk, wv, q, kv, arg = ctx.saved_tensors
        grads = torch.ops.pn2.attn_kv_train_grad(
            grad_att.contiguous(), grad_pmax.contiguous() if ctx.add_max else None, arg, x, wq,
            wk, wv, q, kv, ctx.needs_input_grad[0])
        return (grads[0] if ctx.needs_input_grad[0] else None,) + tuple(grads[1:]) + (None,)

    def bn_setup(ctx, inputs, output):
        x, gamma, beta, eps, relu = inputs
        out, mean, var = output
        ctx.mark_non_differentiable(mean, var)
        ctx.save_for_backward(x, mean, var, gamma, beta)
        ctx.eps, ctx.relu = eps, relu

    def bn_bwd(ctx, grad_out, *_):
        x, mean, var, gamma, beta = ctx.saved_tensors
        gx, gg, gbeta = torch.ops.pn2.bn_train_grad(grad_out.contiguous(), x, mean, var, gamma,
                                                    beta, ctx.eps, ctx.relu)
        return gx, gg, gbeta, None, None

    reg("pn2::attn_kv_train", attn_kv_bwd, setup_context=attn_kv_setup)
    reg("pn2::bn_train", bn_bwd, setup_context=bn_setup)
    reg("pn2::mlp_layer_train", mlp_bwd, setup_context=mlp_setup)
    reg("pn2::mlp_layer_train_pool", mlp_bwd, setup_context=mlp_setup)
    reg("pn2::mlp_layer_train_bf16", mlp_bwd, setup_context=mlp_setup_bf16)
    reg("pn2::mlp_layer_train_pool_bf16", mlp_bwd, setup_context=mlp_setup_bf16)
    reg("pn2::gather_point", gather_bwd, setup_context=save_all)
    reg("pn2::group_point", group_bwd, setup_context=save_all)
    reg("pn2::three_interpolate", interp_bwd, setup_context=save_all)
    reg("pn2::attn_reduce", attn_bwd, setup_context=save_all)
    reg("pn2::attn_reduce_kd", attn_kd_bwd, setup_context=attn_kd_setup)
    reg("pn2::head_mix", head_mix_bwd, setup_context=head_mix_setup)
