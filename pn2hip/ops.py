"""torch.ops.pn2.* under the reference's op names and argument order.

Each name is the registered PyTorch operator itself (csrc/torch_ops.cpp: one body under the CUDA
and Meta keys, so a fake tensor meets the device call's checks; autograd for gather_point / group_point / three_interpolate / attn_reduce and the training
layers mlp_layer_train, mlp_layer_train_pool, attn_kv_train, bn_train), so calls are
visible to torch.compile and TorchScript:

    farthest_point_sample(npoint, inp)                tf_sampling.py:49-57
    gather_point(inp, idx)                            tf_sampling.py:30-38
    prob_sample(inp, inpr)                            tf_sampling.py:14-23
    query_ball_point(radius, nsample, xyz1, xyz2)     tf_grouping.py:8-20  -> (idx, pts_cnt)
    group_point(points, idx)                          tf_grouping.py:33-41
    select_top_k(k, dist)                             tf_grouping.py:22-31 -> (idx, dist_out)
    knn_point(k, xyz1, xyz2)                          tf_grouping.py:48-73 -> (val, idx)
    three_nn(xyz1, xyz2)                              tf_interpolate.py:8-17 -> (dist, idx)
    three_interpolate(points, idx, weight)            tf_interpolate.py:19-28
    attn_reduce(Q, K, V)                              attention_layer.py:29-45 (reduction core)
and the fused / gradient ops of the C ABI (farthest_point_sample_and_gather, group_concat,
idw_weights, fp_fused, group_pool, *_grad), and the training-mode shared-MLP layer:

    mlp_layer_train(x, weight, bias, gamma, beta, eps, relu)   tf_util.py:165-185, is_training
                                                               -> (out, y, mean, var)
    mlp_layer_train_grad(grad_out, x, weight, y, mean, var, gamma, beta, eps, relu, need_grad_x)
                                       -> (grad_x, grad_w, grad_b, grad_gamma, grad_beta)
    mlp_layer_train_pool(x, weight, bias, gamma, beta, eps, relu)   the same layer on x
                         (..., ns, cin) fused with the max over ns (pointnet_util.py:130-136)
                                                               -> (out, y, mean, var, arg)
    mlp_layer_train_pool_grad(grad_out, arg, x, weight, y, mean, var, gamma, beta, eps, relu,
                              need_grad_x)
                                       -> (grad_x, grad_w, grad_b, grad_gamma, grad_beta)

The same four ops with the layer's three GEMMs on the bf16 matrix cores (an opt-in; the contract
is at pn2_mlp_pack_bf16 in include/pn2hip.h: operands rounded to bf16, fp32 sums, everything
after y and everything in the backward but the two GEMMs unchanged), listed in TRAIN_BF16_NAMES:

    mlp_layer_train_bf16, mlp_layer_train_bf16_grad, mlp_layer_train_pool_bf16,
    mlp_layer_train_pool_bf16_grad                     arguments and results as above

and the training-mode AttentionLayer of the attention SA modules (csrc/attn_train.hip):

    attn_kv_train(x, wq, bq, wk, bk, wv, bv, add_max)   attention_layer.py:10-45, :256-259: x
                         (..., ns, C); q = x[..., 0, :] wq + bq; kv = x [wk | wv] + [bk | bv]
                         (..., ns, 2C), one GEMM; att = the reduction (..., C); add_max: pmax, arg
                         = the max over ns of x and the lowest sample that attains it (:303), else
                         0-element tensors               -> (att, pmax, arg, q, kv)
    attn_kv_train_grad(grad_att, grad_pmax, arg, x, wq, wk, wv, q, kv, need_grad_x)
               -> (grad_x, grad_wq, grad_bq, grad_wk, grad_bk, grad_wv, grad_bv)
    bn_train(x, gamma, beta, eps, relu)                 batch-statistics batch norm of x (..., C)
                         (tf_util.py:512-531; :261)      -> (out, mean, var)
    bn_train_grad(grad_out, x, mean, var, gamma, beta, eps, relu)
                                                         -> (grad_x, grad_gamma, grad_beta)

and the reductions of the reference's attention networks (attention_scannet's AttentionNetLayer,
AttentionNetMLPLayer, PoolingAttentionNetLayer; csrc/attn_net.hip), listed in ATTN_NET_NAMES,
with autograd for attn_reduce_kd (Q, K, V) and head_mix (qkv):

    attn_reduce_kd(Q, K, V, key_dim)                    attention_layer.py:29-45 for any key_dim
                         % 4 == 0 up to 512, C = heads * key_dim; key_dim 4 is attn_reduce
    attn_reduce_kd_grad(Q, K, V, grad_out, key_dim)     -> (grad_Q, grad_K, grad_V)
    head_mix(qkv, heads, key_dim)                       InnerAttentionLayer.call (:61-78): qkv
                         (..., 3 * heads * key_dim) = [Q | K | V] per point, softmax((Q_i . K_j) /
                         sqrt(key_dim)) over the point's own heads -> (..., heads * key_dim)
    head_mix_grad(qkv, grad_out, heads, key_dim)        -> grad_qkv

and one packed inference layer at any input width, for the layers whose row the fused MLP kernel
refuses (1,280 channels and up; csrc/mlp_wide.hip), listed in WIDE_NAMES:

    dense_wide(x, packed, cin, cout, relu)              x (..., cin) through one fp32 layer packed
                         by pn2_mlp_pack (tf_util.PackedLayer.buf) -> (..., cout); the training
                         ops above take such widths themselves

and the training-mode segmentation head (csrc/head_train.hip):

    dropout(x, keep_prob, seed)                         tf_util.py:594-612 with is_training: the
                         mask is Philox4x32-10 of (seed, element), nothing is saved; autograd
                         applies the same op to the gradient
    softmax_xent(logits, labels, weights)               tf.losses.sparse_softmax_cross_entropy
                         with SUM_BY_NONZERO_WEIGHTS (pointnet2_sem_seg.py:62-69); pred = argmax
                                                         -> (loss, lse, pred, num_present)
    softmax_xent_grad(grad_loss, logits, labels, weights, lse, num_present) -> grad_logits

and the training-mode geometry of the SA and FP modules (csrc/geom_train.hip): the fused forward
kernels, with gradients that are gathers in a fixed order (no float atomics: two runs give equal
bits); autograd is registered for `points`, `points1` and `points2`, never for coordinates:

    group_concat_train(xyz, points, new_xyz, idx, use_xyz, xyz_last)   group_concat's new_points
    group_concat_train_grad(grad_new_points, idx, N, C, col0)          -> grad_points (B, N, C)
                         from columns [col0, col0 + C) of the gradient, read in place
    fp_apply_train(dist, idx, points1, points2)         IDW weights of three_nn's dist, the
                         interpolation of points2 and the concat [interp, points1]
    fp_apply_train_grad(grad_out, dist, idx, m, C2, C1) -> (grad_points2 (B, m, C2),
                         grad_points1 (B, n, C1)); bit-equal to the reference's CPU
                         ThreeInterpolateGrad loop

and what the training loop runs once the gradients exist (csrc/optim.hip; attention_points/
train.py:145-163, :337), none of it differentiable:

    adam_step(params, grads, exp_avg, exp_avg_sq, alpha, beta1, beta2, epsilon)   TF 1.x ApplyAdam
                         over the four tensor lists, in place, alpha = lr * sqrt(1 - beta2^t) /
                         (1 - beta1^t): ceil(len / 64) launches
    seg_confusion(labels, pred, confusion, counts)      adds the rows with 0 < label < C to the
                         int64 (C, C) confusion matrix and to counts = (correct, assigned)
    mean_iou(confusion)                                 tf.metrics.mean_iou's value
                                                         -> (iou, per_class)

and whole-scene prediction and the label look-ups of the benchmark score (csrc/predict.hip;
attention_points/benchmark/generate_predictions.py:19-53, :139-186, evaluate.py:58-83). These
four are listed in HOST_NAMES, not NAMES: next to the CUDA and Meta keys they have CPU kernels
(host twins with equal bits), because everything in them is integers and copied bytes:

    scene_vote(logits, mask, orig, row0, keys)          argmax per chunk row and a 64-bit atomic
                         max of ((row0 + r + 1) << 8) | label into keys[orig[r]] for the masked
                         rows: numpy's last-write-wins in any launch order   -> pred_rows
    scene_labels(keys, lut, dflt)                       -> (labels, mapped, winner)
    map_back_rows(values, row0, keys, out)              out[p] = values[winner(p) - row0]
    label_lut(inp, lut, dflt)                           0 <= inp < len(lut) ? lut[inp] : dflt

and the training feed (csrc/feed.hip, pn2_val_select in csrc/scene.hip; attention_points/
train.py:74-109, scannet_dataset/data_transformation.py:270-352), listed in FEED_NAMES: CUDA,
Meta and CPU kernels too (host twins with equal bits, csrc/cpu_feed.cpp):

    feed_batch(points, labels, colors, normals, sample_weight, cs, class_weights, use_color,
               use_normal)                              get_data_tensors + random_rotate of a
                         batch in one launch   -> (xyz, features, smpw)
    val_select(points, bounds, margin, inner_margin)    the validation chunker's columns
                                                         -> (counts, sel, inner)
    val_chunks(points, labels, colors, normals, counts, sel, inner, choice, u, npoints,
               label_weights, min_inside)               draws, keep test, compaction, gathers
                         -> (points, labels, colors, normals, weights, column, kept)

and scene rendering (csrc/render.hip; pointnet2_tensorflow/utils/render_balls_so.cpp and
show3d_balls.py:52-74), listed in RENDER_NAMES: CUDA, Meta and CPU kernels (host twins with
equal bits, csrc/cpu_render.cpp), no autograd:

    render_ball(ixyz, c0, c1, c2, labels, palette, r, h, w, background)   the reference's
                         render_ball for (F,n,3) int32 frames: a 64-bit atomic max of
                         ((z2 + 2^31) << 32) | (0xFFFFFFFF - i) per (point, disk entry), then a
                         resolve pass; three (n) colour channels, or labels and a palette
                         -> (F,h,w,3) uint8
    render_project(xyz, mats)                           the viewer's xyz.dot(rotmat) + offset and
                         astype('int32') for (F,12) float64 frames   -> (F,n,3) int32
"""
import importlib

_ops = importlib.import_module("pointcloud-segmentation-attention_amd._torch_ops").ops()

NAMES = ("farthest_point_sample", "farthest_point_sample_and_gather", "gather_point",
         "gather_point_grad", "prob_sample", "query_ball_point", "select_top_k", "knn_point",
         "group_point", "group_point_grad", "group_concat", "three_nn", "three_interpolate",
         "three_interpolate_grad", "idw_weights", "fp_fused", "attn_reduce", "attn_reduce_grad",
         "group_pool", "mlp_layer_train", "mlp_layer_train_grad", "mlp_layer_train_pool",
         "mlp_layer_train_pool_grad", "attn_kv_train", "attn_kv_train_grad", "bn_train",
         "bn_train_grad", "dropout", "softmax_xent", "softmax_xent_grad", "group_concat_train",
         "group_concat_train_grad", "fp_apply_train", "fp_apply_train_grad", "adam_step",
         "seg_confusion", "mean_iou")
# the ops that also run on CPU tensors (every op in NAMES is device-only, three_nn and the two
# three_interpolate ops excepted)
HOST_NAMES = ("scene_vote", "scene_labels", "map_back_rows", "label_lut")
FEED_NAMES = ("feed_batch", "val_select", "val_chunks")
# the training layer's opt-in bf16 matrix-core mode (device-only, like NAMES)
TRAIN_BF16_NAMES = ("mlp_layer_train_bf16", "mlp_layer_train_bf16_grad",
                    "mlp_layer_train_pool_bf16", "mlp_layer_train_pool_bf16_grad")
# the attention networks' reductions (csrc/attn_net.hip; device-only, like NAMES)
ATTN_NET_NAMES = ("attn_reduce_kd", "attn_reduce_kd_grad", "head_mix", "head_mix_grad")
# the K-streamed layer over rows at any input width (csrc/mlp_wide.hip; device-only, inference)
WIDE_NAMES = ("dense_wide",)
# scene rendering (csrc/render.hip; CUDA, Meta and CPU kernels, like FEED_NAMES)
RENDER_NAMES = ("render_ball", "render_project")
_ALL = (NAMES + HOST_NAMES + FEED_NAMES + TRAIN_BF16_NAMES + ATTN_NET_NAMES + WIDE_NAMES +
        RENDER_NAMES)
for _n in _ALL:
    globals()[_n] = getattr(_ops, _n)

__all__ = list(_ALL)
