"""pointnet2_tensorflow/models/pointnet2_sem_seg.py: the SSG semantic-segmentation model and
its loss under the reference's names, on the gfx950 kernels.

get_model has the reference's layers and scopes (pointnet2_sem_seg.py:19-59): four
set-abstraction modules, four feature-propagation modules, fc1 (conv1d + batch norm), dropout
dp1 and fc2. With is_training False it is the fused inference path of the module calls; with
is_training True on a trainable store (tf_util.ParamStore.trainable()) every layer runs the HIP
training kernels. get_loss is tf.losses.sparse_softmax_cross_entropy with the per-point weights
(:62-69).
"""
from . import tf_util
from .pointnet_util import pointnet_fp_module, pointnet_sa_module


# (scope, npoint, radius, nsample, mlp) of the set-abstraction modules and (scope, mlp) of the
# feature-propagation modules, in call order (pointnet2_sem_seg.py:29-50)
SA_LAYERS = (("layer1", 1024, 0.1, 32, [32, 32, 64]),
             ("layer2", 256, 0.2, 32, [64, 64, 128]),
             ("layer3", 64, 0.4, 32, [128, 128, 256]),
             ("layer4", 16, 0.8, 32, [256, 256, 512]))
FP_LAYERS = (("fa_layer1", [256, 256]), ("fa_layer2", [256, 256]), ("fa_layer3", [256, 128]),
             ("fa_layer4", [128, 128, 128]))


def model_body(point_cloud, l0_points, is_training, num_class, bn_decay=None, params=None,
               seed=None, sa_modules=None):
    """The layers of get_model, shared with pointnet2_sem_seg_features.get_model: l0_points is
    None here and the per-point features (B, N, C) there (attention_points/models/
    pointnet2_sem_seg_features.py:25). `seed`: the dropout seed (tf_util.dropout), None to draw
    one from torch's CPU generator. `sa_modules`: the set-abstraction module of each of the four
    layers, callables with pointnet_sa_module's signature (the attention models pass
    attention_layer.pointnet_sa_module_attention / _and_pooling); None: pointnet_sa_module
    everywhere."""
    store = params if params is not None else tf_util.default_store()
    end_points = {"l0_xyz": point_cloud}
    xyz, points = [point_cloud], [l0_points]
    if sa_modules is None:
        sa_modules = (pointnet_sa_module,) * len(SA_LAYERS)
    if len(sa_modules) != len(SA_LAYERS):
        raise ValueError(f"model_body expects {len(SA_LAYERS)} sa_modules, got {len(sa_modules)}")
    for sa_module, (scope, npoint, radius, nsample, mlp) in zip(sa_modules, SA_LAYERS):
        new_xyz, new_points, _ = sa_module(
            xyz[-1], points[-1], npoint, radius, nsample, mlp, None, False, is_training, bn_decay,
            scope, params=store)
        xyz.append(new_xyz)
        points.append(new_points)
    # level k receives level k + 1's features, from the coarsest level down to the input cloud
    for (scope, mlp), k in zip(FP_LAYERS, (3, 2, 1, 0)):
        points[k] = pointnet_fp_module(xyz[k], xyz[k + 1], points[k], points[k + 1], mlp,
                                       is_training, bn_decay, scope, params=store)
    net = tf_util.conv1d(points[0], 128, 1, "fc1", padding="VALID", bn=True,
                         is_training=is_training, bn_decay=bn_decay, params=store)
    end_points["feats"] = net
    net = tf_util.dropout(net, is_training, "dp1", keep_prob=0.5, seed=seed)
    # the reference calls fc2 without is_training; here the flag selects the training layer, and
    # without it fc2's variables would never learn on a trainable store
    # fc2 stays fp32 on a bf16 store, in inference and in training (precision="fp32" holds for
    # both): 21 logits, negligible work, and it decides the argmax
    net = tf_util.conv1d(net, num_class, 1, "fc2", padding="VALID", activation_fn=None,
                         is_training=is_training, params=store, precision="fp32")
    return net, end_points


def get_model(point_cloud, is_training, num_class, bn_decay=None, params=None):
    """Semantic-segmentation PointNet++: point_cloud (B, N, 3) -> (logits (B, N, num_class),
    end_points with 'l0_xyz' and 'feats', the fc1 output). Extra keyword `params`: the
    ParamStore (default: tf_util.default_store())."""
    return model_body(point_cloud, None, is_training, num_class, bn_decay, params)


def get_loss(pred, label, smpw):
    """pred: BxNxC logits, label: BxN, smpw: BxN per-point weights (0 for unannotated points).
    The weighted sum of the cross-entropies over the number of non-zero weights."""
    return tf_util.sparse_softmax_cross_entropy(labels=label, logits=pred, weights=smpw)
