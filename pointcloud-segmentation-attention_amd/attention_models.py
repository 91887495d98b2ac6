"""attention_points/attention_scannet/attention_models.py: the three segmentation networks built
from AttentionNetLayer / AttentionNetMLPLayer instead of set-abstraction modules, on the gfx950
kernels: four such layers, four feature-propagation modules, fc1 (conv1d + batch norm), dropout
dp1 and fc2 (:17-253).

Each class takes the reference's constructor arguments (is_training, bn_decay, num_class) and the
keywords `params` (the ParamStore), `npoints` (the four layers' npoint; the reference's (1024,
256, 64, 16)), `radius` (the reference queries every level with 0.1) and `seed` (the dropout
seed). model(inputs) returns the logits (B, N, num_class), get_end_points(inputs) the dict with
'l0_xyz' and 'feats' (the fc1 output). model.body has pointnet2_sem_seg.model_body's signature, for
train.train_step_with(model.body, store, ...), and get_loss is pointnet2_sem_seg's.

A feature-propagation MLP whose input is wider than the fused kernel takes (fa_layer1 reads
512 + 1024 channels here) runs its first layer on the K-streamed kernel (pn2_dense_wide) with
ParamStore(wide_layers="hip"), from torch ops with the default wide_layers="torch"
(attention_layer.run_layers).
"""
from . import pointnet_util, tf_util
from .attention_layer import (AttentionNetLayer, AttentionNetMLPLayer, _store, plan_accepts,
                              run_layers)
from .pointnet2_sem_seg import FP_LAYERS, get_loss  # noqa: F401

NPOINTS = (1024, 256, 64, 16)


def fp_module(store, xyz1, xyz2, points1, points2, mlp, is_training, bn_decay, scope):
    """pointnet_util.pointnet_fp_module; where the fused kernel refuses the MLP's input width,
    the interpolation and concat kernels, then the layers one by one (run_layers: the wide first
    layer on pn2_dense_wide or from torch ops, as the store's wide_layers says)."""
    C = (0 if points1 is None else int(points1.shape[2])) + int(points2.shape[2])
    training = is_training or pointnet_util._needs_grad(points1, points2)
    if not training and plan_accepts(C, tuple(mlp)):
        return pointnet_util.pointnet_fp_module(xyz1, xyz2, points1, points2, mlp, is_training,
                                                bn_decay, scope, params=store)
    x = pointnet_util.fp_interpolate(xyz1, xyz2, points1, points2)
    scopes = [f"{scope}/conv_{i}" for i in range(len(mlp))]
    return run_layers(store, x, tf_util.torch_layers(store, scopes, C, mlp, bn=True), scopes,
                      is_training, bn_decay)


def propagate_and_classify(store, xyz, points, is_training, num_class, bn_decay, seed):
    """The four feature-propagation modules and the head shared by every network here and by
    pointnet2_sem_seg.model_body (whose scopes these are): xyz, points = the five levels' lists."""
    end_points = {"l0_xyz": xyz[0]}
    for (scope, mlp), k in zip(FP_LAYERS, (3, 2, 1, 0)):
        points[k] = fp_module(store, xyz[k], xyz[k + 1], points[k], points[k + 1], mlp,
                              is_training, bn_decay, scope)
    net = tf_util.conv1d(points[0], 128, 1, "fc1", padding="VALID", bn=True,
                         is_training=is_training, bn_decay=bn_decay, params=store)
    end_points["feats"] = net
    net = tf_util.dropout(net, is_training, "dp1", keep_prob=0.5, seed=seed)
    net = tf_util.conv1d(net, num_class, 1, "fc2", padding="VALID", activation_fn=None,
                         is_training=is_training, params=store, precision="fp32")
    return net, end_points


class _Model:
    """Four layers `self.layers` (callables [xyz, points] -> new_xyz, new_points, idx), then
    propagate_and_classify."""
    takes_features = False

    def __init__(self, is_training, bn_decay, num_class, params=None, npoints=NPOINTS, radius=0.1,
                 seed=None):
        if len(npoints) != 4:
            raise ValueError(f"npoints: one per layer, 4, got {len(npoints)}")
        self.is_training, self.bn_decay, self.num_class = is_training, bn_decay, num_class
        self.params, self.npoints, self.radius, self.seed = params, tuple(npoints), radius, seed
        self.layers = self.build_layers()
        self.l1, self.l2, self.l3, self.l4 = self.layers

    def body(self, point_cloud, features, is_training, num_class, bn_decay=None, params=None,
             seed=None):
        """pointnet2_sem_seg.model_body's signature (train.train_step_with's `model`). The layers
        were built over the constructor's store: `params` must be that store or None."""
        store = _store(self.params)
        if params is not None and params is not store:
            raise ValueError("body: `params` is not the store this model was built with")
        xyz, points = [point_cloud], [features]
        for layer in self.layers:
            new_xyz, new_points, _ = self.call_layer(layer, xyz[-1], points[-1], is_training,
                                                     bn_decay)
            xyz.append(new_xyz)
            points.append(new_points)
        return propagate_and_classify(store, xyz, points, is_training, num_class, bn_decay,
                                      self.seed if seed is None else seed)

    def call_layer(self, layer, xyz, points, is_training, bn_decay):
        return layer([xyz, points], is_training)

    def _split(self, inputs):
        if self.takes_features:
            xyz, features = inputs
            return xyz, features
        return inputs, None

    def __call__(self, inputs):
        return self.body(*self._split(inputs), self.is_training, self.num_class, self.bn_decay)[0]

    def get_end_points(self, inputs):
        return self.body(*self._split(inputs), self.is_training, self.num_class, self.bn_decay)[1]


# (out_dim, inner_dimensions) of l1..l4
NET_LAYERS = ((8, [8]), (16, [16]), (32, [32]), (64, [64]))           # :20-27, :99-106
MLP_LAYERS = ((16, [16] * 4), (32, [32] * 4), (64, [64] * 4), (64, [64] * 4))  # :178-187


class AttentionNetModel(_Model):
    """attention_models.py:17-93: inputs = the cloud (B, N, 3). Variables 'l<k>/...' of the four
    AttentionNetLayer, 'fa_layer<k>/conv_<i>/...', 'fc1/...', 'fc2/...'."""

    def build_layers(self):
        return [AttentionNetLayer(npoint=n, out_dim=d, inner_dimensions=inner, radius=self.radius,
                                  nsample=32, is_training=self.is_training, scope=f"l{k + 1}",
                                  params=self.params)
                for k, (n, (d, inner)) in enumerate(zip(self.npoints, NET_LAYERS))]


class AttentionNetFeatureModel(AttentionNetModel):
    """attention_models.py:96-172: inputs = (cloud (B, N, 3), features (B, N, C))."""
    takes_features = True


class AttentionNetMLPModel(_Model):
    """attention_models.py:175-253: AttentionNetMLPLayer in place of AttentionNetLayer."""

    def build_layers(self):
        return [AttentionNetMLPLayer(npoint=n, out_dim=d, inner_dimensions=inner,
                                     radius=self.radius, nsample=32, is_training=self.is_training,
                                     scope=f"l{k + 1}", params=self.params)
                for k, (n, (d, inner)) in enumerate(zip(self.npoints, MLP_LAYERS))]
