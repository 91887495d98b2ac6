"""attention_points/attention_scannet/pooling_attention_layer.py: a set-abstraction layer whose
pooling over the group is the AttentionLayer with the Dense of the group's centre as the query.
"""
from . import pointnet_util, tf_util
from .attention_layer import _store, group_attention, run_layers


class PoolingAttentionNetLayer:
    """pooling_attention_layer.py:6-46. [xyz, points] -> (new_xyz, new_points (B, npoint,
    16*out_dim), idx): sample_and_group (knn=False, use_xyz=True), the conv2d MLP `mlp` with batch
    norm, then AttentionLayer(out_dim, key_dim=out_dim) over the group with the Dense of new_xyz
    (B, npoint, 3) as the query (:41). The reference's tf.squeeze of axis 2 (:45) has nothing to
    squeeze in the (B, npoint, C) result and is not copied.

    Variables: '<scope>/conv<i>/...' (tf_util.conv2d's, :34-38) and '<scope>/attention/
    {query,key,value}/{kernel,bias}'. Extra keywords `scope` and `params` (the ParamStore);
    calling the layer takes is_training (None: the constructor's)."""

    def __init__(self, bn_decay, mlp, npoint, out_dim, is_training=True, radius=0.1, nsample=32,
                 bn=True, scope="PoolingAttentionNetLayer", params=None):
        if out_dim % 4 or not 4 <= out_dim <= 512:
            raise NotImplementedError("PoolingAttentionNetLayer runs out_dim % 4 == 0, 4 <= out_dim "
                                      f"<= 512 (key_dim = out_dim), got {out_dim}")
        self.bn_decay, self.mlp, self.npoint = bn_decay, list(mlp), npoint
        self.out_dim, self.key_dim = out_dim, out_dim
        self.is_training, self.radius, self.nsample, self.bn = is_training, radius, nsample, bn
        self.scope, self.params = scope, params

    def __call__(self, inputs, is_training=None, bn_decay=None):
        xyz, points = inputs
        training = self.is_training if is_training is None else is_training
        decay = self.bn_decay if bn_decay is None else bn_decay
        store = _store(self.params)
        if pointnet_util._is_empty_points(points):
            points = None
        new_xyz, x, idx, _ = pointnet_util.sample_and_group(self.npoint, self.radius, self.nsample,
                                                           xyz, points, False, True)
        scopes = [f"{self.scope}/conv{i}" for i in range(len(self.mlp))]
        if scopes:
            layers = tf_util.torch_layers(store, scopes, int(x.shape[-1]), self.mlp, bn=self.bn)
            x = run_layers(store, x, layers, scopes, training, decay)
        out = group_attention(store, f"{self.scope}/attention", x, new_xyz.detach(), self.key_dim,
                              16, training)
        return new_xyz, out, idx
