"""attention_points/models/pointnet2_sem_seg_attention.py: the SSG semantic-segmentation model
with attention instead of max pooling in all four set-abstraction modules
(attention_layer.pointnet_sa_module_attention, :28-43), on the gfx950 kernels.

Layer table, scopes, feature propagation and head are pointnet2_sem_seg's (the reference's
files differ in the SA module only): built from pointnet2_sem_seg.model_body. The attention
modules add '<scope>/ScannetAttentionLayer/dense{,_1,_2}/{kernel,bias}' and the batch norm
'<scope>/<scope>' to each SA scope.
"""
from functools import partial

from .attention_layer import pointnet_sa_module_attention
from .pointnet2_sem_seg import SA_LAYERS, get_loss, model_body  # noqa: F401

SA_MODULES = (pointnet_sa_module_attention,) * len(SA_LAYERS)
body = partial(model_body, sa_modules=SA_MODULES)  # model_body's signature, for train_step(model=)


def get_model(point_cloud, is_training, num_class, bn_decay=None, params=None):
    """point_cloud (B, N, 3) -> (logits (B, N, num_class), end_points with 'l0_xyz' and
    'feats'). Extra keyword `params`: the ParamStore (default: tf_util.default_store())."""
    return body(point_cloud, None, is_training, num_class, bn_decay, params)
