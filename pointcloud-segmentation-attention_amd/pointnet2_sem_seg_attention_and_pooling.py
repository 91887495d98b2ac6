"""attention_points/models/pointnet2_sem_seg_attention_and_pooling.py: the SSG
semantic-segmentation model whose four set-abstraction modules add the attention output to the
max pool (attention_layer.pointnet_sa_module_attention_and_pooling, :29-52), on the gfx950
kernels.

Layer table, scopes, feature propagation and head are pointnet2_sem_seg's: built from
pointnet2_sem_seg.model_body.
"""
from functools import partial

from .attention_layer import pointnet_sa_module_attention_and_pooling
from .pointnet2_sem_seg import SA_LAYERS, get_loss, model_body  # noqa: F401

SA_MODULES = (pointnet_sa_module_attention_and_pooling,) * len(SA_LAYERS)
body = partial(model_body, sa_modules=SA_MODULES)  # model_body's signature, for train_step(model=)


def get_model(point_cloud, is_training, num_class, bn_decay=None, params=None):
    """point_cloud (B, N, 3) -> (logits (B, N, num_class), end_points with 'l0_xyz' and
    'feats'). Extra keyword `params`: the ParamStore (default: tf_util.default_store())."""
    return body(point_cloud, None, is_training, num_class, bn_decay, params)
