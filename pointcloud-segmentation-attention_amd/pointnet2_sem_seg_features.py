"""attention_points/models/pointnet2_sem_seg_features.py: the SSG semantic-segmentation model
whose input points carry features (colour and normals), the default model of the reference's
training loop (attention_points/train.py:138), on the gfx950 kernels.

It is pointnet2_sem_seg.get_model with l0_points = features (:25): the first set-abstraction
module groups [xyz, features] and the last feature-propagation module concatenates the features
to the interpolated ones. Both models are built from pointnet2_sem_seg.model_body.
"""
from .pointnet2_sem_seg import get_loss, model_body  # noqa: F401


def get_model(point_cloud, features, is_training, num_class, bn_decay=None, params=None):
    """point_cloud (B, N, 3), features (B, N, C) -> (logits (B, N, num_class), end_points with
    'l0_xyz' and 'feats'). Extra keyword `params`: the ParamStore (default:
    tf_util.default_store())."""
    return model_body(point_cloud, features, is_training, num_class, bn_decay, params)
