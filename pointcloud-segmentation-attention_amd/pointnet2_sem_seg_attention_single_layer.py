"""attention_points/models/pointnet2_sem_seg_attention_single_layer.py: the SSG
semantic-segmentation model with attention in ONE set-abstraction module and max pooling in the
other three (:29-57), on the gfx950 kernels.

Layer table, scopes, feature propagation and head are pointnet2_sem_seg's: built from
pointnet2_sem_seg.model_body.
"""
from functools import partial

from .attention_layer import pointnet_sa_module_attention
from .pointnet2_sem_seg import SA_LAYERS, get_loss, model_body  # noqa: F401
from .pointnet_util import pointnet_sa_module


def sa_modules(attention_layer_idx):
    """The four SA modules: attention at attention_layer_idx (0..3), max pooling elsewhere
    (pointnet_sa_wrapper, :13-26)."""
    assert (0 <= attention_layer_idx < 4)  # :43
    return tuple(pointnet_sa_module_attention if k == attention_layer_idx else pointnet_sa_module
                 for k in range(len(SA_LAYERS)))


def body(attention_layer_idx):
    """model_body with this model's SA modules: model_body's signature, for
    train_step(model=)."""
    return partial(model_body, sa_modules=sa_modules(attention_layer_idx))


def get_model(point_cloud, attention_layer_idx, is_training, num_class, bn_decay=None,
              params=None):
    """point_cloud (B, N, 3), attention_layer_idx in 0..3 -> (logits (B, N, num_class),
    end_points with 'l0_xyz' and 'feats'). Extra keyword `params`: the ParamStore (default:
    tf_util.default_store())."""
    return body(attention_layer_idx)(point_cloud, None, is_training, num_class, bn_decay, params)
