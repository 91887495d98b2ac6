"""attention_points/attention_scannet/pooling_attention_model.py: PointNet++'s SSG segmentation
network with the max pool of every set-abstraction module replaced by the AttentionLayer
(PoolingAttentionNetLayer), on the gfx950 kernels. Constructor, keywords, __call__,
get_end_points and body as attention_models' classes.

The levels' features are 16 * out_dim = 1024, 2048, 4096 and 8192 wide, so l3 and l4 read 2051
and 4099 channels and the first two feature-propagation modules 12288 and 2304: the first layer of
each of those MLPs is wider than the fused kernel takes and runs on the K-streamed kernel
(pn2_dense_wide, csrc/mlp_wide.hip) with ParamStore(wide_layers="hip"), from torch ops with the
default wide_layers="torch" (attention_layer.run_layers; DESIGN.md §3.5c lists them).
"""
from .attention_models import _Model, get_loss  # noqa: F401
from .pooling_attention_layer import PoolingAttentionNetLayer

# (out_dim, mlp) of l1..l4 (:20-27)
POOLING_LAYERS = ((64, [32, 32, 64]), (128, [64, 64, 128]), (256, [128, 128, 256]),
                  (512, [256, 256, 512]))


class PoolingAttentionNetModel(_Model):
    """pooling_attention_model.py:17-93: inputs = the cloud (B, N, 3). Variables 'l<k>/conv<i>/...'
    and 'l<k>/attention/...' of the four layers, 'fa_layer<k>/conv_<i>/...', 'fc1/...', 'fc2/...'."""

    def build_layers(self):
        return [PoolingAttentionNetLayer(npoint=n, out_dim=d, radius=self.radius, nsample=32,
                                         bn_decay=self.bn_decay, is_training=self.is_training,
                                         mlp=mlp, scope=f"l{k + 1}", params=self.params)
                for k, (n, (d, mlp)) in enumerate(zip(self.npoints, POOLING_LAYERS))]

    def call_layer(self, layer, xyz, points, is_training, bn_decay):
        return layer([xyz, points], is_training, bn_decay)
