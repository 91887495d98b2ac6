"""pn2hip — MI355X-native PointNet++ geometric hot path for the attention segmentation models of
tpfeifle/pointcloud-segmentation-attention.

Drop-in modules (reference names, argument order, shapes, dtypes, error messages):
  tf_sampling     farthest_point_sample, gather_point (+grad)
  tf_grouping     query_ball_point, group_point (+grad)
  tf_interpolate  three_nn, three_interpolate (+grad)
  pointnet_util   sample_and_group(_all/_msg), group_pool, fp_interpolate,
                  pointnet_sa_module(_msg), pointnet_fp_module (fused group/interp + MLP + pool)
  tf_util         conv2d / conv1d (1x1), dropout, sparse_softmax_cross_entropy, ParamStore,
                  SharedMLP
  pointnet2_sem_seg      get_model, get_loss (the SSG segmentation model and its weighted loss)
  pointnet2_sem_seg_features  get_model(point_cloud, features, ...): the same model on points
                         that carry features
  train                  get_learning_rate, get_bn_decay, AdamOptimizer, SegMetrics, train_step,
                         eval_step (attention_points/train.py's optimiser, schedules, metrics
                         and validation step)
  data_transformation    get_subset (the ScanNet crop sampler) on the GPU, label_map
  generate_predictions   map_back, map_to_nyu40, export_ids, predict_scene, generate_predictions
                         (attention_points/benchmark: a label for every point of a scene)
  evaluate               evaluate_scan, get_iou, evaluate, write_result_file (the ScanNet
                         benchmark score)
  complete_scene_loader  the whole-scene chunker (selection + gathers on the GPU)
  attention_layer attention_reduce, AttentionLayer
Everything runs the gfx950 kernels of libpn2hip.so (C ABI: include/pn2hip.h).

The directory name has hyphens, so import it with importlib:
    pn2 = importlib.import_module("pointcloud-segmentation-attention_amd")
"""
from . import attention_layer, complete_scene_loader, data_transformation, evaluate, generate_predictions, grid, \
    plan, pointnet2_sem_seg, pointnet2_sem_seg_features, pointnet_util, shard, stack, synth, tf_grouping, \
    tf_interpolate, tf_sampling, tf_util, train
from .generate_predictions import predict_scene
from .train import AdamOptimizer, SegMetrics, eval_step, get_bn_decay, get_learning_rate, train_step
from ._lib import LIB_PATH, InvalidArgumentError, Pn2RuntimeError, lib

__all__ = ["tf_sampling", "tf_grouping", "tf_interpolate", "pointnet_util", "attention_layer", "grid", "tf_util", "data_transformation", "complete_scene_loader",
           "synth", "stack", "shard", "plan", "pointnet2_sem_seg", "pointnet2_sem_seg_features", "train",
           "generate_predictions", "evaluate", "predict_scene", "eval_step",
           "AdamOptimizer", "SegMetrics", "get_learning_rate", "get_bn_decay", "train_step", "lib", "LIB_PATH", "InvalidArgumentError", "Pn2RuntimeError"]
