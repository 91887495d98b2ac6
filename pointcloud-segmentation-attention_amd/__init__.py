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
  pointnet2_sem_seg_attention, pointnet2_sem_seg_attention_and_pooling,
  pointnet2_sem_seg_attention_single_layer  the three attention models' get_model
  train                  get_learning_rate, get_bn_decay, AdamOptimizer, SegMetrics, train_step,
                         eval_step, train_step_with, CLASS_WEIGHTS, get_data_tensors, eval_model, train
                         (attention_points/train.py: optimiser, schedules, metrics, the batch
                         feed, the validation pass and the epoch loop)
  data_transformation    get_subset (the ScanNet crop sampler) on the GPU, label_map,
                         random_rotate, get_all_subsets_for_scene_numpy / scene_val_chunks (the
                         validation chunker)
  compute_class_weights  weights_from_counts, get_weights
  generate_predictions   map_back, map_to_nyu40, export_ids, predict_scene, generate_predictions
                         (attention_points/benchmark: a label for every point of a scene)
  evaluate               evaluate_scan, get_iou, evaluate, write_result_file (the ScanNet
                         benchmark score)
  complete_scene_loader  the whole-scene chunker (selection + gathers on the GPU)
  attention_layer attention_reduce, AttentionLayer (any key_dim % 4 == 0), and the attention
                  networks' layers: InnerAttentionLayer, FeedForwardLayer, InnerAttentionBlock,
                  AttentionNetLayer, AttentionNetMLPLayer
  pooling_attention_layer  PoolingAttentionNetLayer
  attention_models         AttentionNetModel, AttentionNetFeatureModel, AttentionNetMLPModel
  pooling_attention_model  PoolingAttentionNetModel
  show3d_balls           showpoints: the reference's ball viewer, headless (the image comes back as
                         a device tensor; any number of views per call)
  visualization          label_colors, mask_unannotated, orbit, render_scene, animate_prediction,
                         labels_over_training (attention_points/visualization: a scene coloured
                         by label, as frames on disk)
Everything runs the gfx950 kernels of libpn2hip.so (C ABI: include/pn2hip.h).

The directory name has hyphens, so import it with importlib:
    pn2 = importlib.import_module("pointcloud-segmentation-attention_amd")
"""
from . import attention_layer, attention_models, complete_scene_loader, compute_class_weights, data_transformation, evaluate, \
    generate_predictions, grid, plan, pointnet2_sem_seg, pointnet2_sem_seg_attention, \
    pointnet2_sem_seg_attention_and_pooling, pointnet2_sem_seg_attention_single_layer, \
    pointnet2_sem_seg_features, pointnet_util, pooling_attention_layer, pooling_attention_model, shard, show3d_balls, stack, synth, tf_grouping, tf_interpolate, tf_sampling, \
    tf_util, train, visualization
from .data_transformation import random_rotate, rotation_cs, scene_val_chunks
from .generate_predictions import predict_scene
from .train import (CLASS_WEIGHTS, AdamOptimizer, SegMetrics, eval_model, eval_step, get_bn_decay,
                    get_data_tensors, get_learning_rate, train_step, train_step_with)
from ._lib import LIB_PATH, InvalidArgumentError, Pn2RuntimeError, lib

__all__ = ["tf_sampling", "tf_grouping", "tf_interpolate", "pointnet_util", "attention_layer", "grid", "tf_util", "data_transformation", "complete_scene_loader",
           "synth", "stack", "shard", "plan", "pointnet2_sem_seg", "pointnet2_sem_seg_features", "train",
           "generate_predictions", "evaluate", "predict_scene", "eval_step",
           "pointnet2_sem_seg_attention", "pointnet2_sem_seg_attention_and_pooling",
           "pointnet2_sem_seg_attention_single_layer", "attention_models", "pooling_attention_layer",
           "pooling_attention_model", "compute_class_weights", "show3d_balls", "visualization", "random_rotate", "rotation_cs",
           "scene_val_chunks", "CLASS_WEIGHTS", "get_data_tensors", "eval_model", "train_step_with",
           "AdamOptimizer", "SegMetrics", "get_learning_rate", "get_bn_decay", "train_step", "lib", "LIB_PATH", "InvalidArgumentError", "Pn2RuntimeError"]
