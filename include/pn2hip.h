/*
 * pn2hip.h — C ABI of the MI355X (gfx950) PointNet++ geometric hot path.
 *
 * This is the drop-in boundary. Each entry point replaces one TensorFlow custom op (or one
 * inline TF graph fragment) of the reference and keeps its argument meaning:
 *
 *   reference op / fragment                                     → entry point here
 *   FarthestPointSample  tf_sampling.cpp:94-123, .cu:105-170     → pn2_fps (+_gather, _chain)
 *   GatherPoint          tf_sampling.cpp:125-148, .cu:172-181    → pn2_gather_point
 *   GatherPointGrad      tf_sampling.cpp:150-178, .cu:183-192    → pn2_gather_point_grad
 *   ProbSample           tf_sampling.cpp:66-92, .cu:7-104,197-201 → pn2_prob_sample
 *   QueryBallPoint       tf_grouping.cpp:66-106, _g.cu:3-36      → pn2_ball_query,
 *                                                                  pn2_ball_query_grid
 *   SelectionSort        tf_grouping.cpp:108-137, _g.cu:83-123   → pn2_select_top_k
 *   knn_point            tf_grouping.py:48-73                    → pn2_knn_point
 *   GroupPoint           tf_grouping.cpp:139-171, _g.cu:40-57    → pn2_group_point
 *   GroupPointGrad       tf_grouping.cpp:174-208, _g.cu:61-78    → pn2_group_point_grad
 *   ThreeNN              tf_interpolate.cpp:157-187, :60-103     → pn2_three_nn,
 *                                                                  pn2_three_nn_grid,
 *                                                                  pn2cpu_three_nn (host)
 *   ThreeInterpolate     tf_interpolate.cpp:191-222, :107-127    → pn2_three_interpolate,
 *                                                                  pn2cpu_three_interpolate
 *   ThreeInterpolateGrad tf_interpolate.cpp:225-262, :131-153    → pn2_three_interpolate_grad,
 *                                                                  pn2cpu_three_interpolate_grad
 *   IDW weights          pointnet_util.py:219-222                → pn2_idw_weights
 *   sample_and_group     pointnet_util.py:16-58 (SSG), :180-191  → pn2_sample_and_group,
 *                                                                  pn2_group_concat
 *   pointnet_fp_module   pointnet_util.py:218-226 (geometry)     → pn2_fp_fused,
 *                                                                  pn2_fp_grid_fused,
 *                                                                  pn2_fp_apply
 *   AttentionLayer.call  attention_layer.py:29-45 (reduction)    → pn2_attn_reduce,
 *                                                                  pn2_attn_reduce_grad
 *   SA pooling           pointnet_util.py:130-145, :200          → pn2_group_pool
 *   pointnet_sa_module   pointnet_util.py:106-145 (group, conv2d  → pn2_group_mlp
 *     MLP, pooling; tf_util.py:120-185 conv2d + batch_norm)
 *   pointnet_sa_module_attention(_and_pooling)                   → pn2_group_mlp_attention
 *                        attention_layer.py:229-338
 *   pointnet_fp_module   pointnet_util.py:218-238 (interp + MLP)  → pn2_fp_mlp
 *   conv1d head          tf_util.py:52-117, pointnet2_sem_seg.py  → pn2_shared_mlp
 *                        :57-60 (fc1, fc2)
 *   conv2d, is_training  tf_util.py:165-185, :512-531 (batch     → pn2_bn_stats, pn2_bn_act_fwd,
 *                        statistics) and its gradients             pn2_bn_act_bwd, pn2_mlp_wgrad
 *                        (bf16 mode: the weight gradient)           pn2_mlp_wgrad_bf16
 *   conv2d, is_training, pointnet_util.py:106-136 (the last MLP  → pn2_bn_act_pool_fwd,
 *     + max pool         layer and reduce_max over nsample)        pn2_bn_act_pool_bwd
 *   AttentionLayer,      attention_layer.py:10-45, :256-259, :303 → pn2_attn_kv_reduce,
 *     is_training        (K and V projected together, and the     pn2_attn_kv_reduce_grad,
 *                        gradients)                                pn2_attn_dx_scatter,
 *                                                                  pn2_col_sum
 *   dropout, is_training tf_util.py:594-612, pointnet2_sem_seg.py:56 → pn2_dropout,
 *                                                                  pn2cpu_dropout (host)
 *   get_loss             pointnet2_sem_seg.py:62-69 (tf.losses.    → pn2_softmax_xent_fwd,
 *                        sparse_softmax_cross_entropy + weights)   pn2_softmax_xent_bwd
 *   tf.train.AdamOptimizer attention_points/train.py:318-319 (TF 1.x → pn2_adam_step,
 *                        ApplyAdam, no Nesterov)                   pn2cpu_adam_step (host)
 *   get_metrics          attention_points/train.py:145-163         → pn2_seg_confusion,
 *                        (accuracy over the annotated points,      pn2_mean_iou,
 *                        streaming tf.metrics.mean_iou)            pn2cpu_seg_confusion,
 *                                                                  pn2cpu_mean_iou (host)
 *   get_subset          scannet_dataset/data_transformation.py  → pn2_scene_bbox,
 *                        :70-154 (training crop sampler)           pn2_crop_sample
 *   whole-scene chunker  scannet_dataset/complete_scene_loader.py → pn2_subvolume_select,
 *                        :4-117 (subvolume selection, gathers)     pn2_gather_rows
 *   generate_predictions attention_points/benchmark/             → pn2_scene_vote,
 *                        generate_predictions.py:139-186 (argmax,   pn2_scene_labels,
 *                        map_back :19-37, map_to_nyu40 :40-53);     pn2_map_back_rows,
 *                        benchmark/evaluate.py:58-108 and           pn2_label_lut,
 *                        data_transformation.py:21-67 (label        pn2cpu_scene_vote, ...
 *                        look-ups)                                  (host twins)
 *   render_ball          pointnet2_tensorflow/utils/              → pn2_render_ball,
 *                        render_balls_so.cpp:14-56 and the          pn2_render_project,
 *                        projection of show3d_balls.py:52-74        pn2cpu_render_* (host twins)
 *
 * (reference paths are under pointnet2_tensorflow/tf_ops/{sampling,grouping,interpolation_3d},
 *  pointnet2_tensorflow/utils and attention_points/attention_scannet.)
 *
 * Conventions (all entry points):
 *  - every buffer is a caller-owned DEVICE pointer, row-major, channel-last, contiguous;
 *    float = IEEE fp32, indices int32 — the reference's tensor dtypes;
 *  - every launch goes on `stream` (a hipStream_t; NULL = legacy default stream); nothing
 *    synchronises, nothing allocates on the device (the first sampler call pins one 4-byte
 *    host word for device fault codes), so every call can be captured into a hipGraph;
 *  - return 0 on success, PN2_EINVAL (-22) for a shape/attribute error (where the reference
 *    raises InvalidArgument through OP_REQUIRES), PN2_EFAULT (-14) when an earlier sampler
 *    launch reported a device fault (pn2_fault_status), or a positive hipError_t from the
 *    launch;
 *  - alignment: every pointer needs its element's natural alignment (4 bytes for float and
 *    int32_t, 8 for the 64-bit keys and counters) and nothing more, unless the entry point
 *    says otherwise. Rows, clouds and batches are dense (no strides) unless the entry point takes a
 *    leading dimension (ld / col0). The kernels that use
 *    16-byte loads and stores choose them per launch from the pointers they are given and
 *    take a per-element path for any other pointer, with the same arithmetic in the same
 *    order: the bits of the result do not depend on the alignment. The exceptions, which
 *    return PN2_EINVAL for a pointer that is not 16-byte aligned before any launch:
 *    pn2_copy_f4, pn2_attn_reduce, pn2_attn_reduce_layers, pn2_attn_reduce_grad,
 *    pn2_attn_kv_reduce, pn2_attn_kv_reduce_grad (all buffers), pn2_group_mlp_attention (out, bn_scale and
 *    bn_shift; its other buffers follow the general rule), the `packed` weights of
 *    pn2_mlp_layer / pn2_mlp_pack, every grid (pn2_grid_size bytes) and the inverse index
 *    `inv`. The torch and Python front ends copy a misaligned tensor argument of those
 *    functions to a fresh allocation first.
 */
#ifndef PN2HIP_H
#define PN2HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* pn2_stream_t; /* hipStream_t */

#define PN2_OK 0
#define PN2_EINVAL (-22)
#define PN2_EFAULT (-14) /* an earlier launch stored a device fault code (pn2_fault_status)   */
#define PN2_ENOTSUP (-95) /* valid arguments this device / path does not take (see each call)  */

/* device fault codes (pn2_fault_status) */
#define PN2_FAULT_FPS_POLL 1 /* culled sampler: a cold wave waited past its poll bound for
                                 centres the hot wave never published; that launch's indices
                                 are not trustworthy                                      */

/* pn2_fps_gather_sched schedules (all give identical outputs) */
#define PN2_FPS_AUTO 0           /* the library's choice by N (what pn2_fps* run)            */
#define PN2_FPS_BLOCKSCAN 1      /* one block-wide argmax per pick (the v9 register sampler) */

/* flags of pn2_group_concat / pn2_sample_and_group */
#define PN2_USE_XYZ 1  /* concat the centred xyz with the grouped features (use_xyz=True)      */
#define PN2_XYZ_LAST 2 /* MSG order [points, xyz] (pointnet_util.py:191) instead of SSG
                          [xyz, points] (pointnet_util.py:52)                                 */

/* pn2_group_pool modes (pointnet_util.py:130-145) */
#define PN2_POOL_MAX 0
#define PN2_POOL_AVG 1
#define PN2_POOL_WEIGHTED_AVG 2
#define PN2_POOL_MAX_AND_AVG 3
#define PN2_POOL_NONE (-1) /* pn2_group_mlp: per-point output, no pooling */

/* shared-MLP layers (pn2_group_mlp / pn2_fp_mlp / pn2_shared_mlp) */
#define PN2_MLP_MAX_LAYERS 6
#define PN2_MLP_RELU 1 /* activation_fn = tf.nn.relu (tf_util.conv2d's default) */
#define PN2_MLP_BF16 2 /* `packed` is pn2_mlp_pack_bf16's output: the layer's product runs on the
                          bf16 matrix cores (opt-in; the contract is at pn2_mlp_pack_bf16)     */

typedef struct pn2_mlp_layer {
  const void* packed; /* pn2_mlp_pack / pn2_mlp_pack_bf16 output (device, 16-byte aligned) */
  int cin, cout;      /* the conv's input / output channels                              */
  int flags;          /* PN2_MLP_RELU | PN2_MLP_BF16; PN2_MLP_BF16 must be set exactly when
                         `packed` came from pn2_mlp_pack_bf16 (the two layouts differ and
                         nothing in the buffer tells them apart)                          */
} pn2_mlp_layer;

const char* pn2_version(void);
const char* pn2_strerror(int status);

/* Measurement utility (bench.py's copy peak; no operator uses it): copy `bytes` (a multiple
 * of 16, both pointers 16-byte aligned) with float4 loads and stores over 16 workgroups per
 * CU of `cus` CUs. */
int pn2_copy_f4(const void* src, void* dst, size_t bytes, int cus, pn2_stream_t stream);

/* ---------------------------------------------------------------- sampling -------------- */

/* Farthest-point sampling. xyz (B,N,3) → idx (B,npoint). idx[b,0]=0; each next index is the
 * argmax of the running min squared distance, ties broken exactly like the reference's
 * 512-thread block reduction: smallest (k mod 512), then smallest (k div 512)
 * (tf_sampling_g.cu:130-165). Distances are ((dx*dx+dy*dy)+dz*dz) in fp32 without FMA.
 * npoint must be > 0 (tf_sampling.cpp:99). N <= PN2_FPS_MAX_POINTS (= pn2_fps_max_points())
 * needs no workspace; larger N must use pn2_fps_ws. */
#define PN2_FPS_MAX_POINTS 16384
int pn2_fps(const float* xyz, int B, int N, int npoint, int32_t* idx, pn2_stream_t stream);
/* Same, also writing new_xyz (B,npoint,3) = gather_point(xyz, idx) (pointnet_util.py:34). */
int pn2_fps_gather(const float* xyz, int B, int N, int npoint, int32_t* idx, float* new_xyz,
                   pn2_stream_t stream);
int pn2_fps_max_points(void);
/* pn2_fps_gather with an explicit sampler schedule, per call (no process-wide state; used by
 * the parity tests and A/B timing). PN2_FPS_AUTO = pn2_fps_gather; the other schedules exist
 * only where the culled hot-set sampler is the default (4096 < N <= 16384) and return
 * PN2_EINVAL elsewhere. */
int pn2_fps_gather_sched(const float* xyz, int B, int N, int npoint, int32_t* idx,
                         float* new_xyz, int schedule, pn2_stream_t stream);
/* The device fault word: 0, or the PN2_FAULT_* code a sampler launch stored (valid once that
 * launch's stream has synchronised). clear != 0 resets it. The next pn2_fps* call also
 * reports a stored fault, as PN2_EFAULT, and resets it. */
int pn2_fault_status(int clear);
size_t pn2_fps_workspace_size(int B, int N);
int pn2_fps_ws(const float* xyz, int B, int N, int npoint, int32_t* idx, float* new_xyz,
               void* workspace, size_t workspace_bytes, pn2_stream_t stream);

/* The SSG sampler chain: stage 0 samples npoint[0] of the N points of each cloud, stage i
 * samples npoint[i] of stage i-1's output (pointnet2_sem_seg*.py:29-50 samples
 * 8192 -> 1024 -> 256 -> 64 -> 16). idx[i] (B,npoint[i]) and new_xyz[i] (B,npoint[i],3) are
 * exactly what pn2_fps_gather returns for that stage's input. N <= PN2_FPS_MAX_POINTS,
 * npoint[i] <= PN2_FPS_CHAIN_MAX_FEED for every stage that feeds another, 1 <= nstages <=
 * PN2_FPS_CHAIN_MAX_STAGES. Host arrays of device pointers. At most two launches on `stream`:
 * a first stage over N > PN2_FPS_CHAIN_MAX_FEED points as the ordinary sampler, then every
 * remaining stage fused in one launch, one workgroup per cloud. Where those stages can be
 * prefixes of their input (they are when that input is itself a sampler's output -- SA2
 * sampling SA1's picks -- and no two points tie), the workgroup
 * checks that over every point of its cloud and writes the stages as copies of the prefix;
 * a cloud that fails the check (ties, duplicates, non-finite coordinates) has its stages run
 * as samplers by the same workgroup, the same picks either way (csrc/fps.hip
 * fps_chain_prefix_kernel). A single stage or stages that are not nested run on the hot-set
 * schedule (fps_chain_kernel). No output buffer is used as scratch. */
#define PN2_FPS_CHAIN_MAX_FEED 1024
#define PN2_FPS_CHAIN_MAX_STAGES 4
int pn2_fps_chain(const float* xyz, int B, int N, int nstages, const int* npoint,
                  int32_t* const* idx, float* const* new_xyz, pn2_stream_t stream);
/* pn2_fps_chain plus the automatic-edge grid of stage 0's picks (the known points of the last
 * FP layer, pointnet2_sem_seg*.py:55 / pointnet_util.py:218): grid0 (pn2_grid_size(B,
 * npoint[0]) bytes, 16-byte aligned) gets exactly what pn2_grid_build(new_xyz[0], B,
 * npoint[0], 0, grid0) writes, up to the order of the points inside a cell. The culled
 * sampler builds it in its own workgroups after the last pick (npoint[0] <= 4096; otherwise
 * one pn2_grid_build launch follows on `stream`). new_xyz[0] must not be NULL. */
int pn2_fps_chain_grid(const float* xyz, int B, int N, int nstages, const int* npoint,
                       int32_t* const* idx, float* const* new_xyz, void* grid0,
                       size_t grid0_bytes, pn2_stream_t stream);
/* out (B,M,3) = inp[b, idx[b,j], :]; inp must have 3 channels (tf_sampling.cpp:131). */
int pn2_gather_point(const float* inp, const int32_t* idx, int B, int N, int M, float* out,
                     pn2_stream_t stream);
/* inp_g (B,N,3) = scatter-add of out_g (B,M,3) at idx; zero-fills inp_g first
 * (tf_sampling.cpp:174). Float atomics: summation order is not fixed. */
int pn2_gather_point_grad(const float* out_g, const int32_t* idx, int B, int N, int M,
                          float* inp_g, pn2_stream_t stream);
/* Categorical sampling (ProbSample). inp (B,N) weights, inpr (B,M) uniform draws in [0,1) →
 * out (B,M): per row, the first index whose inclusive prefix sum of inp reaches
 * inpr * (the row total), found by the reference's binary search (tf_sampling_g.cu:90-104).
 * The prefix sum repeats cumsumKernel's fp32 addition order (:7-88), so the indices equal
 * the reference's. workspace: pn2_prob_sample_workspace_size(B, N) bytes (the prefix sums,
 * tf_sampling.cpp:85-88). N = 0 with M > 0 is rejected (the reference reads cum[-1]). */
size_t pn2_prob_sample_workspace_size(int B, int N);
int pn2_prob_sample(const float* inp, const float* inpr, int B, int N, int M, float* workspace,
                    size_t workspace_bytes, int32_t* out, pn2_stream_t stream);

/* ---------------------------------------------------------------- grouping -------------- */

/* Ball query. For every query j: the first `nsample` points of xyz1 (in index order) with
 * max(sqrtf(d2),1e-20f) < radius; remaining slots repeat the first hit; pts_cnt = number
 * found (<= nsample) (tf_grouping_g.cu:3-36). A query with no hit gets idx 0 and pts_cnt 0
 * (the reference leaves that row uninitialised). radius > 0, nsample > 0
 * (tf_grouping.cpp:71,74). */
int pn2_ball_query(const float* xyz1, const float* xyz2, int B, int N, int M, float radius,
                   int nsample, int32_t* idx, int32_t* pts_cnt, pn2_stream_t stream);
/* The float T with  d2 < T  <=>  max(sqrtf(d2),1e-20f) < radius  for every fp32 d2 >= 0.
 * Host function (pure, no GPU). */
float pn2_ball_threshold(float radius);
/* ---- spatial grid (grid.h): the same results as the scans, faster on large clouds ----- *
 * pn2_grid_build: per cloud, bbox + counting sort of xyz (B,N,3) into cells of edge
 *   `cell_edge` (<= 0: ~2 points per cell of the bbox), grown until at most 32768 cells, into
 *   `grid` = caller-owned device memory of pn2_grid_size(B, N) bytes, 16-byte aligned.
 * pn2_ball_query_grid: pn2_ball_query over a grid built on xyz1 (cell_edge = radius is the
 *   fast choice; any radius > 0 is exact). N <= 131072.
 * pn2_three_nn_grid (interpolation section): three_nn over a grid built on the known points.
 * Where the front ends (csrc/torch_ops.cpp, tf_grouping.py, tf_interpolate.py) switch from the
 * scans to the grid, a speed choice only: a ball query over N >= PN2_BALL_GRID_MIN_POINTS points
 * with B * M >= PN2_BALL_GRID_MIN_QUERIES queries, a three_nn over n * m >=
 * PN2_NN_GRID_MIN_PAIRS pairs per cloud with m >= PN2_NN_GRID_MIN_KNOWN known points. */
#define PN2_BALL_GRID_MIN_POINTS 2048
#define PN2_BALL_GRID_MIN_QUERIES 1024
#define PN2_NN_GRID_MIN_PAIRS (1 << 21)
#define PN2_NN_GRID_MIN_KNOWN 512
size_t pn2_grid_size(int B, int N);
int pn2_grid_build(const float* xyz, int B, int N, float cell_edge, void* grid,
                   size_t grid_bytes, pn2_stream_t stream);
int pn2_ball_query_grid(const void* grid, const float* xyz2, int B, int N, int M, float radius,
                        int nsample, int32_t* idx, int32_t* pts_cnt, pn2_stream_t stream);
/* pn2_ball_query_grid plus the grouping of an xyz-only layer in the same kernel:
 * grouped_xyz (B,M,nsample,3) = xyz1[idx] - xyz2, i.e. pn2_group_concat with points = NULL
 * (pointnet_util.py:39-40, 55-56), bit for bit. xyz1 (B,N,3) is the cloud the grid was built
 * over. */
int pn2_ball_group_xyz_grid(const void* grid, const float* xyz1, const float* xyz2, int B, int N,
                            int M, float radius, int nsample, int32_t* idx, int32_t* pts_cnt,
                            float* grouped_xyz, pn2_stream_t stream);
/* pn2_ball_group_xyz_grid with features: ONE kernel for query_ball_point + group_point + the
 * centring and concat of sample_and_group (tf_grouping_g.cu:3-57, pointnet_util.py:38-52; MSG
 * order :186-191). new_points (B,M,nsample,3+C) = [xyz1[idx] - xyz2, points[idx]], or with
 * flags & PN2_XYZ_LAST [points[idx], xyz1[idx] - xyz2]; flags must hold PN2_USE_XYZ when C > 0
 * (C = 0: exactly pn2_ball_group_xyz_grid). idx / pts_cnt as pn2_ball_query_grid. Bit for bit
 * pn2_ball_query_grid followed by pn2_group_concat. */
int pn2_ball_group_grid(const void* grid, const float* xyz1, const float* points, int C,
                        int flags, const float* xyz2, int B, int N, int M, float radius,
                        int nsample, int32_t* idx, int32_t* pts_cnt, float* new_points,
                        pn2_stream_t stream);
/* pn2_ball_group_xyz_grid for nr radii (1 <= nr <= PN2_BQ_MAX_RADII) of the same queries in
 * ONE launch (MSG's SA1: pointnet_util.py:162-203, the radius loop): the cells of the largest
 * radius are walked once and every candidate is tested against each radius. Per radius r:
 * radii[r], nsample[r], idx[r] (B,M,nsample[r]), pts_cnt[r] (B,M), grouped_xyz[r]
 * (B,M,nsample[r],3) -- each exactly pn2_ball_group_xyz_grid's output for that radius. The
 * pointer arrays are host memory. The nr bitmasks per wave must fit 64 KB of LDS:
 * nr * ceil(N / 32) <= 4096 (PN2_EINVAL beyond: one launch per radius). */
#define PN2_BQ_MAX_RADII 3
int pn2_ball_group_xyz_grid_radii(const void* grid, const float* xyz1, const float* xyz2, int B,
                                  int N, int M, int nr, const float* radii, const int* nsample,
                                  int32_t* const* idx, int32_t* const* pts_cnt,
                                  float* const* grouped_xyz, pn2_stream_t stream);

/* ---- k nearest neighbours ---------------------------------------------------------- *
 * pn2_select_top_k: select_top_k / SelectionSort (tf_grouping.py:22-31, tf_grouping_g.cu:
 *   83-123): outi, out (B,m,n) = each row of dist (B,m,n) after the reference's k-step
 *   partial selection sort (first minimum by position, swapped to the front), i.e. the k
 *   smallest first, ties in the order those swaps leave them, the rest permuted by the same
 *   swaps. 0 < k <= min(n, 1024). workspace: pn2_select_top_k_workspace_size(B,m,k) bytes.
 * pn2_knn_point: knn_point (tf_grouping.py:48-73): val, idx (B,m,k) = the first k columns of
 *   select_top_k(k, dist) for dist[b,j,t] = sum over the c channels of (xyz1[b,t]-xyz2[b,j])^2
 *   (summed left to right); the (B,m,n) matrix is never materialised. */
int pn2_select_top_k(const float* dist, int B, int m, int n, int k, int32_t* outi, float* out,
                     int32_t* workspace, pn2_stream_t stream);
size_t pn2_select_top_k_workspace_size(int B, int m, int k);
int pn2_knn_point(const float* xyz1, const float* xyz2, int B, int n, int m, int c, int k,
                  float* val, int32_t* idx, pn2_stream_t stream);

/* out (B,M,nsample,C) = points[b, idx[b,j,k], :] (tf_grouping_g.cu:40-57). */
int pn2_group_point(const float* points, const int32_t* idx, int B, int N, int C, int M,
                    int nsample, float* out, pn2_stream_t stream);
/* grad_points (B,N,C) = scatter-add of grad_out (B,M,nsample,C); zero-fills first
 * (tf_grouping.cpp:204, tf_grouping_g.cu:61-78). Float atomics. */
int pn2_group_point_grad(const float* grad_out, const int32_t* idx, int B, int N, int C, int M,
                         int nsample, float* grad_points, pn2_stream_t stream);

/* Fused group + centre + concat (pointnet_util.py:39-56 SSG, :186-193 MSG):
 *   grouped_xyz (B,M,nsample,3) = xyz[idx] - new_xyz[j]            (optional, may be NULL)
 *   new_points  (B,M,nsample,Cout):
 *     points == NULL          → Cout = 3,      grouped_xyz
 *     !(flags & PN2_USE_XYZ)  → Cout = C,      points[idx]
 *     flags & PN2_XYZ_LAST    → Cout = C + 3,  [points[idx], grouped_xyz]   (MSG)
 *     otherwise               → Cout = 3 + C,  [grouped_xyz, points[idx]]   (SSG) */
int pn2_group_concat(const float* xyz, const float* points, const float* new_xyz,
                     const int32_t* idx, int B, int N, int C, int M, int nsample, int flags,
                     float* grouped_xyz, float* new_points, pn2_stream_t stream);
/* sample_and_group (pointnet_util.py:16-58, knn=False): FPS + gather + ball query + fused
 * group/centre/concat, four launches on `stream`. Outputs as in the reference:
 * fps_idx (B,npoint), new_xyz (B,npoint,3), idx (B,npoint,nsample), pts_cnt (B,npoint),
 * grouped_xyz (B,npoint,nsample,3) (may be NULL), new_points (B,npoint,nsample,Cout). */
int pn2_sample_and_group(const float* xyz, const float* points, int B, int N, int C,
                         int npoint, float radius, int nsample, int flags, int32_t* fps_idx,
                         float* new_xyz, int32_t* idx, int32_t* pts_cnt, float* grouped_xyz,
                         float* new_points, pn2_stream_t stream);

/* Several set-abstraction layers' ball query + fused group/centre/concat in ONE launch
 * (the SSG stack's SA2..SA4, or one MSG level's radii, which all wait for the same sampler).
 * Per layer the outputs equal pn2_ball_query (idx, pts_cnt) followed by pn2_group_concat
 * (new_points, grouped_xyz) with the same arguments, bit for bit. Limits: N <=
 * PN2_SA_GROUP_MAX_POINTS points per cloud (the cloud is staged in LDS), nsample <=
 * PN2_SA_GROUP_MAX_NSAMPLE, at most PN2_SA_MAX_LAYERS layers; every layer has the same B.
 * grouped_xyz may be NULL. */
#define PN2_SA_MAX_LAYERS 4
#define PN2_SA_GROUP_MAX_POINTS 1024
#define PN2_SA_GROUP_MAX_NSAMPLE 128
typedef struct pn2_sa_layer {
  const float* xyz;     /* (B,N,3) */
  const float* points;  /* (B,N,C) or NULL (then C is ignored and Cout = 3) */
  const float* new_xyz; /* (B,M,3) query centres */
  int N, C, M, nsample;
  float radius;
  int flags;            /* PN2_USE_XYZ | PN2_XYZ_LAST, as pn2_group_concat */
  int32_t* idx;         /* (B,M,nsample) */
  int32_t* pts_cnt;     /* (B,M) */
  float* grouped_xyz;   /* (B,M,nsample,3) or NULL */
  float* new_points;    /* (B,M,nsample,Cout) */
} pn2_sa_layer;
int pn2_ball_group_layers(const pn2_sa_layer* layers, int nlayers, int B, pn2_stream_t stream);

/* ---------------------------------------------------------------- interpolation --------- */

/* Three nearest known points (xyz2, (B,m,3)) of every unknown point (xyz1, (B,n,3)):
 * SQUARED distances ascending, ties keep the lower index, m<3 leaves idx 0 / dist +inf
 * (tf_interpolate.cpp:60-103). */
int pn2_three_nn(const float* xyz1, const float* xyz2, int B, int n, int m, float* dist,
                 int32_t* idx, pn2_stream_t stream);
/* out (B,n,C) = ((p[i1]*w1) + (p[i2]*w2)) + (p[i3]*w3)  (tf_interpolate.cpp:107-127). */
int pn2_three_interpolate(const float* points, const int32_t* idx, const float* weight, int B,
                          int m, int C, int n, float* out, pn2_stream_t stream);
/* grad_points (B,m,C) scatter-add (tf_interpolate.cpp:131-153); zero-fills first. */
int pn2_three_interpolate_grad(const float* grad_out, const int32_t* idx, const float* weight,
                               int B, int n, int C, int m, float* grad_points,
                               pn2_stream_t stream);
/* Host twins of the three ops the reference registers ONLY on DEVICE_CPU
 * (tf_interpolate.cpp:187,222,262): the same arguments minus the stream, HOST pointers,
 * synchronous (std::thread over clouds), the reference's fp32 arithmetic and order, so the
 * results equal threenn_cpu / threeinterpolate_cpu / threeinterpolate_grad_cpu bit for bit
 * (the grad's sums keep the reference's order within a cloud). */
int pn2cpu_three_nn(const float* xyz1, const float* xyz2, int B, int n, int m, float* dist,
                    int32_t* idx);
int pn2cpu_three_interpolate(const float* points, const int32_t* idx, const float* weight, int B,
                             int m, int C, int n, float* out);
int pn2cpu_three_interpolate_grad(const float* grad_out, const int32_t* idx, const float* weight,
                                  int B, int n, int C, int m, float* grad_points);
/* weight = (1/d)/sum(1/d), d = max(dist,1e-10)  (pointnet_util.py:219-222). */
int pn2_idw_weights(const float* dist, int B, int n, float* weight, pn2_stream_t stream);
/* pointnet_fp_module geometry (pointnet_util.py:218-226): three_nn + IDW weights +
 * three_interpolate + concat [interp (C2), points1 (C1)] → out (B,n,C2+C1).
 * points1 may be NULL (C1 must then be 0). */
int pn2_fp_fused(const float* xyz1, const float* xyz2, const float* points1, int C1,
                 const float* points2, int C2, int B, int n, int m, float* out,
                 pn2_stream_t stream);

/* Several pn2_fp_fused layers in ONE launch (the FP layers that wait for the same sampler):
 * per layer exactly pn2_fp_fused's output, bit for bit. At most PN2_FP_MAX_LAYERS layers,
 * every layer has the same B. */
#define PN2_FP_MAX_LAYERS 4
typedef struct pn2_fp_layer {
  const float* xyz1;    /* (B,n,3) unknown points */
  const float* xyz2;    /* (B,m,3) known points */
  const float* points1; /* (B,n,C1) or NULL (C1 = 0) */
  const float* points2; /* (B,m,C2) */
  int C1, C2, n, m;
  float* out;           /* (B,n,C2+C1) */
} pn2_fp_layer;
int pn2_fp_fused_layers(const pn2_fp_layer* layers, int nlayers, int B, pn2_stream_t stream);

/* three_nn over pn2_grid_build(xyz2 = the m known points): the same dist/idx as
 * pn2_three_nn. `unknown_grid` (optional, a grid over the n unknown points xyz1) only orders
 * the work so that neighbouring lanes share cells; with it xyz1 may be NULL. */
int pn2_three_nn_grid(const void* known_grid, const void* unknown_grid, const float* xyz1,
                      int B, int n, int m, float* dist, int32_t* idx, pn2_stream_t stream);
/* pn2_fp_fused from a previous three_nn: IDW weights of dist (B,n,3), interpolation of
 * points2 (B,m,C2) with idx (B,n,3), concat [interp, points1 (B,n,C1)]. `unknown_grid`
 * (optional, a grid over the n unknown points) only orders the rows for cache reuse. */
int pn2_fp_apply(const float* dist, const int32_t* idx, const void* unknown_grid,
                 const float* points1, int C1, const float* points2, int C2, int B, int n, int m,
                 float* out, pn2_stream_t stream);
/* pn2_fp_fused for a large search (FP4: n = 8192 unknowns, m = 1024 known) in ONE launch:
 * every workgroup sorts the cloud's m known points into a grid in its own LDS (the automatic
 * edge of pn2_grid_build) and searches it, then writes its rows -- the output of
 * pn2_grid_build + pn2_three_nn_grid + pn2_fp_apply, bit for bit. 1 <= m <=
 * PN2_FP_GRID_MAX_KNOWN (else PN2_EINVAL); PN2_ENOTSUP when the known grid does not fit this
 * device's LDS per workgroup (use those three). `unknown_grid` (optional, a grid over the n unknown points)
 * orders the rows as in pn2_fp_apply; with it xyz1 may be NULL. dist / idx (B,n,3): the
 * three_nn result as well, or both NULL. C1 + C2 >= 1. */
#define PN2_FP_GRID_MAX_KNOWN 4096
int pn2_fp_grid_fused(const float* xyz1, const float* xyz2, const void* unknown_grid,
                      const float* points1, int C1, const float* points2, int C2, int B, int n,
                      int m, float* out, float* dist, int32_t* idx, pn2_stream_t stream);
/* pn2_fp_grid_fused from a grid of the known points built before (known_grid =
 * pn2_grid_build(xyz2, B, m, 0, ...) or pn2_fps_chain_grid's grid0): each workgroup copies
 * its cloud's grid into LDS instead of sorting xyz2 itself. The same output, bit for bit. A
 * grid with more than max(m, 64) cells (an explicit edge) is not staged: the workgroups then
 * build their own from xyz2, which is therefore always required. */
int pn2_fp_grid_fused_known(const void* known_grid, const float* xyz1, const float* xyz2,
                            const void* unknown_grid, const float* points1, int C1,
                            const float* points2, int C2, int B, int n, int m, float* out,
                            float* dist, int32_t* idx, pn2_stream_t stream);

/* ---------------------------------------------------------------- ordered gradients ------ */

/* The gradients of group_point and three_interpolate as gathers in a fixed order
 * (csrc/geom_train.hip): no float atomics, no zero-fill pass, two runs give equal bits. The
 * training path of the SA and FP modules uses them; pn2_group_point_grad and
 * pn2_three_interpolate_grad above keep the reference's atomics.
 *
 * Inverse index. keys (B,S) int32 with values in [0,K): slot s of cloud b points at row
 * keys[b][s]. The index holds, per cloud, offsets[K+1] and the slots grouped by key, each key's
 * slots in ascending slot order: a pure function of `keys`. A key outside [0,K) is never used as
 * an index; its slot is left out (the reference would write out of bounds). Any segment length
 * from 0 to S is handled, all slots on one key included. `inv` is a 16-byte aligned device
 * buffer of at least pn2_inverse_index_size(B,S,K) bytes (a multiple of 16, monotonic in each
 * argument, 0 for B <= 0). Bounds: K <= PN2_INV_MAX_KEYS (the counts of a cloud live in one
 * workgroup's LDS), S <= PN2_INV_MAX_SLOTS, B <= 65535 (clouds are grid rows); beyond them, for a
 * NULL, misaligned or too small buffer: PN2_EINVAL before any launch. B = 0 or S = 0: a no-op. */
#define PN2_INV_MAX_KEYS 16384
#define PN2_INV_MAX_SLOTS (1 << 20)
size_t pn2_inverse_index_size(int B, int S, int K);
int pn2_inverse_index_build(const int32_t* keys, int B, int S, int K, void* inv, size_t inv_bytes,
                            pn2_stream_t stream);
/* grad_points (B,N,C): grad_points[b][n][c] = ((+0.0f + g[s0]) + g[s1]) + ... over the slots
 * s0 < s1 < ... of key n in `inv` = the index of idx (B, M*nsample) with K = N, where
 * g[s] = grad_out[(b*M*nsample + s)*ld + col0 + c]: the source rows are `ld` floats apart and
 * columns [col0, col0+C) are read in place (col0 + C <= ld, else PN2_EINVAL), so the points'
 * columns of group_concat's gradient need no slice copy (ld = C + 3; col0 = 3 in the SSG
 * order, 0 with PN2_XYZ_LAST). Every element is written: a point no group took gets +0.0f.
 * One __fadd_rn per slot. M*nsample = 0: all +0.0f, `inv` is not read. */
int pn2_group_point_grad_ordered(const float* grad_out, int ld, int col0, const void* inv, int B,
                                 int N, int C, int M, int nsample, float* grad_points,
                                 pn2_stream_t stream);
/* grad_points (B,m,C), the same ordered sum over `inv` = the index of idx (B, 3n) with K = m
 * (slot s = 3*i + t), of __fmul_rn(grad_out[(b*n + i)*ld + col0 + c], weight[b][s]): product
 * rounded, then added, no FMA: tf_interpolate.cpp:143-145 in its loop order. With ld = C and
 * col0 = 0 the result equals pn2cpu_three_interpolate_grad bit for bit for any idx in range. */
int pn2_three_interpolate_grad_ordered(const float* grad_out, int ld, int col0, const void* inv,
                                       const float* weight, int B, int n, int C, int m,
                                       float* grad_points, pn2_stream_t stream);

/* ---------------------------------------------------------------- attention / pooling --- */

/* AttentionLayer reduction core (attention_layer.py:35-42) with key_dim = output_dim = 4 (the
 * SA attention modules; any other key_dim: pn2_attn_reduce_kd), heads H = C/4. Q (B,M,C),
 * K,V (B,M,ns,C) → out (B,M,C). Head h reads the CONTIGUOUS
 * block [4*ns*h, 4*ns*(h+1)) of each group's flattened ns*C K/V values as ns rows of 4
 * (the reference's tf.reshape reinterpretation), s = (K_h·q_h)/2, a = softmax(s),
 * out[4h:4h+4] = aᵀ V_h. C must be a multiple of 4; Q, K, V and out 16-byte aligned
 * (PN2_EINVAL otherwise, before any launch). */
int pn2_attn_reduce(const float* Q, const float* K, const float* V, int B, int M, int ns,
                    int C, float* out, pn2_stream_t stream);
/* Several attention reductions of one nsample in ONE launch (the SSG stack's four SA layers,
 * attention_layer.py:35-42 per layer): per layer exactly pn2_attn_reduce(Q, K, V, B, M, ns,
 * C, out); one nsample for every layer, else PN2_EINVAL (an nsample outside {8, 16, 32, 64, 128},
 * or a layer too large for the one-launch task arithmetic, runs as pn2_attn_reduce does).
 * Every layer's Q, K, V and out 16-byte aligned, as for pn2_attn_reduce. */
#define PN2_ATTN_MAX_LAYERS 4
typedef struct pn2_attn_layer {
  const float* Q;
  const float* K;
  const float* V;
  int M, ns, C;
  float* out;
} pn2_attn_layer;
int pn2_attn_reduce_layers(const pn2_attn_layer* layers, int nlayers, int B,
                           pn2_stream_t stream);
/* Backward of pn2_attn_reduce (TF autodiff of attention_layer.py:35-42): grad_Q (B,M,C),
 * grad_K / grad_V (B,M,ns,C) from grad_out (B,M,C). Every element written (no accumulation);
 * 16-byte aligned buffers, C % 4 == 0. */
int pn2_attn_reduce_grad(const float* Q, const float* K, const float* V, const float* grad_out,
                         int B, int M, int ns, int C, float* grad_Q, float* grad_K,
                         float* grad_V, pn2_stream_t stream);
/* The same reduction for any key_dim (csrc/attn_net.hip): the attention networks build
 * AttentionLayer(out_dim, key_dim=out_dim) with 16 heads, key_dim 8 .. 512 (attention_layer.py
 * :142, :185, pooling_attention_layer.py:17). C = H * key_dim. Head h reads the CONTIGUOUS block
 * [h*ns*kd, (h+1)*ns*kd) of each group's flattened ns*C K / V values as ns rows of kd,
 * s = (K_h q_h) / sqrtf(kd), a = softmax(s), out[h*kd : (h+1)*kd] = aᵀ V_h, fp32 throughout.
 * key_dim % 4 == 0, 4 <= key_dim <= 512, C % key_dim == 0, ns >= 1, every pointer 16-byte
 * aligned: PN2_EINVAL otherwise, before any launch. No groups: PN2_OK. key_dim == 4 IS
 * pn2_attn_reduce / pn2_attn_reduce_grad (the same bits). The backward writes every element of
 * grad_Q (B,M,C) and grad_K / grad_V (B,M,ns,C) exactly once (no atomics: two runs, equal bits).
 * Beyond PN2_ATTN_NET_MAX_BLOCKS blocks of four (group, head) waves the grid strides. */
#define PN2_ATTN_NET_MAX_BLOCKS 4096
int pn2_attn_reduce_kd(const float* Q, const float* K, const float* V, int B, int M, int ns,
                       int C, int key_dim, float* out, pn2_stream_t stream);
int pn2_attn_reduce_kd_grad(const float* Q, const float* K, const float* V,
                            const float* grad_out, int B, int M, int ns, int C, int key_dim,
                            float* grad_Q, float* grad_K, float* grad_V, pn2_stream_t stream);
/* InnerAttentionLayer.call (attention_layer.py:61-78): attention among the heads of ONE point,
 * never across the group. qkv (rows, 3*H*kd) holds [Q | K | V] per row, each H vectors of kd
 * (one GEMM over [Wq | Wk | Wv] writes it). S[i][j] = (Q_i . K_j) / sqrtf(kd), A = softmax over
 * j, out (rows, H*kd) row = [sum_j A[0][j] V_j | .. | sum_j A[H-1][j] V_j]. pn2_head_mix_grad:
 * grad_qkv (rows, 3*H*kd) from grad_out (rows, H*kd), every element written once.
 * 1 <= heads <= PN2_HEAD_MIX_MAX_HEADS, key_dim % 4 == 0, 4 <= key_dim <= 256, 16-byte aligned
 * pointers (PN2_EINVAL otherwise, before any launch); no rows: PN2_OK. 64 / (key_dim / 4 rounded
 * up to a power of two) rows share a wave; beyond PN2_ATTN_NET_MAX_BLOCKS blocks the grid
 * strides. */
#define PN2_HEAD_MIX_MAX_HEADS 8
int pn2_head_mix(const float* qkv, long long rows, int heads, int key_dim, float* out,
                 pn2_stream_t stream);
int pn2_head_mix_grad(const float* qkv, const float* grad_out, long long rows, int heads,
                      int key_dim, float* grad_qkv, pn2_stream_t stream);
/* Per-group pooling over nsample (pointnet_util.py:130-145): x (B,M,ns,C) → out (B,M,C),
 * or (B,M,2C) = [avg, max] for PN2_POOL_MAX_AND_AVG. grouped_xyz (B,M,ns,3) is read only
 * by PN2_POOL_WEIGHTED_AVG (w = exp(-5|xyz|)/sum). */
int pn2_group_pool(const float* x, const float* grouped_xyz, int B, int M, int ns, int C,
                   int mode, float* out, pn2_stream_t stream);

/* ---------------------------------------------------------------- shared MLP ------------ */

/* One 1x1-conv layer of tf_util.conv2d / conv1d in inference mode (tf_util.py:165-185):
 *   y[o] = act(((sum_f x[f] * weight[f][o]) + bias[o]) * bn_scale[o] + bn_shift[o])
 * with bn_scale = gamma / sqrt(moving_var + eps), bn_shift = beta - moving_mean * bn_scale
 * (tf.contrib.layers.batch_norm, is_training=False; tf_util.py:512-531). weight (cin,cout)
 * is TF's [1,1,cin,cout] kernel, row-major. bias, bn_scale, bn_shift (cout) may be NULL
 * (bn_scale and bn_shift together). Packs into `packed` (pn2_mlp_packed_size bytes, 16-byte
 * aligned device memory); stored as scale and (bias*scale + shift). */
size_t pn2_mlp_packed_size(int cin, int cout);
int pn2_mlp_pack(const float* weight, const float* bias, const float* bn_scale,
                 const float* bn_shift, int cin, int cout, void* packed, size_t packed_bytes,
                 pn2_stream_t stream);
/* The same layer for the bf16 matrix cores (v_mfma_f32_32x32x16_bf16), an opt-in: nothing
 * selects it but a caller that packs with this function and sets PN2_MLP_BF16 in the layer's
 * flags. Numerical contract of a layer packed here:
 *   y[o] = act((sum_f bf16(x[f]) * bf16(weight[f][o])) * scale[o] + shift[o])
 * - bf16(.) is round-to-nearest-even from fp32; the weights are rounded once, here, the
 *   activations at the layer's input (the layer before still hands over fp32 values);
 * - the products are exact and the sums accumulate in fp32;
 * - scale = bn_scale, shift = bias * bn_scale + bn_shift, the ReLU, the pooling, the gather and
 *   centring, the IDW interpolation, the attention's query, scores, softmax, weighted sum and
 *   batch norm, and everything written to HBM stay fp32 and unrounded;
 * - a chain may mix bf16 and fp32 layers in any order;
 * - subnormal operands (inputs, weights, and values that round to a bf16 subnormal) are out of
 *   contract: the matrix cores may flush them.
 * Layout: Wp[to][c][h][i][j] = bf16(weight[16c + 8h + j][32to + i]) for output tile to, input
 * chunk c of 16, lane half h, lane i, element j = 0..7 (one 16-byte load per lane per MFMA), cin
 * padded with zeros to a multiple of 16, cout to a multiple of 32; then fp32 scale and shift
 * (32 * ceil(cout/32) each), as in pn2_mlp_pack's layout. pn2_mlp_packed_size_bf16 =
 *   ceil(cout/32) * (ceil(cin/16) * 1024 + 256) bytes.
 * pn2_group_mlp, pn2_fp_mlp, pn2_shared_mlp, pn2_shared_mlp_plan and pn2_group_mlp_attention
 * honour the flag per layer; in pn2_group_mlp_attention qkv[1] and qkv[2] (key, value) may be
 * bf16, qkv[0] (the query, VALU work on the fp32 layout) may not: PN2_EINVAL before any
 * launch.
 *
 * Training in bf16 mode (also an opt-in; the training entry points take no packed layers, the
 * caller packs per step). One tf_util.conv2d layer with is_training=True computes
 *   forward          y[r][o]      = sum_f bf16(x[r][f]) * bf16(W[f][o]) + b[o]
 *                    pn2_mlp_pack_bf16 of W, b (no batch norm, no activation), then
 *                    pn2_shared_mlp with PN2_MLP_BF16: the layer contract above
 *   input gradient   grad_x[r][f] = sum_o bf16(grad_y[r][o]) * bf16(W[f][o])
 *                    the same kernel over a pn2_mlp_pack_bf16 of W^T
 *   weight gradient  grad_w[f][o] = sum_r bf16(x[r][f]) * bf16(grad_y[r][o])
 *                    pn2_mlp_wgrad_bf16
 * - bf16(.) is round-to-nearest-even from fp32, the products are exact, the sums are fp32 on
 *   the matrix cores, and the weight gradient adds its slabs in double as pn2_mlp_wgrad does;
 * - everything else stays fp32 and unrounded: the batch statistics, the activation and its
 *   backward (grad_y, grad_gamma, grad_beta, the bias gradient), the fused max pool and its
 *   arg, the moving averages, Adam and the stored variables;
 * - the variables are fp32 master copies, rounded per step when packed;
 * - the backward treats the rounding as the identity (straight-through);
 * - subnormal operands are out of contract, as above.
 * Without the opt-in the training layers are the fp32 ones, unchanged. */
size_t pn2_mlp_packed_size_bf16(int cin, int cout);
int pn2_mlp_pack_bf16(const float* weight, const float* bias, const float* bn_scale,
                      const float* bn_shift, int cin, int cout, void* packed,
                      size_t packed_bytes, pn2_stream_t stream);

/* pointnet_sa_module after sampling and ball query (pointnet_util.py:106-145, MSG :184-200):
 * group + centre + concat exactly as pn2_group_concat (flags), then `nlayers` packed layers
 * (layers[0].cin = the grouped width; layers[i+1].cin = layers[i].cout), then pooling over the
 * nsample neighbours:
 *   pool = PN2_POOL_MAX / AVG / WEIGHTED_AVG → out (B,M,cout); PN2_POOL_MAX_AND_AVG →
 *   (B,M,2*cout) = [avg, max]; PN2_POOL_NONE → out (B,M,nsample,cout) (the per-point
 *   features the attention SA modules feed to AttentionLayer, attention_layer.py:229-263).
 * Products and sums in fp32 on the matrix cores; the grouped input and the per-layer
 * activations stay on chip. Host array `layers`. `points` rows are gathered with 16-byte
 * loads when C % 4 == 0 and `points` is 16-byte aligned, float by float otherwise (slower,
 * the same bits); xyz, new_xyz, idx and out need 4-byte alignment only. */
int pn2_group_mlp(const float* xyz, const float* points, const float* new_xyz,
                  const int32_t* idx, int B, int N, int C, int M, int nsample, int flags,
                  int nlayers, const pn2_mlp_layer* layers, int pool, float* out,
                  pn2_stream_t stream);
/* pointnet_sa_module_attention (attention_layer.py:229-276) after sampling and ball query:
 * group + MLP as pn2_group_mlp, then — without the per-point features leaving the chip — the
 * AttentionLayer (attention_layer.py:10-45, output_dim = key_dim = 4, heads = C/4):
 * qkv[0..2] = the packed Dense query / key / value layers (C -> C, no activation;
 * pn2_mlp_pack with the Dense kernel and bias), query = the group's first neighbour (:259),
 * head h = the flat block [4*ns*h, 4*ns*(h+1)) of the group's (ns, C) keys and values (the
 * tf.reshape of :35-36), softmax((K_h q_h)/2) V_h; then the inference batch norm
 * out = att * bn_scale + bn_shift (:261; NULL = none) and, with add_max, + the max over nsample
 * of the MLP output (pointnet_sa_module_attention_and_pooling, :296-303). out (B,M,C).
 * nsample <= 128; C = layers[nlayers-1].cout, a multiple of 32. out, bn_scale and
 * bn_shift are accessed in 16-byte units and must be 16-byte aligned (PN2_EINVAL otherwise,
 * before any launch); xyz, points, new_xyz and idx as for pn2_group_mlp (a misaligned `points`
 * takes the per-float gather). */
int pn2_group_mlp_attention(const float* xyz, const float* points, const float* new_xyz,
                            const int32_t* idx, int B, int N, int C, int M, int nsample,
                            int flags, int nlayers, const pn2_mlp_layer* layers,
                            const pn2_mlp_layer* qkv, const float* bn_scale,
                            const float* bn_shift, int add_max, float* out,
                            pn2_stream_t stream);
/* pointnet_fp_module (pointnet_util.py:218-238): IDW weights of dist (B,n,3) + interpolation
 * of points2 (B,m,C2) at nn_idx (B,n,3) + concat [interp, points1 (B,n,C1)] (bit-identical to
 * pn2_fp_apply's output) fed to the packed layers → out (B,n,cout). points1 may be NULL
 * (C1 = 0). dist / nn_idx come from pn2_three_nn or pn2_three_nn_grid. points2 rows are read
 * with 16-byte loads when C2 % 4 == 0 and points2 is 16-byte aligned, points1 rows when
 * C1 % 4 == 0, C2 % 4 == 0 and points1 is 16-byte aligned; any other pointer takes the
 * per-float gather (slower, the same bits). out is stored in 16-byte units when cout % 4 == 0
 * and it is 16-byte aligned, per float otherwise. */
int pn2_fp_mlp(const float* dist, const int32_t* nn_idx, const float* points1, int C1,
               const float* points2, int C2, int B, int n, int m, int nlayers,
               const pn2_mlp_layer* layers, float* out, pn2_stream_t stream);
/* Per-point MLP over rows: x (rows,cin) → out (rows,cout) (tf_util.conv1d with kernel 1,
 * e.g. the fc1/fc2 head of pointnet2_sem_seg.py:57-60). x is read with 16-byte loads when
 * cin % 4 == 0 and x is 16-byte aligned, out stored in 16-byte units when cout % 4 == 0 and
 * out is 16-byte aligned; any other pointer takes the per-float path (slower, the same bits). */
int pn2_shared_mlp(const float* x, long long rows, int cin, int nlayers,
                   const pn2_mlp_layer* layers, float* out, pn2_stream_t stream);
/* R (row tiles per workgroup) and tpw (tiles per workgroup) that pn2_shared_mlp would launch
 * with for these arguments on the current device; launches nothing. The same argument checks
 * as pn2_shared_mlp (apart from the buffers it does not take); both are 0 for rows = 0. */
int pn2_shared_mlp_plan(long long rows, int cin, int nlayers, const pn2_mlp_layer* layers,
                        int* row_tiles, int* tiles_per_wg);
/* One packed layer over rows at any input width: x (rows,cin) → out (rows,cout),
 *   out[r][o] = act((sum_f x[r][f] * W[f][o]) * scale[o] + shift[o]),
 * for the layers whose input row does not fit pn2_shared_mlp's on-chip rows (it refuses from
 * 1,280 channels up): any cin from 1 to 4,194,304, any cout >= 1. `layer` is one fp32 layer
 * packed by pn2_mlp_pack, the pack that pn2_shared_mlp reads, unchanged; layer->cin must equal
 * cin. A layer flagged PN2_MLP_BF16 is refused (fp32 only). The kernel streams K through the
 * chip in slabs and keeps each 32 x 32 output tile's sum in registers (csrc/mlp_wide.hip).
 * - Summation order: up to 1,248 input channels (every width pn2_shared_mlp takes) an output is
 *   one fp32 chain on the matrix cores over the chunks of 8 channels in ascending order, the
 *   chunk's channels in pn2_shared_mlp's order, and the result is pn2_shared_mlp's, bit for
 *   bit. A wider row is cut into segments of 512 channels: one such chain per segment, the
 *   segments' sums added in ascending order (a single chain of thousands of additions would
 *   round worse than the project's tests allow). No sum is split over waves or workgroups and
 *   nothing is added with atomics: two runs give equal bits, and the bits depend on cin, never
 *   on rows or the launch shape.
 * - Alignment: x is read with 16-byte loads when cin % 4 == 0 and x is 16-byte aligned, out is
 *   stored in 16-byte units when cout % 4 == 0 and out is 16-byte aligned; any other pointer
 *   takes the per-float path (slower, the same bits). layer->packed must be 16-byte aligned.
 * - Limits: 0 <= rows <= 2^31 - 1 (rows = 0: PN2_OK, nothing launched); row offsets into x and
 *   out are 64-bit, so rows * cin and rows * cout may pass 2^31. Grid x = ceil(rows / (32 *
 *   row_tiles)) row blocks, grid y = ceil(ceil(cout / 32) / out_tiles_per_wg) <= 65,535.
 * Null x, out (with rows > 0), layer or layer->packed, cin <= 0 or above 4,194,304,
 * layer->cout <= 0, rows < 0, a misaligned pack and a bf16 layer return PN2_EINVAL before any
 * launch. */
int pn2_dense_wide(const float* x, long long rows, int cin, const pn2_mlp_layer* layer,
                   float* out, pn2_stream_t stream);
/* The launch shape pn2_dense_wide would use for these arguments; launches nothing and needs no
 * device. row_tiles: tiles of 32 rows per workgroup; k_slab: input channels per slab (a
 * multiple of 8); out_tiles_per_wg: tiles of 32 output columns per workgroup. A workgroup's LDS
 * is 2 * 32 * row_tiles * (k_slab + 4) * 4 bytes. The same argument checks as pn2_dense_wide
 * (apart from the buffers it does not take); all three are 0 for rows = 0. */
int pn2_dense_wide_plan(long long rows, int cin, const pn2_mlp_layer* layer, int* row_tiles,
                        int* k_slab, int* out_tiles_per_wg);

/* ---------------------------------------------------------------- shared MLP, training -- */
/* One tf_util.conv2d / conv1d layer with is_training=True (tf_util.py:165-185, batch norm on
 * batch statistics :512-531): y = x W + b (pn2_shared_mlp over a pn2_mlp_pack of W and b with
 * no batch norm and no activation), then the entry points below. All tensors row-major fp32.
 * Every reduction is two-stage with a fixed order and no floating-point atomics, so results
 * are bitwise reproducible. */

/* Per-channel mean and BIASED variance of y (rows,C) over the rows. Stage 1: each workgroup
 * reduces PN2_BN_BLOCK_ROWS rows of 32 channels to (mean, M2) partials (8-row batches merged
 * with Chan's formula); stage 2 merges the partials in double precision. workspace:
 * pn2_bn_workspace_size(rows, C) bytes of device memory (also enough for pn2_bn_act_bwd). */
#define PN2_BN_BLOCK_ROWS 1024
size_t pn2_bn_workspace_size(long long rows, int C);
int pn2_bn_stats(const float* y, long long rows, int C, float* mean, float* var, void* workspace,
                 size_t workspace_bytes, pn2_stream_t stream);
/* out = act((y - mean) * (gamma / sqrt(var + eps)) + beta), act = ReLU when `relu`, else the
 * identity. mean, var, gamma and beta may be NULL together: no batch norm, out = act(y). */
int pn2_bn_act_fwd(const float* y, long long rows, int C, const float* mean, const float* var,
                   const float* gamma, const float* beta, float eps, int relu, float* out,
                   pn2_stream_t stream);
/* Backward of pn2_bn_act_fwd. dz = grad_out * [pre-activation > 0] (the pre-activation is
 * recomputed from y with the forward's fp32 expression, so the mask equals out > 0);
 * grad_beta = sum dz, grad_gamma = sum dz * xhat, xhat = (y - mean) / sqrt(var + eps);
 * grad_y = gamma / sqrt(var + eps) * (dz - grad_beta / rows - xhat * grad_gamma / rows).
 * Without batch norm (mean, var, gamma, beta and grad_gamma NULL): grad_y = dz and grad_beta
 * = sum dz (the bias gradient). workspace: pn2_bn_workspace_size(rows, C) bytes. */
int pn2_bn_act_bwd(const float* grad_out, const float* y, long long rows, int C,
                   const float* mean, const float* var, const float* gamma, const float* beta,
                   float eps, int relu, float* grad_y, float* grad_gamma, float* grad_beta,
                   void* workspace, size_t workspace_bytes, pn2_stream_t stream);
/* pn2_bn_act_fwd fused with the max pool over the ns samples of a group, for the last MLP
 * layer of a set-abstraction module: y is (groups,ns,C), out[g][c] = max_j act(bn(y[g][j][c]))
 * (groups,C), bit for bit pn2_bn_act_fwd followed by a max over j, without the (groups,ns,C)
 * activation being written. The max is over the activation, not over y (gamma may be
 * negative). arg[g][c] (int32, (groups,C)) is the LOWEST j that attains it: 0 for a group whose
 * activations are all equal (a dead ReLU channel), and never one of the rows a ball query pads
 * with copies of its first neighbour. groups * ns <= 2^31 - 1. NaN inputs are unsupported. */
int pn2_bn_act_pool_fwd(const float* y, long long groups, int ns, int C, const float* mean,
                        const float* var, const float* gamma, const float* beta, float eps,
                        int relu, float* out, int* arg, pn2_stream_t stream);
/* Backward of pn2_bn_act_pool_fwd from grad_out (groups,C): dz[g][j][c] = grad_out[g][c] where
 * j == arg[g][c] and (no ReLU or the recomputed pre-activation > 0), else 0 (an arg outside
 * [0, ns) selects nothing); then pn2_bn_act_bwd's formulas with rows = groups * ns, written to
 * every element of grad_y (groups,ns,C). The sums read one y element per (group, channel):
 * stage 1 writes one partial per PN2_BN_POOL_BLOCK_GROUPS groups, stage 2 adds them in double
 * precision in a fixed order. Without batch norm (mean, var, gamma, beta, grad_gamma NULL):
 * grad_y = dz, grad_beta = sum dz. workspace: pn2_bn_pool_workspace_size(groups, C) bytes. */
#define PN2_BN_POOL_BLOCK_GROUPS 128
size_t pn2_bn_pool_workspace_size(long long groups, int C);
int pn2_bn_act_pool_bwd(const float* grad_out, const int* arg, const float* y, long long groups,
                        int ns, int C, const float* mean, const float* var, const float* gamma,
                        const float* beta, float eps, int relu, float* grad_y, float* grad_gamma,
                        float* grad_beta, void* workspace, size_t workspace_bytes,
                        pn2_stream_t stream);
/* grad_w (cin,cout) = x^T grad_y for x (rows,cin), grad_y (rows,cout), on the fp32 matrix
 * cores. Rows are cut into slabs of PN2_WGRAD_SLAB_ROWS; a slab's 32x32 tile product is
 * accumulated in fp32 from zero, slab results are added in double precision and written as at
 * most PN2_WGRAD_MAX_PARTS partial tiles per output tile (fewer when that would exceed
 * PN2_WGRAD_MAX_WS_BYTES of workspace), and stage 2 sums the partials in double precision.
 * workspace: pn2_mlp_wgrad_workspace_size(rows, cin, cout) bytes. */
#define PN2_WGRAD_SLAB_ROWS 1024
#define PN2_WGRAD_MAX_PARTS 512
#define PN2_WGRAD_MAX_WS_BYTES (64u << 20)
size_t pn2_mlp_wgrad_workspace_size(long long rows, int cin, int cout);
int pn2_mlp_wgrad(const float* x, const float* grad_y, long long rows, int cin, int cout,
                  float* grad_w, void* workspace, size_t workspace_bytes, pn2_stream_t stream);
/* The weight gradient of a training layer in bf16 mode (the contract is at pn2_mlp_pack_bf16):
 *   grad_w[f][o] = sum_r bf16(x[r][f]) * bf16(grad_y[r][o])
 * on v_mfma_f32_32x32x16_bf16: x and grad_y are read as fp32, straight from the row-major
 * tensors, and rounded on the way into the matrix cores (one MFMA covers 16 rows). Arguments,
 * checks, slabs, parts, workspace (pn2_mlp_wgrad_workspace_size) and stage 2 are pn2_mlp_wgrad's:
 * a slab's tile is four fp32 chains of 16 MFMAs from zero, added in wave order, slabs and parts
 * in double. No atomics: two runs give equal bits. */
int pn2_mlp_wgrad_bf16(const float* x, const float* grad_y, long long rows, int cin, int cout,
                       float* grad_w, void* workspace, size_t workspace_bytes,
                       pn2_stream_t stream);

/* ---------------------------------------------------------------- attention, training --- */
/* The AttentionLayer of the attention SA modules (attention_layer.py:10-45, :256-259) with
 * is_training=True: K and V are projected together, KV = X [Wk | Wv] + [bk | bv] (one
 * pn2_shared_mlp over a pn2_mlp_pack of the (C, 2C) matrix), so KV (G,ns,2C) holds in row j of
 * group g the K row followed by the V row, and X is read once. */

/* pn2_attn_reduce on that layout: Q (G,C), KV (G,ns,2C) -> out (G,C). Pseudo-key i of head h is
 * the 4 floats at flat index f = 4*ns*h + 4*i of the group's row-major (ns,C) K matrix (the
 * tf.reshape reinterpretation), i.e. KV[g][f / C][f % C .. +3]; its value vector is
 * KV[g][f / C][C + f % C .. +3]. The result has the bits of pn2_attn_reduce on de-interleaved
 * copies. 16-byte aligned buffers, C % 4 == 0, ns > 0, ns * C < 2^30; G = 0 is a no-op. */
int pn2_attn_kv_reduce(const float* Q, const float* KV, long long G, int ns, int C, float* out,
                       pn2_stream_t stream);
/* Its backward (the formulas of pn2_attn_reduce_grad): grad_Q (G,C) and grad_KV (G,ns,2C), in
 * KV's layout, from grad_out (G,C). Every element written, no accumulation; K and V are read
 * once, and every reduction has a fixed order (two runs give equal bits; they are not the
 * bits of pn2_attn_reduce_grad, whose reduction order differs). */
int pn2_attn_kv_reduce_grad(const float* Q, const float* KV, const float* grad_out, long long G,
                            int ns, int C, float* grad_Q, float* grad_KV, pn2_stream_t stream);
/* In place on grad_x (G,ns,C): grad_x[g][0][c] += grad_xq[g][c] (the query is the group's
 * first row, attention_layer.py:259); then, where grad_pmax is given and 0 <= arg[g][c] < ns,
 * grad_x[g][arg[g][c]][c] += grad_pmax[g][c] (the max pool of the _and_pooling module, :303).
 * One thread per (g, c) does both adds in that order: no atomics, deterministic. An arg
 * outside [0, ns) selects nothing and is never dereferenced. grad_pmax and arg (int32, (G,C))
 * are NULL together. */
int pn2_attn_dx_scatter(float* grad_x, const float* grad_xq, const float* grad_pmax,
                        const int* arg, long long G, int ns, int C, pn2_stream_t stream);
/* out[c] = sum over the rows of x (rows,C): the bias gradients. Two-stage like pn2_bn_act_bwd's
 * sums: fp32 partials over PN2_BN_BLOCK_ROWS rows, then double precision in a fixed order.
 * workspace: pn2_col_sum_workspace_size(rows, C) bytes. */
size_t pn2_col_sum_workspace_size(long long rows, int C);
int pn2_col_sum(const float* x, long long rows, int C, float* out, void* workspace,
                size_t workspace_bytes, pn2_stream_t stream);

/* ---------------------------------------------------------------- segmentation head, training */
/* The last three operations of a pointnet2_sem_seg training step (pointnet2_sem_seg.py:56,
 * :62-69): the dropout between fc1 and fc2 and get_loss. csrc/head_train.hip. */

/* tf_util.dropout with is_training (tf_util.py:594-612; TF 1.x: div(x, keep_prob) * mask):
 *   out[e] = keep(e) ? x[e] / keep_prob : 0      (one correctly rounded fp32 division)
 * over n floats. keep(e) is Philox4x32-10 (csrc/philox.h): key = (seed & 0xffffffff,
 * seed >> 32), counter = (q & 0xffffffff, q >> 32, 0, 0) with q = e / 4; element e takes output
 * word e % 4 and is kept iff word < floor(keep_prob * 2^32) (computed on the host in double).
 * The mask is a pure function of (seed, e): nothing is saved, the backward is the same call on
 * the gradient with the same seed, and the result does not depend on the launch shape. It is
 * not TensorFlow's generator. keep_prob must lie in (0, 1] (1 copies); n = 0
 * returns 0 without a launch; out == x is allowed. Pointers that are not 16-byte aligned take a
 * scalar path. */
int pn2_dropout(const float* x, long long n, float keep_prob, uint64_t seed, float* out,
                pn2_stream_t stream);
/* The same function on HOST pointers in plain C++, synchronous: the GPU result equals it bit
 * for bit. */
int pn2cpu_dropout(const float* x, long long n, float keep_prob, uint64_t seed, float* out);

/* tf.losses.sparse_softmax_cross_entropy(labels, logits, weights) with its default reduction
 * SUM_BY_NONZERO_WEIGHTS. logits (rows,C) fp32, labels (rows) int32, weights (rows) fp32 or
 * NULL for all ones. One read of the logits. Per row: lse = m + log sum exp(z - m), m = max z,
 * (saved for the backward), pred = the argmax with the lowest index on ties (may be NULL), ce =
 * lse - z[label]. Two scalars in device memory: num_present = the rows with w != 0, loss = sum
 * w * ce / num_present, or 0 when num_present = 0. The sum is two-stage: one fp32 partial per
 * PN2_XENT_BLOCK_ROWS rows, added in double in a fixed order; no atomics, two runs give equal
 * bits. A label outside [0, C) is never dereferenced: that row's ce is NaN (TF's GPU kernel).
 * NaN logits are unsupported. 0 < rows < 2^31, 0 < C <= 65535. workspace:
 * pn2_softmax_xent_workspace_size(rows) bytes. */
#define PN2_XENT_BLOCK_ROWS 128
size_t pn2_softmax_xent_workspace_size(long long rows);
int pn2_softmax_xent_fwd(const float* logits, const int32_t* labels, const float* weights,
                         long long rows, int C, float* lse, int32_t* pred, float* loss,
                         int32_t* num_present, void* workspace, size_t workspace_bytes,
                         pn2_stream_t stream);
/* Its backward, one read of the logits and one write: grad_logits[i][c] = g * w_i /
 * num_present * (exp(z_ic - lse_i) - [c == label_i]), g = *grad_loss. g and num_present are
 * read from device memory (nothing synchronises); num_present = 0 writes every element as 0.
 * The weights get no gradient (the reference feeds them from a placeholder). */
int pn2_softmax_xent_bwd(const float* grad_loss, const float* logits, const int32_t* labels,
                         const float* weights, const float* lse, const int32_t* num_present,
                         long long rows, int C, float* grad_logits, pn2_stream_t stream);

/* ---------------------------------------------------------------- optimiser and metrics ---- */
/* What the reference's training loop (attention_points/train.py:288-387) runs once the
 * gradients exist: tf.train.AdamOptimizer and get_metrics. csrc/optim.hip, with host twins in
 * csrc/cpu_optim.cpp. */

/* One variable of an Adam step: the parameter p, its gradient g and the two slot variables
 * m (<var>/Adam) and v (<var>/Adam_1), n floats each. */
typedef struct {
  float* p;
  const float* g;
  float* m;
  float* v;
  long long n;
} pn2_adam_slot;
#define PN2_ADAM_SLOTS 64   /* slots per launch: the by-value argument block stays <= 4096 bytes */
#define PN2_ADAM_CHUNK 2048 /* elements one workgroup updates                                    */
#define PN2_ADAM_MAX_N (1LL << 35) /* largest n of one slot                                      */

/* TF 1.x ApplyAdam without Nesterov (training_ops.cc), over `nslots` variables. Per element, in
 * fp32, every operation rounded on its own (no contraction), in this order:
 *   omb1 = 1 - beta1;  omb2 = 1 - beta2
 *   m' = m + (g - m) * omb1
 *   v' = v + (g * g - v) * omb2
 *   p' = p - (alpha * m') / (sqrt(v') + epsilon)
 * The caller folds both bias corrections into the step size, alpha = lr * sqrt(1 - beta2^t) /
 * (1 - beta1^t), so epsilon is added to the uncorrected sqrt(v') (TF's "epsilon hat"; not
 * torch.optim.Adam's arithmetic). The division and the square root are correctly rounded and
 * denormals are kept, so the device result equals the host twin bit for bit and does not depend
 * on the launch shape.
 * `slots` is a HOST array of device pointers. It travels by value in the kernel arguments,
 * PN2_ADAM_SLOTS slots per launch: a step is ceil(nslots / PN2_ADAM_SLOTS) launches, with no
 * device-side table, no allocation, no copy and no synchronisation. A workgroup updates one
 * PN2_ADAM_CHUNK-element chunk of one slot, with 16-byte loads and stores when the slot's four
 * pointers are 16-byte aligned and a scalar path when one is not. Slots must not overlap. n = 0
 * slots are skipped (their pointers may be NULL); nslots = 0 returns 0 without a launch.
 * PN2_EINVAL, checked before any launch: slots NULL with nslots > 0, nslots < 0, a NULL pointer
 * in a slot with n > 0, n < 0 or n > PN2_ADAM_MAX_N, beta1 or beta2 outside [0, 1), epsilon < 0
 * (or NaN), a non-finite alpha. */
int pn2_adam_step(const pn2_adam_slot* slots, int nslots, float alpha, float beta1, float beta2,
                  float epsilon, pn2_stream_t stream);
/* The same function on HOST pointers in plain C++, synchronous: the GPU result equals it bit
 * for bit. */
int pn2cpu_adam_step(const pn2_adam_slot* slots, int nslots, float alpha, float beta1,
                     float beta2, float epsilon);

/* get_metrics (attention_points/train.py:145-163): labels and pred (rows) int32, pred the
 * argmax that pn2_softmax_xent_fwd returns. For every row with 0 < label < C and 0 <= pred < C:
 *   confusion[label][pred] += 1      (C,C) int64, the total of tf.metrics.mean_iou
 *   counts[1] += 1                   the assigned points
 *   counts[0] += (pred == label)     the correct ones: accuracy = counts[0] / counts[1]
 * Other rows are ignored: label 0 is "unannotated", and a value out of range is never used as
 * an index. Both outputs are ADDED to (the caller zeroes them). Each workgroup counts
 * PN2_CONFUSION_BLOCK_ROWS rows into a C x C histogram of 32-bit counters in LDS and adds its
 * non-zero cells with 64-bit integer atomic adds: integer adds commute, two runs give equal
 * bits. 0 < C <= PN2_METRICS_MAX_C, 0 <= rows (below 2^31 workgroups' worth); rows = 0 returns
 * 0 without a launch. */
#define PN2_METRICS_MAX_C 64
#define PN2_CONFUSION_BLOCK_ROWS 2048
int pn2_seg_confusion(const int32_t* labels, const int32_t* pred, long long rows, int C,
                      long long* confusion, long long* counts, pn2_stream_t stream);
/* tf.metrics.mean_iou's value of a (C,C) confusion matrix, one small launch: per class c, den =
 * row_sum[c] + col_sum[c] - cm[c][c]; classes with den = 0 are left out; iou_c = cm[c][c] / den
 * in double; *iou = the double sum in class order over the number of classes with den > 0,
 * rounded to fp32, or 0 when there is none; per_class[c] (C floats, may be NULL) = iou_c as
 * fp32, 0 where den = 0. TensorFlow divides in fp32, so its last bit can differ. */
int pn2_mean_iou(const long long* confusion, int C, float* iou, float* per_class,
                 pn2_stream_t stream);
/* The same two functions on HOST pointers in plain C++, synchronous: equal integers, equal
 * fp32 bits. */
int pn2cpu_seg_confusion(const int32_t* labels, const int32_t* pred, long long rows, int C,
                         long long* confusion, long long* counts);
int pn2cpu_mean_iou(const long long* confusion, int C, float* iou, float* per_class);

/* ---------------------------------------------------------------- scene crops ---------- */

/* Scene bounding box: bbox = [min x, min y, min z, max x, max y, max z] of points (N,3)
 * (reduce_min / reduce_max, data_transformation.py:90-91). workspace:
 * pn2_scene_workspace_size(N) bytes of device memory. */
size_t pn2_scene_workspace_size(int N);
int pn2_scene_bbox(const float* points, int N, float* bbox, void* workspace,
                   size_t workspace_bytes, pn2_stream_t stream);
/* get_subset (data_transformation.py:70-154) for B crops of one scene, with the reference's
 * random draws supplied by the caller: centres (B,T) = the point index each try is centred on
 * (:95-97, T = 10 in the reference), u (B,K) = the uniform [0,1) draws of the final choice
 * (:146). Try t's area: x, y within the centre -+ 0.75, z over the scene (:98-103); points
 * inside it +0.2 (>= lo, < hi) in index order; valid if labelled / (3 n) >= 0.7 (the
 * reference divides by reduce_sum(ones_like((n,3) points)), :113) and the occupied voxel keys
 * / 31 / 31 / 62 >= 0.02 (:119-126); the first valid try is kept, else the last (:138-141).
 * With the 3 n denominator no try can be valid (labelled / 3n <= 1/3), so the last try is
 * used without evaluating the others; the earlier centres only mirror the reference's draws.
 * Outputs (B,K[,3]): points, labels, colors (int32, may be NULL with out_colors NULL),
 * normals (may be NULL likewise), weights = label_weights[label] * mask, mask = inside the
 * area +0.01 (:114-117, :150-153). bbox from pn2_scene_bbox. workspace:
 * pn2_crop_workspace_size(B, N, T) bytes. */
size_t pn2_crop_workspace_size(int B, int N, int T);
int pn2_crop_sample(const float* points, const int32_t* labels, const int32_t* colors,
                    const float* normals, int N, const float* bbox, const int32_t* centres,
                    int B, int T, const float* u, int K, const float* label_weights, int nlw,
                    void* workspace, size_t workspace_bytes, float* out_points,
                    int32_t* out_labels, int32_t* out_colors, float* out_normals,
                    float* out_weights, pn2_stream_t stream);
/* Whole-scene chunker, selection part (complete_scene_loader.py:33-40): for each of S boxes
 * bounds (S,6) = [lo xyz, hi xyz] in FLOAT64 (the reference's float32 points compare against
 * float64 bounds), the indices of the points with lo - margin <= p <= hi + margin on all axes,
 * ascending, in sel[s*N ...], inner[s*N + k] = 1 if that point is also within [lo, hi], and the
 * per-slice counts in counts (S, pn2_subvolume_slices(N)) — their row sums are the subvolume
 * sizes. The random shuffle / fill-up of the chunks is drawn by the caller. */
int pn2_subvolume_slices(int N);
int pn2_subvolume_select(const float* points, int N, const double* bounds, int S, double margin,
                         int32_t* counts, int32_t* sel, uint8_t* inner, pn2_stream_t stream);
/* dst[r] = src[idx[r]] for n rows of row_bytes bytes (a multiple of 4); idx outside
 * [0, nsrc) reads row 0. */
int pn2_gather_rows(const void* src, long long nsrc, int row_bytes, const int32_t* idx,
                    long long n, void* dst, pn2_stream_t stream);

/* ---------------------------------------------------------------- scene prediction ----- */

/* What the reference does with a trained model (attention_points/benchmark/
 * generate_predictions.py:139-186): the argmax of every chunk row's logits and map_back
 * (:19-37), res = zeros(res_shape); res[orig[mask]] = values[mask], over a scene's
 * concatenated chunks. numpy writes repeated indices in order, so of the masked rows that name
 * one point the last row in concatenation order wins. csrc/predict.hip, with host twins in
 * csrc/cpu_predict.cpp.
 *
 * Every scene point holds one 64-bit key, ((global_row + 1) << PN2_VOTE_LABEL_BITS) | label,
 * 0 = never written, and a voting row applies an unsigned 64-bit atomic max to its point's
 * key. The largest global row wins, numpy's order; an integer max commutes, so the keys are the
 * same bits for any launch order, any stream and any split of the scene into batches. */
#define PN2_VOTE_LABEL_BITS 8

/* One batch of chunk rows votes. logits (rows, C) fp32 or NULL (the label is 0 and C is
 * ignored: the vote then only records which row wins, for pn2_map_back_rows); mask (rows)
 * uint8, orig (rows) int32: the chunker's `mask` and `points_orig_idxs`; row0: the global index
 * of the batch's first row; keys (n_scene) as above, zeroed by the caller once per scene;
 * pred_rows (rows) int32 or NULL: every row's argmax, voting or not. The argmax takes the lowest
 * index of a tie (np.argmax); NaN logits are unsupported. Row r votes iff mask[r] != 0 and
 * 0 <= orig[r] < n_scene; no other row indexes keys (the reference raises IndexError for an
 * index past the scene and wraps a negative one).
 * PN2_EINVAL, checked before any launch: C outside [1, 1 << PN2_VOTE_LABEL_BITS] when logits
 * are given, rows < 0, row0 < 0, row0 + rows >= 2^55 (the key's 56 row bits), n_scene outside
 * [0, 2^31), a NULL mask, orig or keys. rows = 0 returns 0 without a launch. */
int pn2_scene_vote(const float* logits, long long rows, int C, const uint8_t* mask,
                   const int32_t* orig, long long row0, long long n_scene, long long* keys,
                   int32_t* pred_rows, pn2_stream_t stream);
/* The keys resolved, each output (n_scene) and optional (NULL):
 *   labels[p] = key ? key & 255 : 0             int32: the remapped prediction, 0 where unwritten
 *   winner[p] = key ? (key >> 8) - 1 : -1       int64: the global row that wrote point p
 *   mapped[p] = 0 <= labels[p] < nlut ? lut[labels[p]] : dflt   (needs lut: map_to_nyu40 in the
 *               same pass) */
int pn2_scene_labels(const long long* keys, long long n_scene, const int32_t* lut, int nlut,
                     int32_t dflt, int32_t* labels, int32_t* mapped, long long* winner,
                     pn2_stream_t stream);
/* map_back of any per-row values: values (rows, row_bytes) are the rows [row0, row0 + rows) of
 * the scene's concatenated chunks, out (n_scene, row_bytes). Per point p with winner w:
 *   key 0                      out[p] = zero bytes
 *   row0 <= w < row0 + rows    out[p] = values[w - row0]
 *   otherwise                  out[p] stays as it is,
 * so a caller that keeps one batch at a time resolves batch by batch into one `out`. row_bytes
 * is a multiple of 4, as in pn2_gather_rows; the row0 / rows / n_scene bounds are
 * pn2_scene_vote's. */
int pn2_map_back_rows(const void* values, int row_bytes, long long row0, long long rows,
                      const long long* keys, long long n_scene, void* out, pn2_stream_t stream);
/* out[i] = 0 <= in[i] < nlut ? lut[in[i]] : dflt over n int32 labels; in == out is allowed. One
 * kernel for generate_predictions.py's map_to_nyu40 (dict.get(label, 1): dflt = 1),
 * data_transformation.py's label_map (a 41-entry table, dflt = 0: the reference's
 * min(label, 40) look-up for every non-negative label) and evaluate.py's two tests against
 * VALID_CLASS_IDS (ground truth not valid -> 0, prediction not valid -> 40). A negative label
 * gives dflt, where the reference's gather wraps around or raises. */
int pn2_label_lut(const int32_t* in, long long n, const int32_t* lut, int nlut, int32_t dflt,
                  int32_t* out, pn2_stream_t stream);
/* The same four functions on HOST pointers in plain C++, synchronous: equal bits. */
int pn2cpu_scene_vote(const float* logits, long long rows, int C, const uint8_t* mask,
                      const int32_t* orig, long long row0, long long n_scene, long long* keys,
                      int32_t* pred_rows);
int pn2cpu_scene_labels(const long long* keys, long long n_scene, const int32_t* lut, int nlut,
                        int32_t dflt, int32_t* labels, int32_t* mapped, long long* winner);
int pn2cpu_map_back_rows(const void* values, int row_bytes, long long row0, long long rows,
                         const long long* keys, long long n_scene, void* out);
int pn2cpu_label_lut(const int32_t* in, long long n, const int32_t* lut, int nlut, int32_t dflt,
                     int32_t* out);

/* ---------------------------------------------------------------- training feed -------- */

/* What stands between a stored crop and the training step (attention_points/train.py:74-109,
 * scannet_dataset/data_transformation.py:270-352). csrc/feed.hip and csrc/scene.hip, with host
 * twins in csrc/cpu_feed.cpp.
 *
 * get_data_tensors (train.py:94-108) and random_rotate (data_transformation.py:334-352) of a
 * whole batch in one launch. Inputs: points (B,N,3), labels (B,N), colors (B,N,3) int32 or NULL,
 * normals (B,N,3) or NULL, sample_weight (B,N) as stored, cs (B,2) = each cloud's (cos, sin) or
 * NULL, class_weights (L). Outputs: xyz (B,N,3), features (B,N,F) with F = 3 use_color +
 * 3 use_normal, colours first (NULL when F = 0), smpw (B,N).
 *   rotation   x' = x c + y s, y' = y c - x s, z' = z: each product rounded, then the sum (the
 *              row vector times [[c,-s,0],[s,c,0],[0,0,1]]); the points, and the normals when
 *              use_normal. cs NULL: nothing is rotated, the coordinates are copied.
 *   colour     (float)c / 255.0f, a correctly rounded fp32 division
 *   smpw       (0 <= label < L ? class_weights[label] : 0) * (sample_weight != 0 ? 1 : 0):
 *              -0.0 gives mask 0 and NaN mask 1, as tf.not_equal does
 * Every access is one 4-byte element: any 4-byte aligned pointer is taken and the bits do not
 * depend on it. PN2_EINVAL before any launch: B, N or L negative, a NULL points, labels,
 * sample_weight, xyz or smpw, use_color without colors, use_normal without normals, F > 0
 * without features, L > 0 without class_weights. B * N = 0 is a no-op. */
int pn2_feed_batch(const float* points, const int32_t* labels, const int32_t* colors,
                   const float* normals, const float* sample_weight, const float* cs,
                   const float* class_weights, int L, int B, int N, int use_color,
                   int use_normal, float* xyz, float* features, float* smpw,
                   pn2_stream_t stream);
/* The validation chunker get_all_subsets_for_scene_numpy (data_transformation.py:270-331),
 * selection part: pn2_subvolume_select's kernels with the inner test's margin as a parameter
 * (the reference masks with curmin - 0.001 .. curmax + 0.001 in float64, :309) and one count per
 * column: counts (S), sel (S,N), inner (S,N). workspace: pn2_val_select_workspace_size(N, S)
 * bytes. PN2_EINVAL: N or S negative, S * N > 2^31 - 1, S > 65535, a NULL buffer, a workspace
 * too small. S = 0 is a no-op; N = 0 zeroes counts. */
size_t pn2_val_select_workspace_size(int N, int S);
int pn2_val_select(const float* points, int N, const double* bounds, int S, double margin,
                   double inner_margin, void* workspace, size_t workspace_bytes, int32_t* counts,
                   int32_t* sel, uint8_t* inner, pn2_stream_t stream);
/* The validation chunker, draw and gather part (:311-325). For each column s with
 * n = counts[s] > 0, draw r is choice[s*K + r] when choice (S,K) is given (clamped to
 * [0, n - 1]; the caller's np.random.choice), else min(max((int)(u[s*K + r] * (float)n), 0),
 * n - 1) (pn2_crop_sample's rule); point, label, colour and normal are gathered through sel,
 * mask = inner, weight = (0 <= label < L ? label_weights[label] : 0) * mask. The chunk is kept
 * unless (double)sum(mask) / (double)K < min_inside (:317, 0.01). Kept chunks are written
 * compacted in column order into the outputs, which hold S chunks: out_points (S,K,3),
 * out_labels (S,K), out_colors (S,K,3) (with colors, else NULL), out_normals likewise,
 * out_weights (S,K); column (S) = the column of each kept chunk, -1 past them; kept (1) = their
 * number. The chunks past `kept` are zeroed. Mask sums are integer adds and the slots come from
 * one scan over the columns, so the outputs are the same bits in every run. workspace:
 * pn2_val_chunks_workspace_size(S) bytes. PN2_EINVAL: N, S, K or L negative, S * N or S * K
 * > 2^31 - 1, S > 65535, kept NULL, a NULL buffer that is needed, neither choice nor u with
 * K > 0, a workspace too small. */
size_t pn2_val_chunks_workspace_size(int S);
int pn2_val_chunks(const float* points, const int32_t* labels, const int32_t* colors,
                   const float* normals, int N, const int32_t* counts, const int32_t* sel,
                   const uint8_t* inner, int S, const int32_t* choice, const float* u, int K,
                   const float* label_weights, int L, double min_inside, void* workspace,
                   size_t workspace_bytes, float* out_points, int32_t* out_labels,
                   int32_t* out_colors, float* out_normals, float* out_weights, int32_t* column,
                   int32_t* kept, pn2_stream_t stream);
/* The same three functions on HOST pointers in plain C++, synchronous, without workspace:
 * equal bits. */
int pn2cpu_feed_batch(const float* points, const int32_t* labels, const int32_t* colors,
                      const float* normals, const float* sample_weight, const float* cs,
                      const float* class_weights, int L, int B, int N, int use_color,
                      int use_normal, float* xyz, float* features, float* smpw);
int pn2cpu_val_select(const float* points, int N, const double* bounds, int S, double margin,
                      double inner_margin, int32_t* counts, int32_t* sel, uint8_t* inner);
int pn2cpu_val_chunks(const float* points, const int32_t* labels, const int32_t* colors,
                      const float* normals, int N, const int32_t* counts, const int32_t* sel,
                      const uint8_t* inner, int S, const int32_t* choice, const float* u, int K,
                      const float* label_weights, int L, double min_inside, float* out_points,
                      int32_t* out_labels, int32_t* out_colors, float* out_normals,
                      float* out_weights, int32_t* column, int32_t* kept);

/* ---------------------------------------------------------------- scene rendering ------ */

/* The reference's ball renderer, headless (pointnet2_tensorflow/utils/render_balls_so.cpp
 * render_ball and the projection of show3d_balls.py:52-74). csrc/render.hip, with host twins in
 * csrc/cpu_render.cpp; both run the arithmetic of csrc/render_math.h.
 *
 * render_ball is a serial loop over points x disk entries in which a pixel keeps the first point
 * that reaches the greatest depth. Here every pixel holds one 64-bit key,
 *     ((z2 + 2^31) << 32) | (0xFFFFFFFF - i),      0 = nothing drawn,
 * and every (point, disk entry) pair applies an unsigned 64-bit atomic max; a second pass shades
 * the winners. Tie rule: the greatest z2 wins and among equal z2 the lowest point index, the
 * serial loop's strict `depth < z2`. An integer max commutes: the image is a pure function of the
 * inputs, the same bits in every run. No float atomics.
 *
 * pn2_render_ball renders F frames in one call. ixyz (F,n,3) int32: each frame's x (row), y
 * (column), z (depth). Colours: c0, c1, c2 (n) fp32 shared by the frames, or, with labels (n)
 * int32 not NULL, palette (npal,3) fp32 whose row labels[i] is (c0, c1, c2) of point i (a label
 * outside [0, npal) reads row 0; the look-up runs once per pixel). images (F,h,w,3) uint8.
 *   radius     r = max(r, 1). The disk's entries are the (dx, dy) with dx*dx + dy*dy < r*r;
 *              dz = sqrt(double(r*r - dx*dx - dy*dy)), depth offset int(dz), shade
 *              float(dz / r).
 *   reach      entry (dx, dy) of point i reaches pixel (x + dx, y + dy) with z2 = z + int(dz) if
 *              the pixel lies in the image and z2 > -2100000000. A point may lie partly or
 *              wholly outside.
 *   depth cue  zmin = min(z) - r and zmax = max(z) + r over all n points of the frame, those
 *              outside the image too; intensity = min(1.0, (z2 - zmin) / (zmax - zmin) * 0.7 +
 *              0.3) in double.
 *   pixel      (shade * c2[i] * intensity, shade * c0[i] * intensity, shade * c1[i] *
 *              intensity), the reference's channel order: a float product, then a double
 *              product, then truncation to uint8. Colours are expected in [0, 255] and are
 *              clamped into it first (NaN: 0), because the reference's conversion is undefined
 *              outside. A pixel nothing reaches is (bg0, bg1, bg2).
 * Coordinates are supported for |value| < 2^30 (outside, where the reference's int arithmetic
 * overflows, an entry whose z2 leaves int32 is not drawn). workspace:
 * pn2_render_ball_workspace_size(F, h, w) bytes (the keys and each frame's depth range),
 * 8-byte aligned; the call zeroes it.
 * PN2_EINVAL, checked before any launch: F, n, h or w negative, n >= 2^31, h * w >= 2^31,
 * F > 65535, r > PN2_RENDER_MAX_RADIUS, a background byte outside [0, 255], a NULL images, a
 * workspace that is NULL, misaligned or too small, and for n > 0 a NULL ixyz, a NULL channel
 * without labels, labels without a palette or with npal < 1. F, h or w = 0 is a no-op; n = 0
 * returns the background. */
#define PN2_RENDER_MAX_RADIUS 32767
size_t pn2_render_ball_workspace_size(int F, int h, int w);
int pn2_render_ball(const int32_t* ixyz, int F, long long n, const float* c0, const float* c1,
                    const float* c2, const int32_t* labels, const float* palette, int npal, int r,
                    int h, int w, int bg0, int bg1, int bg2, uint8_t* images, void* workspace,
                    size_t workspace_bytes, pn2_stream_t stream);
/* The viewer's projection, xyz.dot(rotmat) + offset and astype('int32'), for F frames. xyz (n,3)
 * fp32 (is_f64 = 0) or fp64 (is_f64 != 0), already centred and scaled; mats (F,12) fp64: each
 * frame's 3x3 matrix R row-major, then the offset. ixyz (F,n,3) int32:
 *   ixyz[f,i,k] = int32(trunc((x*R[0][k] + y*R[1][k]) + z*R[2][k] + off[k]))
 * in double, in exactly that order, no contraction; a value outside int32 (or NaN) gives
 * INT32_MIN as the reference's conversion does on x86. Supported range: |value| < 2^30.
 * PN2_EINVAL before any launch: F or n negative, n >= 2^31, a NULL buffer, mats (or an fp64
 * xyz) not 8-byte aligned. F = 0 or n = 0 is a no-op. */
int pn2_render_project(const void* xyz, int is_f64, long long n, const double* mats, int F,
                       int32_t* ixyz, pn2_stream_t stream);
/* The same two functions on HOST pointers in plain C++, synchronous, without workspace: equal
 * bits. */
int pn2cpu_render_ball(const int32_t* ixyz, int F, long long n, const float* c0, const float* c1,
                       const float* c2, const int32_t* labels, const float* palette, int npal,
                       int r, int h, int w, int bg0, int bg1, int bg2, uint8_t* images);
int pn2cpu_render_project(const void* xyz, int is_f64, long long n, const double* mats, int F,
                          int32_t* ixyz);

#ifdef __cplusplus
}
#endif
#endif /* PN2HIP_H */
