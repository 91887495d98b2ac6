// torch_ops.cpp — the pn2hip C ABI (include/pn2hip.h) registered as PyTorch operators,
// torch.ops.pn2.*, with the reference's op names, argument order and shape checks.
//
// This is layer (2) of the drop-in boundary: the reference exposes these
// as TensorFlow custom ops loaded by tf.load_op_library (tf_sampling.py:13, tf_grouping.py:7,
// tf_interpolate.py:7) whose OP_REQUIRES checks raise InvalidArgument; here every check raises
// ValueError (TORCH_CHECK_VALUE) with the reference's message, outputs come from the caching
// allocator, and every launch goes on the current HIP stream of the input's device
// (c10::hip::getCurrentHIPStream), so the ops compose with torch streams and hipGraph capture.
// Each op has one body, registered under the CUDA (= HIP on ROCm) and the Meta dispatch keys:
// fake tensors and torch.compile get the device call's checks, dtypes and output shapes, and the
// body returns before its first launch.
// Autograd for gather_point / group_point / three_interpolate (w.r.t.
// the points only, tf_sampling.py:44-48, tf_grouping.py:42-46, tf_interpolate.py:29-34) and
// attn_reduce (and the attention networks' attn_reduce_kd and head_mix, csrc/attn_net.hip)
// is registered from Python (torch.library.register_autograd, _torch_ops.py), and
// so is the training-mode shared-MLP layer's (mlp_layer_train -> mlp_layer_train_grad, and
// mlp_layer_train_pool -> mlp_layer_train_pool_grad for the layer fused with the max pool), the
// training-mode attention layer's (attn_kv_train -> attn_kv_train_grad) and the stand-alone
// batch-statistics batch norm's (bn_train -> bn_train_grad). The training head's autograd
// (dropout -> dropout with the same seed, softmax_xent -> softmax_xent_grad;
// csrc/head_train.hip) is registered here, in C++: see "autograd (C++)" below.
// CPU kernels exist only for the three ops the reference itself runs on the CPU (ThreeNN,
// ThreeInterpolate, ThreeInterpolateGrad: registered for DEVICE_CPU only,
// tf_interpolate.cpp:187,222,262), through the host twins pn2cpu_* (csrc/cpu_interp.cpp);
// and for the four prediction ops (scene_vote, scene_labels, map_back_rows, label_lut: integers
// and copied bytes, host twins in csrc/cpu_predict.cpp with equal bits) and the three feed ops
// (feed_batch, val_select, val_chunks: host twins in csrc/cpu_feed.cpp with equal bits) and the two
// rendering ops (render_ball, render_project: host twins in csrc/cpu_render.cpp with equal bits).
// Those twelve bodies are templates over HIP / CPU; every other op has no CPU kernel, so a CPU tensor fails in the
// dispatcher (no CPU fallback).
#include <ATen/ATen.h>
#include <c10/hip/HIPGuard.h>
#include <c10/hip/HIPStream.h>
#include <torch/csrc/autograd/custom_function.h>
#include <torch/library.h>

#include <climits>
#include <initializer_list>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/pn2hip.h"

namespace {

using at::Tensor;

pn2_stream_t stream_of(const Tensor& t) {
  return reinterpret_cast<pn2_stream_t>(c10::hip::getCurrentHIPStream(t.device().index()).stream());
}

void check_rc(int rc, const char* op) {
  TORCH_CHECK_VALUE(rc != PN2_EINVAL, op, ": invalid argument");
  TORCH_CHECK(rc != PN2_EFAULT, op, ": an earlier sampler launch reported a device fault ",
              "(its indices are not trustworthy; see pn2_fault_status)");
  TORCH_CHECK(rc == 0, op, ": HIP error ", rc, ": ", pn2_strerror(rc));
}

// a fake tensor (the Meta key): the body runs up to its allocations and returns them
bool fake(const Tensor& t) { return t.device().type() == at::kMeta; }

// A GPU (or Meta) input of the reference dtype, made contiguous.
Tensor dev(const Tensor& t, const char* name, at::ScalarType dt) {
  TORCH_CHECK(t.is_cuda() || fake(t), name, " is on ", t.device(),
              ": pn2hip ops run on the MI355X only (no CPU fallback)");
  TORCH_CHECK_TYPE(t.scalar_type() == dt, name, " must be ", dt, ", got ", t.scalar_type());
  return t.contiguous();
}

// dev() for an argument whose C function demands 16-byte alignment (the attention reductions,
// include/pn2hip.h): a contiguous view at an odd offset into a larger buffer is copied to a
// fresh allocation. Arguments whose kernels have a scalar path go through dev() and stay put.
Tensor dev16(const Tensor& t, const char* name, at::ScalarType dt) {
  Tensor c = dev(t, name, dt);
  if (!fake(c) && reinterpret_cast<uintptr_t>(c.data_ptr()) % 16 != 0) c = c.clone();
  return c;
}

int I(int64_t v) { return static_cast<int>(v); }
at::TensorOptions f32(const Tensor& like) { return like.options().dtype(at::kFloat); }
at::TensorOptions i32(const Tensor& like) { return like.options().dtype(at::kInt); }
void* P(const Tensor& t) { return t.defined() ? t.data_ptr() : nullptr; }
const float* F(const Tensor& t) { return t.defined() ? t.data_ptr<float>() : nullptr; }
const int32_t* Ii(const Tensor& t) { return t.data_ptr<int32_t>(); }

// ------------------------------------------------------------------------- shape checks
// (the messages are the reference's OP_REQUIRES texts)
void chk_fps(int64_t npoint, const Tensor& inp) {
  TORCH_CHECK_VALUE(npoint > 0, "FarthestPointSample expects positive npoint");  // tf_sampling.cpp:99
  TORCH_CHECK_VALUE(inp.dim() == 3 && inp.size(2) == 3,                          // :105
                    "FarthestPointSample expects (batch_size,num_points,3) inp shape");
}
void chk_gather(const Tensor& inp, const Tensor& idx, const char* name) {
  TORCH_CHECK_VALUE(inp.dim() == 3 && inp.size(2) == 3, name,                    // :131
                    " expects (batch_size,num_points,3) inp shape");
  TORCH_CHECK_VALUE(idx.dim() == 2 && idx.size(0) == inp.size(0), name,          // :135
                    " expects (batch_size,num_result) idx shape");
}
void chk_prob(const Tensor& inp, const Tensor& inpr) {
  TORCH_CHECK_VALUE(inp.dim() == 2, "ProbSample expects (batch_size,num_choices) inp shape");
  TORCH_CHECK_VALUE(inpr.dim() == 2 && inpr.size(0) == inp.size(0),               // :76-79
                    "ProbSample expects (batch_size,num_points) inpr shape");
}
void chk_ball(double radius, int64_t nsample, const Tensor& xyz1, const Tensor& xyz2) {
  TORCH_CHECK_VALUE(radius > 0, "QueryBallPoint expects positive radius");    // tf_grouping.cpp:71
  TORCH_CHECK_VALUE(nsample > 0, "QueryBallPoint expects positive nsample");  // :74
  TORCH_CHECK_VALUE(xyz1.dim() == 3 && xyz1.size(2) == 3,                      // :79
                    "QueryBallPoint expects (batch_size, ndataset, 3) xyz1 shape.");
  TORCH_CHECK_VALUE(xyz2.dim() == 3 && xyz2.size(2) == 3,                      // :84
                    "QueryBallPoint expects (batch_size, npoint, 3) xyz2 shape.");
  TORCH_CHECK_VALUE(xyz1.size(0) == xyz2.size(0),
                    "QueryBallPoint expects xyz1 and xyz2 with the same batch size");
}
void chk_group(const Tensor& points, const Tensor& idx, const char* name) {
  TORCH_CHECK_VALUE(points.dim() == 3, name,                                   // :149
                    " expects (batch_size, num_points, channel) points shape");
  TORCH_CHECK_VALUE(idx.dim() == 3 && idx.size(0) == points.size(0), name,     // :155
                    " expects (batch_size, npoints, nsample) idx shape");
}
void chk_nn(const Tensor& xyz1, const Tensor& xyz2) {
  TORCH_CHECK_VALUE(xyz1.dim() == 3 && xyz1.size(2) == 3,            // tf_interpolate.cpp:163
                    "ThreeNN expects (b,n,3) xyz1 shape.");
  TORCH_CHECK_VALUE(xyz2.dim() == 3 && xyz2.size(2) == 3,            // :168
                    "ThreeNN expects (b,m,3) xyz2 shape.");
  TORCH_CHECK_VALUE(xyz1.size(0) == xyz2.size(0), "ThreeNN expects xyz1 and xyz2 with the same b");
}
void chk_interp(const Tensor& points, const Tensor& idx, const Tensor& weight, const char* name) {
  TORCH_CHECK_VALUE(points.dim() == 3, name, " expects (b,m,c) points shape");  // :197
  const int64_t b = points.size(0);
  TORCH_CHECK_VALUE(idx.dim() == 3 && idx.size(0) == b && idx.size(2) == 3, name,  // :203
                    " expects (b,n,3) idx shape");
  TORCH_CHECK_VALUE(weight.dim() == 3 && weight.size(0) == b && weight.size(1) == idx.size(1) &&
                        weight.size(2) == 3,
                    name, " expects (b,n,3) weight shape");                       // :206
}
void chk_attn(const Tensor& Q, const Tensor& K, const Tensor& V) {
  TORCH_CHECK_VALUE(Q.dim() == 3 && K.dim() == 4 && V.sizes() == K.sizes() &&
                        K.size(0) == Q.size(0) && K.size(1) == Q.size(1) && K.size(3) == Q.size(2),
                    "attn_reduce expects Q (B,M,C) and K, V (B,M,ns,C)");
  TORCH_CHECK_VALUE(Q.size(2) % 4 == 0, "attn_reduce expects C % 4 == 0 (key_dim 4)");
}
// fused group + centre + concat (pointnet_util.py:16-58 / :180-191): every tensor must agree
// with xyz's batch and point count, or the kernel would index past idx, new_xyz or points
void chk_group_concat(const Tensor& xyz, const std::optional<Tensor>& points,
                      const Tensor& new_xyz, const Tensor& idx) {
  TORCH_CHECK_VALUE(xyz.dim() == 3 && xyz.size(2) == 3 && new_xyz.dim() == 3 &&
                        new_xyz.size(2) == 3 && idx.dim() == 3 && idx.size(1) == new_xyz.size(1),
                    "group_concat expects xyz (B,N,3), new_xyz (B,M,3), idx (B,M,ns)");
  TORCH_CHECK_VALUE(new_xyz.size(0) == xyz.size(0) && idx.size(0) == xyz.size(0),
                    "group_concat expects xyz, new_xyz and idx with the same batch size");
  if (points.has_value() && points->numel() > 0)
    TORCH_CHECK_VALUE(points->dim() == 3 && points->size(0) == xyz.size(0) &&
                          points->size(1) == xyz.size(1),
                      "group_concat expects points (B,N,C) for xyz (B,N,3)");
}
// pooling over nsample (pointnet_util.py:130-145); weighted_avg needs grouped_xyz (B,M,ns,3)
void chk_group_pool(const Tensor& x, const std::optional<Tensor>& gxyz, int64_t mode) {
  TORCH_CHECK_VALUE(x.dim() == 4, "group_pool expects (B,M,ns,C) x");
  TORCH_CHECK_VALUE(mode >= PN2_POOL_MAX && mode <= PN2_POOL_MAX_AND_AVG, "group_pool: unknown mode");
  if (mode == PN2_POOL_WEIGHTED_AVG)
    TORCH_CHECK_VALUE(gxyz.has_value() && gxyz->dim() == 4 && gxyz->size(0) == x.size(0) &&
                          gxyz->size(1) == x.size(1) && gxyz->size(2) == x.size(2) &&
                          gxyz->size(3) == 3,
                      "group_pool weighted_avg needs grouped_xyz (B,M,ns,3)");
}

// Clouds / query batches at least this large take the spatial grid (identical results;
// tf_grouping.GRID_MIN_* and tf_interpolate.GRID_MIN_* read the same defines).
constexpr int64_t kBallGridMinPoints = PN2_BALL_GRID_MIN_POINTS,
                  kBallGridMinQueries = PN2_BALL_GRID_MIN_QUERIES;
constexpr int64_t kNnGridMinPairs = PN2_NN_GRID_MIN_PAIRS, kNnGridMinKnown = PN2_NN_GRID_MIN_KNOWN;

Tensor grid_over(const Tensor& xyz, double cell_edge, const char* op) {
  const int B = I(xyz.size(0)), N = I(xyz.size(1));
  const size_t bytes = pn2_grid_size(B, N);
  Tensor g = at::empty({static_cast<int64_t>(bytes > 16 ? bytes : 16)}, xyz.options().dtype(at::kByte));
  check_rc(pn2_grid_build(F(xyz), B, N, static_cast<float>(cell_edge), P(g), bytes, stream_of(xyz)), op);
  return g;
}

// ------------------------------------------------------------------------- the ops' bodies
// Each: the shape checks; the inputs (dev / dev16 / dev_opt) and every output; the return for Meta;
// then the device guard, workspaces and launches.
std::tuple<Tensor, Tensor> fps_and_gather_hip(int64_t npoint, const Tensor& inp_) {
  chk_fps(npoint, inp_);
  Tensor inp = dev(inp_, "inp", at::kFloat);
  const int B = I(inp.size(0)), N = I(inp.size(1)), M = I(npoint);
  Tensor idx = at::empty({B, M}, i32(inp));
  Tensor nx = at::empty({B, M, 3}, f32(inp));
  if (fake(inp) || B == 0) return {idx, nx};
  c10::hip::HIPGuard g(inp.device().index());
  const size_t ws = pn2_fps_workspace_size(B, N);
  if (ws) {
    Tensor w = at::empty({static_cast<int64_t>((ws + 3) / 4)}, f32(inp));
    check_rc(pn2_fps_ws(F(inp), B, N, M, idx.data_ptr<int32_t>(), nx.data_ptr<float>(), P(w), ws,
                        stream_of(inp)), "FarthestPointSample");
  } else {
    check_rc(pn2_fps_gather(F(inp), B, N, M, idx.data_ptr<int32_t>(), nx.data_ptr<float>(),
                            stream_of(inp)), "FarthestPointSample");
  }
  return {idx, nx};
}
Tensor fps_hip(int64_t npoint, const Tensor& inp) { return std::get<0>(fps_and_gather_hip(npoint, inp)); }

Tensor gather_point_hip(const Tensor& inp_, const Tensor& idx_) {
  chk_gather(inp_, idx_, "GatherPoint");
  Tensor inp = dev(inp_, "inp", at::kFloat), idx = dev(idx_, "idx", at::kInt);
  const int B = I(inp.size(0)), N = I(inp.size(1)), M = I(idx.size(1));
  Tensor out = at::empty({B, M, 3}, f32(inp));
  if (fake(inp)) return out;
  c10::hip::HIPGuard g(inp.device().index());
  check_rc(pn2_gather_point(F(inp), Ii(idx), B, N, M, out.data_ptr<float>(), stream_of(inp)),
           "GatherPoint");
  return out;
}

Tensor gather_point_grad_hip(const Tensor& inp, const Tensor& idx_, const Tensor& out_g_) {
  chk_gather(inp, idx_, "GatherPointGradGpuOp");
  const int B = I(inp.size(0)), N = I(inp.size(1)), M = I(idx_.size(1));
  TORCH_CHECK_VALUE(out_g_.dim() == 3 && out_g_.size(0) == B && out_g_.size(1) == M &&
                        out_g_.size(2) == 3,
                    "GatherPointGradGpuOp expects (batch_size,num_result,3) out_g shape");
  Tensor idx = dev(idx_, "idx", at::kInt), out_g = dev(out_g_, "out_g", at::kFloat);
  Tensor inp_g = at::empty({B, N, 3}, f32(out_g));
  if (fake(out_g)) return inp_g;
  c10::hip::HIPGuard g(out_g.device().index());
  check_rc(pn2_gather_point_grad(F(out_g), Ii(idx), B, N, M, inp_g.data_ptr<float>(),
                                 stream_of(out_g)), "GatherPointGrad");
  return inp_g;
}

Tensor prob_sample_hip(const Tensor& inp_, const Tensor& inpr_) {
  chk_prob(inp_, inpr_);
  Tensor inp = dev(inp_, "inp", at::kFloat), inpr = dev(inpr_, "inpr", at::kFloat);
  const int B = I(inp.size(0)), N = I(inp.size(1)), M = I(inpr.size(1));
  Tensor out = at::empty({B, M}, i32(inp));
  if (fake(inp) || B == 0 || M == 0) return out;
  c10::hip::HIPGuard g(inp.device().index());
  const size_t ws = pn2_prob_sample_workspace_size(B, N);
  Tensor w = at::empty({static_cast<int64_t>(ws / 4 > 1 ? ws / 4 : 1)}, f32(inp));
  check_rc(pn2_prob_sample(F(inp), F(inpr), B, N, M, w.data_ptr<float>(), ws,
                           out.data_ptr<int32_t>(), stream_of(inp)), "ProbSample");
  return out;
}

std::tuple<Tensor, Tensor> query_ball_point_hip(double radius, int64_t nsample, const Tensor& xyz1_,
                                                const Tensor& xyz2_) {
  chk_ball(radius, nsample, xyz1_, xyz2_);
  Tensor xyz1 = dev(xyz1_, "xyz1", at::kFloat), xyz2 = dev(xyz2_, "xyz2", at::kFloat);
  const int B = I(xyz1.size(0)), N = I(xyz1.size(1)), M = I(xyz2.size(1)), ns = I(nsample);
  Tensor idx = at::empty({B, M, ns}, i32(xyz1));
  Tensor cnt = at::empty({B, M}, i32(xyz1));
  if (fake(xyz1)) return {idx, cnt};
  c10::hip::HIPGuard g(xyz1.device().index());
  const float r = static_cast<float>(radius);
  if (N >= kBallGridMinPoints && int64_t(B) * M >= kBallGridMinQueries) {
    Tensor grid = grid_over(xyz1, r, "QueryBallPoint");
    check_rc(pn2_ball_query_grid(P(grid), F(xyz2), B, N, M, r, ns, idx.data_ptr<int32_t>(),
                                 cnt.data_ptr<int32_t>(), stream_of(xyz1)), "QueryBallPoint");
  } else {
    check_rc(pn2_ball_query(F(xyz1), F(xyz2), B, N, M, r, ns, idx.data_ptr<int32_t>(),
                            cnt.data_ptr<int32_t>(), stream_of(xyz1)), "QueryBallPoint");
  }
  return {idx, cnt};
}

std::tuple<Tensor, Tensor> select_top_k_hip(int64_t k, const Tensor& dist_) {
  TORCH_CHECK_VALUE(k > 0, "SelectionSort expects positive k");                    // :113
  TORCH_CHECK_VALUE(dist_.dim() == 3, "SelectionSort expects (b,m,n) dist shape.");  // :118
  TORCH_CHECK_VALUE(k <= dist_.size(2), "SelectionSort expects k <= n");
  Tensor dist = dev(dist_, "dist", at::kFloat);
  const int B = I(dist.size(0)), m = I(dist.size(1)), n = I(dist.size(2));
  Tensor outi = at::empty({B, m, n}, i32(dist));
  Tensor out = at::empty({B, m, n}, f32(dist));
  if (fake(dist)) return {outi, out};
  c10::hip::HIPGuard g(dist.device().index());
  size_t ws = pn2_select_top_k_workspace_size(B, m, I(k));
  Tensor w = at::empty({static_cast<int64_t>(ws > 16 ? ws : 16)}, dist.options().dtype(at::kByte));
  check_rc(pn2_select_top_k(F(dist), B, m, n, I(k), outi.data_ptr<int32_t>(), out.data_ptr<float>(),
                            static_cast<int32_t*>(P(w)), stream_of(dist)), "SelectionSort");
  return {outi, out};
}

void chk_knn(int64_t k, const Tensor& xyz1, const Tensor& xyz2) {
  TORCH_CHECK_VALUE(xyz1.dim() == 3 && xyz2.dim() == 3 && xyz1.size(0) == xyz2.size(0) &&
                        xyz1.size(2) == xyz2.size(2),
                    "knn_point expects (b,n,c) xyz1 and (b,m,c) xyz2");
  TORCH_CHECK_VALUE(k > 0 && k <= xyz1.size(1), "SelectionSort expects positive k");
}

std::tuple<Tensor, Tensor> knn_point_hip(int64_t k, const Tensor& xyz1_, const Tensor& xyz2_) {
  chk_knn(k, xyz1_, xyz2_);
  Tensor xyz1 = dev(xyz1_, "xyz1", at::kFloat), xyz2 = dev(xyz2_, "xyz2", at::kFloat);
  const int B = I(xyz1.size(0)), n = I(xyz1.size(1)), c = I(xyz1.size(2)), m = I(xyz2.size(1));
  Tensor val = at::empty({B, m, k}, f32(xyz1));
  Tensor idx = at::empty({B, m, k}, i32(xyz1));
  if (fake(xyz1)) return {val, idx};
  c10::hip::HIPGuard g(xyz1.device().index());
  check_rc(pn2_knn_point(F(xyz1), F(xyz2), B, n, m, c, I(k), val.data_ptr<float>(),
                         idx.data_ptr<int32_t>(), stream_of(xyz1)), "knn_point");
  return {val, idx};
}

Tensor group_point_hip(const Tensor& points_, const Tensor& idx_) {
  chk_group(points_, idx_, "GroupPoint");
  Tensor points = dev(points_, "points", at::kFloat), idx = dev(idx_, "idx", at::kInt);
  const int B = I(points.size(0)), N = I(points.size(1)), C = I(points.size(2));
  const int M = I(idx.size(1)), ns = I(idx.size(2));
  Tensor out = at::empty({B, M, ns, C}, f32(points));
  if (fake(points)) return out;
  c10::hip::HIPGuard g(points.device().index());
  check_rc(pn2_group_point(F(points), Ii(idx), B, N, C, M, ns, out.data_ptr<float>(),
                           stream_of(points)), "GroupPoint");
  return out;
}

Tensor group_point_grad_hip(const Tensor& points, const Tensor& idx_, const Tensor& grad_out_) {
  chk_group(points, idx_, "GroupPointGrad");
  const int B = I(points.size(0)), N = I(points.size(1)), C = I(points.size(2));
  const int M = I(idx_.size(1)), ns = I(idx_.size(2));
  TORCH_CHECK_VALUE(grad_out_.dim() == 4 && grad_out_.size(0) == B && grad_out_.size(1) == M &&
                        grad_out_.size(2) == ns && grad_out_.size(3) == C,  // tf_grouping.cpp:191
                    "GroupPointGrad expects (batch_size, npoints, nsample, channel) grad_out shape");
  Tensor idx = dev(idx_, "idx", at::kInt), grad_out = dev(grad_out_, "grad_out", at::kFloat);
  Tensor gp = at::empty({B, N, C}, f32(grad_out));
  if (fake(grad_out)) return gp;
  c10::hip::HIPGuard g(grad_out.device().index());
  check_rc(pn2_group_point_grad(F(grad_out), Ii(idx), B, N, C, M, ns, gp.data_ptr<float>(),
                                stream_of(grad_out)), "GroupPointGrad");
  return gp;
}

// (want_gx false: grouped_xyz is not written and comes back undefined)
std::tuple<Tensor, Tensor> group_concat_impl(const Tensor& xyz_, const std::optional<Tensor>& points_,
                                             const Tensor& new_xyz_, const Tensor& idx_, bool use_xyz,
                                             bool xyz_last, bool want_gx) {
  chk_group_concat(xyz_, points_, new_xyz_, idx_);
  Tensor xyz = dev(xyz_, "xyz", at::kFloat), new_xyz = dev(new_xyz_, "new_xyz", at::kFloat);
  Tensor idx = dev(idx_, "idx", at::kInt);
  Tensor points;
  if (points_.has_value() && points_->numel() > 0) points = dev(*points_, "points", at::kFloat);
  const int B = I(xyz.size(0)), N = I(xyz.size(1)), M = I(idx.size(1)), ns = I(idx.size(2));
  const int C = points.defined() ? I(points.size(2)) : 0;
  const int cout = !points.defined() ? 3 : (use_xyz ? C + 3 : C);
  Tensor gx;
  if (want_gx) gx = at::empty({B, M, ns, 3}, f32(xyz));
  Tensor np = at::empty({B, M, ns, cout}, f32(xyz));
  if (fake(xyz)) return {gx, np};
  c10::hip::HIPGuard g(xyz.device().index());
  const int flags = (use_xyz ? PN2_USE_XYZ : 0) | (xyz_last ? PN2_XYZ_LAST : 0);
  check_rc(pn2_group_concat(F(xyz), F(points), F(new_xyz), Ii(idx), B, N, C, M, ns, flags,
                            want_gx ? gx.data_ptr<float>() : nullptr, np.data_ptr<float>(),
                            stream_of(xyz)),
           "group_concat");
  return {gx, np};
}
std::tuple<Tensor, Tensor> group_concat_hip(const Tensor& xyz, const std::optional<Tensor>& points,
                                            const Tensor& new_xyz, const Tensor& idx, bool use_xyz,
                                            bool xyz_last) {
  return group_concat_impl(xyz, points, new_xyz, idx, use_xyz, xyz_last, true);
}

// The three ops the reference itself runs on the CPU have host twins (csrc/cpu_interp.cpp):
// HIP false is the CPU kernel, which takes its inputs through host() and calls pn2cpu_*.
Tensor host(const Tensor& t, const char* name, at::ScalarType dt) {
  TORCH_CHECK(t.device().is_cpu(), name, " must be a CPU tensor here");
  TORCH_CHECK_TYPE(t.scalar_type() == dt, name, " must be ", dt, ", got ", t.scalar_type());
  return t.contiguous();
}

template <bool HIP>
std::tuple<Tensor, Tensor> three_nn_impl(const Tensor& xyz1_, const Tensor& xyz2_) {
  chk_nn(xyz1_, xyz2_);
  const auto in = HIP ? dev : host;
  Tensor xyz1 = in(xyz1_, "xyz1", at::kFloat), xyz2 = in(xyz2_, "xyz2", at::kFloat);
  const int B = I(xyz1.size(0)), n = I(xyz1.size(1)), m = I(xyz2.size(1));
  Tensor dist = at::empty({B, n, 3}, f32(xyz1));
  Tensor idx = at::empty({B, n, 3}, i32(xyz1));
  if (fake(xyz1)) return {dist, idx};
  if (!HIP) {
    check_rc(pn2cpu_three_nn(F(xyz1), F(xyz2), B, n, m, dist.data_ptr<float>(),
                             idx.data_ptr<int32_t>()), "ThreeNN");
    return {dist, idx};
  }
  c10::hip::HIPGuard g(xyz1.device().index());
  if (int64_t(n) * m >= kNnGridMinPairs && m >= kNnGridMinKnown) {
    Tensor grid = grid_over(xyz2, 0.0, "ThreeNN");
    check_rc(pn2_three_nn_grid(P(grid), nullptr, F(xyz1), B, n, m, dist.data_ptr<float>(),
                               idx.data_ptr<int32_t>(), stream_of(xyz1)), "ThreeNN");
  } else {
    check_rc(pn2_three_nn(F(xyz1), F(xyz2), B, n, m, dist.data_ptr<float>(),
                          idx.data_ptr<int32_t>(), stream_of(xyz1)), "ThreeNN");
  }
  return {dist, idx};
}

template <bool HIP>
Tensor three_interpolate_impl(const Tensor& points_, const Tensor& idx_, const Tensor& weight_) {
  chk_interp(points_, idx_, weight_, "ThreeInterpolate");
  const auto in = HIP ? dev : host;
  Tensor points = in(points_, "points", at::kFloat), idx = in(idx_, "idx", at::kInt);
  Tensor weight = in(weight_, "weight", at::kFloat);
  const int B = I(points.size(0)), m = I(points.size(1)), C = I(points.size(2)), n = I(idx.size(1));
  Tensor out = at::empty({B, n, C}, f32(points));
  if (fake(points)) return out;
  if (HIP) {
    c10::hip::HIPGuard g(points.device().index());
    check_rc(pn2_three_interpolate(F(points), Ii(idx), F(weight), B, m, C, n,
                                   out.data_ptr<float>(), stream_of(points)), "ThreeInterpolate");
  } else {
    check_rc(pn2cpu_three_interpolate(F(points), Ii(idx), F(weight), B, m, C, n,
                                      out.data_ptr<float>()), "ThreeInterpolate");
  }
  return out;
}

template <bool HIP>
Tensor three_interpolate_grad_impl(const Tensor& points, const Tensor& idx_, const Tensor& weight_,
                                   const Tensor& grad_out_) {
  chk_interp(points, idx_, weight_, "ThreeInterpolateGrad");
  const int B = I(points.size(0)), m = I(points.size(1)), C = I(points.size(2)), n = I(idx_.size(1));
  TORCH_CHECK_VALUE(grad_out_.dim() == 3 && grad_out_.size(0) == B && grad_out_.size(1) == n &&
                        grad_out_.size(2) == C,  // tf_interpolate.cpp:243
                    "ThreeInterpolateGrad expects (b,n,c) grad_out shape");
  const auto in = HIP ? dev : host;
  Tensor idx = in(idx_, "idx", at::kInt), weight = in(weight_, "weight", at::kFloat);
  Tensor grad_out = in(grad_out_, "grad_out", at::kFloat);
  Tensor gp = at::empty({B, m, C}, f32(grad_out));
  if (fake(grad_out)) return gp;
  if (HIP) {
    c10::hip::HIPGuard g(grad_out.device().index());
    check_rc(pn2_three_interpolate_grad(F(grad_out), Ii(idx), F(weight), B, n, C, m,
                                        gp.data_ptr<float>(), stream_of(grad_out)),
             "ThreeInterpolateGrad");
  } else {
    check_rc(pn2cpu_three_interpolate_grad(F(grad_out), Ii(idx), F(weight), B, n, C, m,
                                           gp.data_ptr<float>()), "ThreeInterpolateGrad");
  }
  return gp;
}

Tensor idw_weights_hip(const Tensor& dist_) {
  TORCH_CHECK_VALUE(dist_.dim() == 3 && dist_.size(2) == 3, "idw_weights expects (b,n,3) dist shape");
  Tensor dist = dev(dist_, "dist", at::kFloat);
  Tensor w = at::empty_like(dist);
  if (fake(dist)) return w;
  c10::hip::HIPGuard g(dist.device().index());
  check_rc(pn2_idw_weights(F(dist), I(dist.size(0)), I(dist.size(1)), w.data_ptr<float>(),
                           stream_of(dist)), "idw_weights");
  return w;
}

Tensor fp_fused_hip(const Tensor& xyz1_, const Tensor& xyz2_, const std::optional<Tensor>& points1_,
                    const Tensor& points2_) {
  chk_nn(xyz1_, xyz2_);
  TORCH_CHECK_VALUE(points2_.dim() == 3 && points2_.size(0) == xyz2_.size(0) &&
                        points2_.size(1) == xyz2_.size(1),
                    "fp_fused expects (b,m,c2) points2");
  Tensor xyz1 = dev(xyz1_, "xyz1", at::kFloat), xyz2 = dev(xyz2_, "xyz2", at::kFloat);
  Tensor points2 = dev(points2_, "points2", at::kFloat);
  Tensor points1;
  if (points1_.has_value() && points1_->numel() > 0) {
    TORCH_CHECK_VALUE(points1_->dim() == 3 && points1_->size(0) == xyz1.size(0) &&
                          points1_->size(1) == xyz1.size(1),
                      "fp_fused expects (b,n,c1) points1");
    points1 = dev(*points1_, "points1", at::kFloat);
  }
  const int B = I(xyz1.size(0)), n = I(xyz1.size(1)), m = I(xyz2.size(1)), C2 = I(points2.size(2));
  const int C1 = points1.defined() ? I(points1.size(2)) : 0;
  Tensor out = at::empty({B, n, C2 + C1}, f32(xyz1));
  if (fake(xyz1)) return out;
  c10::hip::HIPGuard g(xyz1.device().index());
  check_rc(pn2_fp_fused(F(xyz1), F(xyz2), F(points1), C1, F(points2), C2, B, n, m,
                        out.data_ptr<float>(), stream_of(xyz1)), "fp_fused");
  return out;
}

Tensor attn_reduce_hip(const Tensor& Q_, const Tensor& K_, const Tensor& V_) {
  chk_attn(Q_, K_, V_);
  Tensor Q = dev16(Q_, "Q", at::kFloat), K = dev16(K_, "K", at::kFloat);
  Tensor V = dev16(V_, "V", at::kFloat);
  const int B = I(K.size(0)), M = I(K.size(1)), ns = I(K.size(2)), C = I(K.size(3));
  Tensor out = at::empty({B, M, C}, f32(Q));
  if (fake(Q)) return out;
  c10::hip::HIPGuard g(Q.device().index());
  check_rc(pn2_attn_reduce(F(Q), F(K), F(V), B, M, ns, C, out.data_ptr<float>(), stream_of(Q)),
           "attn_reduce");
  return out;
}

std::tuple<Tensor, Tensor, Tensor> attn_reduce_grad_hip(const Tensor& Q_, const Tensor& K_,
                                                        const Tensor& V_, const Tensor& go_) {
  chk_attn(Q_, K_, V_);
  TORCH_CHECK_VALUE(go_.sizes() == Q_.sizes(), "attn_reduce_grad expects grad_out shaped like Q");
  Tensor Q = dev16(Q_, "Q", at::kFloat), K = dev16(K_, "K", at::kFloat);
  Tensor V = dev16(V_, "V", at::kFloat), go = dev16(go_, "grad_out", at::kFloat);
  const int B = I(K.size(0)), M = I(K.size(1)), ns = I(K.size(2)), C = I(K.size(3));
  Tensor gQ = at::empty_like(Q), gK = at::empty_like(K), gV = at::empty_like(V);
  if (fake(Q)) return {gQ, gK, gV};
  c10::hip::HIPGuard g(Q.device().index());
  check_rc(pn2_attn_reduce_grad(F(Q), F(K), F(V), F(go), B, M, ns, C, gQ.data_ptr<float>(),
                                gK.data_ptr<float>(), gV.data_ptr<float>(), stream_of(Q)),
           "attn_reduce_grad");
  return {gQ, gK, gV};
}

// the reduction for any key_dim (csrc/attn_net.hip); the checks are pn2_attn_reduce_kd's, made
// here so that a fake tensor meets them too
void chk_attn_kd(const Tensor& Q, const Tensor& K, const Tensor& V, int64_t kd, const char* op) {
  TORCH_CHECK_VALUE(Q.dim() == 3 && K.dim() == 4 && V.sizes() == K.sizes() &&
                        K.size(0) == Q.size(0) && K.size(1) == Q.size(1) && K.size(3) == Q.size(2),
                    op, " expects Q (B,M,C) and K, V (B,M,ns,C)");
  TORCH_CHECK_VALUE(kd >= 4 && kd <= 512 && kd % 4 == 0, op,
                    " expects key_dim % 4 == 0, 4 <= key_dim <= 512");
  TORCH_CHECK_VALUE(Q.size(2) % kd == 0, op, " expects C % key_dim == 0 (C = heads * key_dim)");
  TORCH_CHECK_VALUE(K.size(2) >= 1, op, " expects ns >= 1");
}

Tensor attn_reduce_kd_hip(const Tensor& Q_, const Tensor& K_, const Tensor& V_, int64_t kd) {
  chk_attn_kd(Q_, K_, V_, kd, "attn_reduce_kd");
  Tensor Q = dev16(Q_, "Q", at::kFloat), K = dev16(K_, "K", at::kFloat);
  Tensor V = dev16(V_, "V", at::kFloat);
  const int B = I(K.size(0)), M = I(K.size(1)), ns = I(K.size(2)), C = I(K.size(3));
  Tensor out = at::empty({B, M, C}, f32(Q));
  if (fake(Q)) return out;
  c10::hip::HIPGuard g(Q.device().index());
  check_rc(pn2_attn_reduce_kd(F(Q), F(K), F(V), B, M, ns, C, I(kd), out.data_ptr<float>(),
                              stream_of(Q)), "attn_reduce_kd");
  return out;
}

std::tuple<Tensor, Tensor, Tensor> attn_reduce_kd_grad_hip(const Tensor& Q_, const Tensor& K_,
                                                           const Tensor& V_, const Tensor& go_,
                                                           int64_t kd) {
  chk_attn_kd(Q_, K_, V_, kd, "attn_reduce_kd_grad");
  TORCH_CHECK_VALUE(go_.sizes() == Q_.sizes(),
                    "attn_reduce_kd_grad expects grad_out shaped like Q");
  Tensor Q = dev16(Q_, "Q", at::kFloat), K = dev16(K_, "K", at::kFloat);
  Tensor V = dev16(V_, "V", at::kFloat), go = dev16(go_, "grad_out", at::kFloat);
  const int B = I(K.size(0)), M = I(K.size(1)), ns = I(K.size(2)), C = I(K.size(3));
  Tensor gQ = at::empty_like(Q), gK = at::empty_like(K), gV = at::empty_like(V);
  if (fake(Q)) return {gQ, gK, gV};
  c10::hip::HIPGuard g(Q.device().index());
  check_rc(pn2_attn_reduce_kd_grad(F(Q), F(K), F(V), F(go), B, M, ns, C, I(kd),
                                   gQ.data_ptr<float>(), gK.data_ptr<float>(),
                                   gV.data_ptr<float>(), stream_of(Q)), "attn_reduce_kd_grad");
  return {gQ, gK, gV};
}

// head mixing (InnerAttentionLayer.call, csrc/attn_net.hip): qkv (..., 3*heads*key_dim)
void chk_head_mix(const Tensor& qkv, int64_t heads, int64_t kd, const char* op) {
  TORCH_CHECK_VALUE(heads >= 1 && heads <= PN2_HEAD_MIX_MAX_HEADS, op, " expects 1 <= heads <= ",
                    PN2_HEAD_MIX_MAX_HEADS);
  TORCH_CHECK_VALUE(kd >= 4 && kd <= 256 && kd % 4 == 0, op,
                    " expects key_dim % 4 == 0, 4 <= key_dim <= 256");
  TORCH_CHECK_VALUE(qkv.dim() >= 1 && qkv.size(-1) == 3 * heads * kd, op,
                    " expects qkv (..., 3 * heads * key_dim) = [Q | K | V]");
}

Tensor head_mix_hip(const Tensor& qkv_, int64_t heads, int64_t kd) {
  chk_head_mix(qkv_, heads, kd, "head_mix");
  Tensor qkv = dev16(qkv_, "qkv", at::kFloat);
  std::vector<int64_t> shape = qkv.sizes().vec();
  shape.back() = heads * kd;
  Tensor out = at::empty(shape, f32(qkv));
  if (fake(qkv)) return out;
  c10::hip::HIPGuard g(qkv.device().index());
  check_rc(pn2_head_mix(F(qkv), out.numel() / (heads * kd), I(heads), I(kd),
                        out.data_ptr<float>(), stream_of(qkv)), "head_mix");
  return out;
}

Tensor head_mix_grad_hip(const Tensor& qkv_, const Tensor& go_, int64_t heads, int64_t kd) {
  chk_head_mix(qkv_, heads, kd, "head_mix_grad");
  TORCH_CHECK_VALUE(go_.dim() == qkv_.dim() && go_.size(-1) == heads * kd &&
                        go_.sizes().slice(0, go_.dim() - 1) ==
                            qkv_.sizes().slice(0, qkv_.dim() - 1),
                    "head_mix_grad expects grad_out (..., heads * key_dim) for qkv's rows");
  Tensor qkv = dev16(qkv_, "qkv", at::kFloat), go = dev16(go_, "grad_out", at::kFloat);
  Tensor gqkv = at::empty_like(qkv);
  if (fake(qkv)) return gqkv;
  c10::hip::HIPGuard g(qkv.device().index());
  check_rc(pn2_head_mix_grad(F(qkv), F(go), go.numel() / (heads * kd), I(heads), I(kd),
                             gqkv.data_ptr<float>(), stream_of(qkv)), "head_mix_grad");
  return gqkv;
}

Tensor group_pool_hip(const Tensor& x_, const std::optional<Tensor>& gxyz_, int64_t mode) {
  chk_group_pool(x_, gxyz_, mode);
  Tensor x = dev(x_, "x", at::kFloat);
  Tensor gxyz;
  if (mode == PN2_POOL_WEIGHTED_AVG) gxyz = dev(*gxyz_, "grouped_xyz", at::kFloat);
  const int B = I(x.size(0)), M = I(x.size(1)), ns = I(x.size(2)), C = I(x.size(3));
  Tensor out = at::empty({B, M, mode == PN2_POOL_MAX_AND_AVG ? 2 * C : C}, f32(x));
  if (fake(x)) return out;
  c10::hip::HIPGuard g(x.device().index());
  check_rc(pn2_group_pool(F(x), F(gxyz), B, M, ns, C, I(mode), out.data_ptr<float>(), stream_of(x)),
           "group_pool");
  return out;
}

// ---- training-mode shared-MLP layer (csrc/mlp_train.hip): tf_util.conv2d with is_training
// (tf_util.py:165-185), conv + bias + batch-statistics batch norm + ReLU and its gradients
bool has(const std::optional<Tensor>& t) { return t.has_value() && t->defined(); }

// x (..., cin), weight (cin, cout), the per-channel vectors (cout) or all absent
void chk_mlp_layer(const Tensor& x, const Tensor& weight, const std::optional<Tensor>& bias,
                   const std::optional<Tensor>& gamma, const std::optional<Tensor>& beta,
                   const char* name) {
  TORCH_CHECK_VALUE(weight.dim() == 2 && weight.size(0) > 0 && weight.size(1) > 0, name,
                    " expects (cin, cout) weight");
  TORCH_CHECK_VALUE(x.dim() >= 1 && x.size(-1) == weight.size(0), name,
                    " expects (..., cin) x for (cin, cout) weight");
  TORCH_CHECK_VALUE(has(gamma) == has(beta), name, " expects gamma and beta together");
  const int64_t cout = weight.size(1);
  for (const auto* v : {&bias, &gamma, &beta})
    if (has(*v))
      TORCH_CHECK_VALUE((*v)->dim() == 1 && (*v)->size(0) == cout, name,
                        " expects (cout) bias, gamma and beta");
}
std::vector<int64_t> with_last(const Tensor& x, int64_t c) {
  std::vector<int64_t> s(x.sizes().begin(), x.sizes().end());
  s.back() = c;
  return s;
}
Tensor workspace(const Tensor& like, size_t bytes) {
  return at::empty({static_cast<int64_t>((bytes + 3) / 4 > 4 ? (bytes + 3) / 4 : 4)}, f32(like));
}

// out (rows, cout) = in (rows, cin) * w (cin, cout) + bias: pn2_mlp_pack + pn2_shared_mlp as one
// layer with no batch norm and no activation; bf16: pn2_mlp_pack_bf16 and PN2_MLP_BF16, so both
// operands are rounded to bf16 (the training layer's bf16 mode, include/pn2hip.h)
void linear_rows(const Tensor& in, const Tensor& w, const Tensor& bias, int64_t rows, Tensor& out,
                 const char* op, bool bf16 = false) {
  const int cin = I(w.size(0)), cout = I(w.size(1));
  const size_t bytes = bf16 ? pn2_mlp_packed_size_bf16(cin, cout) : pn2_mlp_packed_size(cin, cout);
  Tensor packed = workspace(in, bytes);
  check_rc((bf16 ? pn2_mlp_pack_bf16 : pn2_mlp_pack)(F(w), F(bias), nullptr, nullptr, cin, cout,
                                                     P(packed), bytes, stream_of(in)), op);
  const pn2_mlp_layer layer = {P(packed), cin, cout, bf16 ? PN2_MLP_BF16 : 0};
  // a row too wide for the fused kernel's LDS: the K-streamed kernel over the same pack (fp32
  // only; the bf16 ops keep raising for such a layer)
  int row_tiles = 0, tiles_per_wg = 0;
  if (!bf16 && pn2_shared_mlp_plan(rows, cin, 1, &layer, &row_tiles, &tiles_per_wg) == PN2_EINVAL) {
    check_rc(pn2_dense_wide(F(in), rows, cin, &layer, out.data_ptr<float>(), stream_of(in)), op);
    return;
  }
  check_rc(pn2_shared_mlp(F(in), rows, cin, 1, &layer, out.data_ptr<float>(), stream_of(in)), op);
}

// dense_wide: one packed fp32 layer (pn2_mlp_pack) over rows at any input width, inference:
// x (..., cin) -> (..., cout) on pn2_dense_wide (csrc/mlp_wide.hip)
Tensor dense_wide_hip(const Tensor& x_, const Tensor& packed_, int64_t cin, int64_t cout,
                      bool relu) {
  TORCH_CHECK_VALUE(cin > 0 && cout > 0 && cin <= INT_MAX && cout <= INT_MAX,
                    "dense_wide expects positive cin and cout");
  TORCH_CHECK_VALUE(x_.dim() >= 1 && x_.size(-1) == cin, "dense_wide expects (..., cin) x");
  const size_t bytes = pn2_mlp_packed_size(I(cin), I(cout));
  TORCH_CHECK_VALUE(packed_.dim() == 1 && static_cast<size_t>(packed_.numel()) * 4 >= bytes,
                    "dense_wide expects packed with the pn2_mlp_packed_size(cin, cout) bytes of "
                    "pn2_mlp_pack");
  Tensor x = dev(x_, "x", at::kFloat), packed = dev16(packed_, "packed", at::kFloat);
  Tensor out = at::empty(with_last(x, cout), f32(x));
  if (fake(x)) return out;
  c10::hip::HIPGuard g(x.device().index());
  const pn2_mlp_layer layer = {P(packed), I(cin), I(cout), relu ? PN2_MLP_RELU : 0};
  check_rc(pn2_dense_wide(F(x), x.numel() / cin, I(cin), &layer, out.data_ptr<float>(),
                          stream_of(x)), "dense_wide");
  return out;
}

// the last layer of a set-abstraction MLP fused with the max pool over nsample
// (pn2_bn_act_pool_fwd / _bwd): x (..., ns, cin) -> out, arg (..., cout); the (..., ns, cout)
// activation is never allocated
void chk_mlp_pool(const Tensor& x, const Tensor& weight, const std::optional<Tensor>& bias,
                  const std::optional<Tensor>& gamma, const std::optional<Tensor>& beta,
                  const char* name) {
  TORCH_CHECK_VALUE(x.dim() >= 2, name, " expects (..., ns, cin) x");
  chk_mlp_layer(x, weight, bias, gamma, beta, name);
  TORCH_CHECK_VALUE(x.size(-2) > 0, name, " expects at least one sample per group");
}
std::vector<int64_t> pooled_sizes(const Tensor& x, int64_t c) {
  std::vector<int64_t> s(x.sizes().begin(), x.sizes().end() - 2);
  s.push_back(c);
  return s;
}
void chk_mean_var(const std::optional<Tensor>& mean, const std::optional<Tensor>& var,
                  const std::optional<Tensor>& gamma, int64_t cout, const char* op) {
  if (has(gamma))
    TORCH_CHECK_VALUE(has(mean) && has(var) && mean->dim() == 1 && mean->size(0) == cout &&
                          var->dim() == 1 && var->size(0) == cout,
                      op, " expects (cout) mean and var with gamma and beta");
}
void chk_mlp_layer_grad(const Tensor& grad_out, const Tensor& x, const Tensor& weight,
                        const Tensor& y, const std::optional<Tensor>& mean,
                        const std::optional<Tensor>& var, const std::optional<Tensor>& gamma,
                        const std::optional<Tensor>& beta, const char* op) {
  chk_mlp_layer(x, weight, std::nullopt, gamma, beta, op);
  const int64_t cin = weight.size(0), cout = weight.size(1);
  TORCH_CHECK_VALUE(y.sizes() == grad_out.sizes() && y.dim() == x.dim() && y.size(-1) == cout &&
                        y.numel() / cout == x.numel() / cin,
                    op, " expects (..., cout) grad_out and y for (..., cin) x");
  chk_mean_var(mean, var, gamma, cout, op);
}
void chk_mlp_pool_grad(const Tensor& grad_out, const Tensor& arg, const Tensor& x,
                       const Tensor& weight, const Tensor& y, const std::optional<Tensor>& mean,
                       const std::optional<Tensor>& var, const std::optional<Tensor>& gamma,
                       const std::optional<Tensor>& beta, const char* op) {
  chk_mlp_pool(x, weight, std::nullopt, gamma, beta, op);
  const int64_t cout = weight.size(1);
  TORCH_CHECK_VALUE(y.sizes() == c10::IntArrayRef(with_last(x, cout)), op,
                    " expects (..., ns, cout) y for (..., ns, cin) x");
  TORCH_CHECK_VALUE(grad_out.sizes() == c10::IntArrayRef(pooled_sizes(x, cout)) &&
                        arg.sizes() == grad_out.sizes(),
                    op, " expects (..., cout) grad_out and arg for (..., ns, cin) x");
  chk_mean_var(mean, var, gamma, cout, op);
}

// an optional per-channel vector on the device; undefined (a null pointer under F) if absent
Tensor dev_opt(const std::optional<Tensor>& t, const char* name, bool wanted = true) {
  return wanted && has(t) ? dev(*t, name, at::kFloat) : Tensor();
}
// no rows, no statistics and no sums: defined values (tf_util.mlp_train skips its update)
bool no_rows(int64_t rows, std::initializer_list<Tensor*> zeroed) {
  if (rows != 0) return false;
  for (Tensor* t : zeroed) t->zero_();
  return true;
}
void bn_stats(const Tensor& y, int64_t rows, int C, Tensor& mean, Tensor& var, const char* op) {
  const size_t ws = pn2_bn_workspace_size(rows, C);
  Tensor w = workspace(y, ws);
  check_rc(pn2_bn_stats(F(y), rows, C, mean.data_ptr<float>(), var.data_ptr<float>(), P(w), ws,
                        stream_of(y)), op);
}
// pn2_bn_act_bwd, or with arg pn2_bn_act_pool_bwd over groups of ns rows; mean, var, gamma, beta
// and grad_gamma are undefined without batch norm
void bn_act_bwd(const Tensor& go, const Tensor* arg, const Tensor& y, int64_t rows, int64_t ns,
                int C, const Tensor& mean, const Tensor& var, const Tensor& gamma,
                const Tensor& beta, double eps, bool relu, Tensor& grad_y,
                const Tensor& grad_gamma, Tensor& grad_beta, const char* op) {
  const size_t ws = arg ? pn2_bn_pool_workspace_size(rows / ns, C) : pn2_bn_workspace_size(rows, C);
  Tensor w = workspace(y, ws);
  float* gg = grad_gamma.defined() ? grad_gamma.data_ptr<float>() : nullptr;
  const float e = static_cast<float>(eps);
  const int r = relu ? 1 : 0;
  check_rc(arg ? pn2_bn_act_pool_bwd(F(go), Ii(*arg), F(y), rows / ns, I(ns), C, F(mean), F(var),
                                     F(gamma), F(beta), e, r, grad_y.data_ptr<float>(), gg,
                                     grad_beta.data_ptr<float>(), P(w), ws, stream_of(y))
               : pn2_bn_act_bwd(F(go), F(y), rows, C, F(mean), F(var), F(gamma), F(beta), e, r,
                                grad_y.data_ptr<float>(), gg, grad_beta.data_ptr<float>(), P(w),
                                ws, stream_of(y)), op);
}
void wgrad(const Tensor& x, const Tensor& grad_y, int64_t rows, int cin, int cout, Tensor& grad_w,
           const char* op, bool bf16 = false) {
  const size_t ws = pn2_mlp_wgrad_workspace_size(rows, cin, cout);
  Tensor w = workspace(x, ws);
  check_rc((bf16 ? pn2_mlp_wgrad_bf16 : pn2_mlp_wgrad)(F(x), F(grad_y), rows, cin, cout,
                                                       grad_w.data_ptr<float>(), P(w), ws,
                                                       stream_of(x)), op);
}

// mlp_layer_train and, pooled, mlp_layer_train_pool: out, y, mean, var and (pooled) arg. bf16
// (the _bf16 ops): the layer's GEMM runs on the bf16 matrix cores, everything after y is the
// same fp32 code
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> mlp_train_fwd(
    const Tensor& x_, const Tensor& weight_, const std::optional<Tensor>& bias_,
    const std::optional<Tensor>& gamma_, const std::optional<Tensor>& beta_, double eps, bool relu,
    bool pooled, const char* op, bool bf16 = false) {
  (pooled ? chk_mlp_pool : chk_mlp_layer)(x_, weight_, bias_, gamma_, beta_, op);
  Tensor x = dev(x_, "x", at::kFloat), weight = dev(weight_, "weight", at::kFloat);
  Tensor bias = dev_opt(bias_, "bias"), gamma = dev_opt(gamma_, "gamma");
  Tensor beta = dev_opt(beta_, "beta");
  const bool bn = gamma.defined();
  const int cin = I(weight.size(0)), cout = I(weight.size(1));
  const int64_t rows = x.numel() / cin;
  const std::vector<int64_t> out_sizes = pooled ? pooled_sizes(x, cout) : with_last(x, cout);
  Tensor out = at::empty(out_sizes, f32(x)), arg;
  if (pooled) arg = at::empty(out_sizes, i32(x));
  Tensor y = at::empty(with_last(x, cout), f32(x));
  Tensor mean = at::empty({bn ? cout : 0}, f32(x)), var = at::empty({bn ? cout : 0}, f32(x));
  if (fake(x)) return {out, y, mean, var, arg};
  c10::hip::HIPGuard g(x.device().index());
  if (no_rows(rows, {&mean, &var})) return {out, y, mean, var, arg};
  linear_rows(x, weight, bias, rows, y, op, bf16);
  if (bn) bn_stats(y, rows, cout, mean, var, op);
  const float* m = bn ? F(mean) : nullptr;
  const float* v = bn ? F(var) : nullptr;
  const float e = static_cast<float>(eps);
  if (pooled) {
    const int64_t ns = x.size(-2);
    check_rc(pn2_bn_act_pool_fwd(F(y), rows / ns, I(ns), cout, m, v, F(gamma), F(beta), e,
                                 relu ? 1 : 0, out.data_ptr<float>(), arg.data_ptr<int32_t>(),
                                 stream_of(x)), op);
  } else {
    check_rc(pn2_bn_act_fwd(F(y), rows, cout, m, v, F(gamma), F(beta), e, relu ? 1 : 0,
                            out.data_ptr<float>(), stream_of(x)), op);
  }
  return {out, y, mean, var, arg};
}

// mlp_layer_train_grad and, with arg, mlp_layer_train_pool_grad (grad_out is then (..., cout)).
// bf16 (the _bf16 ops): the two GEMMs on the fp32 grad_y run on the bf16 matrix cores
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> mlp_train_bwd(
    const Tensor& grad_out_, const Tensor* arg_, const Tensor& x_, const Tensor& weight_,
    const Tensor& y_, const std::optional<Tensor>& mean_, const std::optional<Tensor>& var_,
    const std::optional<Tensor>& gamma_, const std::optional<Tensor>& beta_, double eps, bool relu,
    bool need_grad_x, const char* op, bool bf16 = false) {
  if (arg_) chk_mlp_pool_grad(grad_out_, *arg_, x_, weight_, y_, mean_, var_, gamma_, beta_, op);
  else chk_mlp_layer_grad(grad_out_, x_, weight_, y_, mean_, var_, gamma_, beta_, op);
  const bool bn = has(gamma_);
  Tensor go = dev(grad_out_, "grad_out", at::kFloat), arg;
  if (arg_) arg = dev(*arg_, "arg", at::kInt);
  Tensor x = dev(x_, "x", at::kFloat), weight = dev(weight_, "weight", at::kFloat);
  Tensor y = dev(y_, "y", at::kFloat);
  Tensor mean = dev_opt(mean_, "mean", bn), var = dev_opt(var_, "var", bn);
  Tensor gamma = dev_opt(gamma_, "gamma"), beta = dev_opt(beta_, "beta");
  const int cin = I(weight.size(0)), cout = I(weight.size(1));
  const int64_t rows = x.numel() / cin;
  Tensor grad_x = need_grad_x ? at::empty(x.sizes(), f32(x)) : at::empty({0}, f32(x));
  Tensor grad_w = at::empty({cin, cout}, f32(x));
  // under batch norm the bias shifts the batch mean with it: its gradient is identically zero
  Tensor grad_b = bn ? at::zeros({cout}, f32(x)) : at::empty({cout}, f32(x));
  Tensor grad_gamma = at::empty({bn ? cout : 0}, f32(x));
  Tensor grad_beta = at::empty({bn ? cout : 0}, f32(x));
  if (fake(x)) return {grad_x, grad_w, grad_b, grad_gamma, grad_beta};
  c10::hip::HIPGuard g(x.device().index());
  if (no_rows(rows, {&grad_w, &grad_b, &grad_gamma, &grad_beta}))
    return {grad_x, grad_w, grad_b, grad_gamma, grad_beta};
  Tensor grad_y = at::empty(y.sizes(), f32(x));
  bn_act_bwd(go, arg_ ? &arg : nullptr, y, rows, arg_ ? x.size(-2) : 1, cout, mean, var, gamma,
             beta, eps, relu, grad_y, bn ? grad_gamma : Tensor(), bn ? grad_beta : grad_b, op);
  wgrad(x, grad_y, rows, cin, cout, grad_w, op, bf16);
  if (need_grad_x) linear_rows(grad_y, weight.t().contiguous(), Tensor(), rows, grad_x, op, bf16);
  return {grad_x, grad_w, grad_b, grad_gamma, grad_beta};
}

// the fp32 ops and their _bf16 namesakes (the training layer's bf16 mode): the same bodies
template <bool BF16>
std::tuple<Tensor, Tensor, Tensor, Tensor> mlp_layer_train_hip(
    const Tensor& x, const Tensor& weight, const std::optional<Tensor>& bias,
    const std::optional<Tensor>& gamma, const std::optional<Tensor>& beta, double eps, bool relu) {
  auto [out, y, mean, var, arg] =
      mlp_train_fwd(x, weight, bias, gamma, beta, eps, relu, false,
                    BF16 ? "mlp_layer_train_bf16" : "mlp_layer_train", BF16);
  return {out, y, mean, var};
}
template <bool BF16>
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> mlp_layer_train_pool_hip(
    const Tensor& x, const Tensor& weight, const std::optional<Tensor>& bias,
    const std::optional<Tensor>& gamma, const std::optional<Tensor>& beta, double eps, bool relu) {
  return mlp_train_fwd(x, weight, bias, gamma, beta, eps, relu, true,
                       BF16 ? "mlp_layer_train_pool_bf16" : "mlp_layer_train_pool", BF16);
}
template <bool BF16>
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> mlp_layer_train_grad_hip(
    const Tensor& grad_out, const Tensor& x, const Tensor& weight, const Tensor& y,
    const std::optional<Tensor>& mean, const std::optional<Tensor>& var,
    const std::optional<Tensor>& gamma, const std::optional<Tensor>& beta, double eps, bool relu,
    bool need_grad_x) {
  return mlp_train_bwd(grad_out, nullptr, x, weight, y, mean, var, gamma, beta, eps, relu,
                       need_grad_x, BF16 ? "mlp_layer_train_bf16_grad" : "mlp_layer_train_grad",
                       BF16);
}
template <bool BF16>
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> mlp_layer_train_pool_grad_hip(
    const Tensor& grad_out, const Tensor& arg, const Tensor& x, const Tensor& weight,
    const Tensor& y, const std::optional<Tensor>& mean, const std::optional<Tensor>& var,
    const std::optional<Tensor>& gamma, const std::optional<Tensor>& beta, double eps, bool relu,
    bool need_grad_x) {
  return mlp_train_bwd(grad_out, &arg, x, weight, y, mean, var, gamma, beta, eps, relu,
                       need_grad_x,
                       BF16 ? "mlp_layer_train_pool_bf16_grad" : "mlp_layer_train_pool_grad", BF16);
}

// ---- training-mode AttentionLayer of the attention SA modules (csrc/attn_train.hip;
// attention_layer.py:10-45 as instantiated at :256-259): the Dense query of each group's first
// row, K and V projected together into one (..., ns, 2C) tensor, the reduction on that layout
// and, with add_max, the max over ns of x with its arg (the _and_pooling module, :303)
void chk_attn_kv(const Tensor& x, const Tensor& wq, const Tensor& wk, const Tensor& wv,
                 const char* op) {
  TORCH_CHECK_VALUE(x.dim() >= 2 && x.size(-2) > 0 && x.size(-1) > 0 && x.size(-1) % 4 == 0, op,
                    " expects (..., ns, C) x with ns > 0 and C % 4 == 0 (key_dim 4)");
  const int64_t C = x.size(-1);
  for (const Tensor* w : {&wq, &wk, &wv})
    TORCH_CHECK_VALUE(w->dim() == 2 && w->size(0) == C && w->size(1) == C, op,
                      " expects (C, C) wq, wk and wv for (..., ns, C) x");
}
void chk_attn_kv_bias(const Tensor& x, const Tensor& bq, const Tensor& bk, const Tensor& bv,
                      const char* op) {
  for (const Tensor* b : {&bq, &bk, &bv})
    TORCH_CHECK_VALUE(b->dim() == 1 && b->size(0) == x.size(-1), op,
                      " expects (C) bq, bk and bv for (..., ns, C) x");
}
void chk_attn_kv_grad(const Tensor& grad_att, const std::optional<Tensor>& grad_pmax,
                      const Tensor& arg, const Tensor& x, const Tensor& wq, const Tensor& wk,
                      const Tensor& wv, const Tensor& q, const Tensor& kv, const char* op) {
  chk_attn_kv(x, wq, wk, wv, op);
  const int64_t C = x.size(-1);
  const std::vector<int64_t> pooled = pooled_sizes(x, C);
  TORCH_CHECK_VALUE(grad_att.sizes() == c10::IntArrayRef(pooled) && q.sizes() == grad_att.sizes(),
                    op, " expects (..., C) grad_att and q for (..., ns, C) x");
  TORCH_CHECK_VALUE(kv.sizes() == c10::IntArrayRef(with_last(x, 2 * C)), op,
                    " expects (..., ns, 2C) kv for (..., ns, C) x");
  if (has(grad_pmax))
    TORCH_CHECK_VALUE(grad_pmax->sizes() == c10::IntArrayRef(pooled) &&
                          arg.sizes() == grad_pmax->sizes(),
                      op, " expects (..., C) grad_pmax and arg for (..., ns, C) x");
}

void col_sum(const Tensor& x, int64_t rows, int C, Tensor& out, const char* op) {
  const size_t ws = pn2_col_sum_workspace_size(rows, C);
  Tensor w = workspace(x, ws);
  check_rc(pn2_col_sum(F(x), rows, C, out.data_ptr<float>(), P(w), ws, stream_of(x)), op);
}

std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> attn_kv_train_hip(
    const Tensor& x_, const Tensor& wq_, const Tensor& bq_, const Tensor& wk_, const Tensor& bk_,
    const Tensor& wv_, const Tensor& bv_, bool add_max) {
  const char* op = "attn_kv_train";
  chk_attn_kv(x_, wq_, wk_, wv_, op);
  chk_attn_kv_bias(x_, bq_, bk_, bv_, op);
  Tensor x = dev(x_, "x", at::kFloat);
  Tensor wq = dev(wq_, "wq", at::kFloat), bq = dev(bq_, "bq", at::kFloat);
  Tensor wk = dev(wk_, "wk", at::kFloat), bk = dev(bk_, "bk", at::kFloat);
  Tensor wv = dev(wv_, "wv", at::kFloat), bv = dev(bv_, "bv", at::kFloat);
  const int C = I(x.size(-1)), ns = I(x.size(-2));
  const int64_t rows = x.numel() / C, G = rows / ns;
  const std::vector<int64_t> pooled = pooled_sizes(x, C);
  Tensor att = at::empty(pooled, f32(x)), q = at::empty(pooled, f32(x));
  Tensor kv = at::empty(with_last(x, 2 * C), f32(x));
  Tensor pmax = add_max ? at::empty(pooled, f32(x)) : at::empty({0}, f32(x));
  Tensor arg = add_max ? at::empty(pooled, i32(x)) : at::empty({0}, i32(x));
  if (fake(x) || G == 0) return {att, pmax, arg, q, kv};
  c10::hip::HIPGuard g(x.device().index());
  // the query is the group's first row (attention_layer.py:259): G rows
  linear_rows(x.select(-2, 0).contiguous(), wq, bq, G, q, op);
  // [K | V] = x [wk | wv] + [bk | bv]: one GEMM, x read once
  linear_rows(x, at::cat({wk, wv}, 1), at::cat({bk, bv}, 0), rows, kv, op);
  check_rc(pn2_attn_kv_reduce(F(q), F(kv), G, ns, C, att.data_ptr<float>(), stream_of(x)), op);
  if (add_max)  // no batch norm, no ReLU: the plain max over ns, arg = the lowest j
    check_rc(pn2_bn_act_pool_fwd(F(x), G, ns, C, nullptr, nullptr, nullptr, nullptr, 0.f, 0,
                                 pmax.data_ptr<float>(), arg.data_ptr<int32_t>(), stream_of(x)),
             op);
  return {att, pmax, arg, q, kv};
}

std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor> attn_kv_train_grad_hip(
    const Tensor& grad_att_, const std::optional<Tensor>& grad_pmax_, const Tensor& arg_,
    const Tensor& x_, const Tensor& wq_, const Tensor& wk_, const Tensor& wv_, const Tensor& q_,
    const Tensor& kv_, bool need_grad_x) {
  const char* op = "attn_kv_train_grad";
  chk_attn_kv_grad(grad_att_, grad_pmax_, arg_, x_, wq_, wk_, wv_, q_, kv_, op);
  Tensor go = dev16(grad_att_, "grad_att", at::kFloat), x = dev(x_, "x", at::kFloat);
  Tensor wq = dev(wq_, "wq", at::kFloat), wk = dev(wk_, "wk", at::kFloat);
  Tensor wv = dev(wv_, "wv", at::kFloat), q = dev16(q_, "q", at::kFloat);
  Tensor kv = dev16(kv_, "kv", at::kFloat);
  Tensor gp, arg;
  if (has(grad_pmax_)) {
    gp = dev(*grad_pmax_, "grad_pmax", at::kFloat);
    arg = dev(arg_, "arg", at::kInt);
  }
  const int C = I(x.size(-1)), ns = I(x.size(-2));
  const int64_t rows = x.numel() / C, G = rows / ns;
  Tensor grad_x = need_grad_x ? at::empty(x.sizes(), f32(x)) : at::empty({0}, f32(x));
  Tensor grad_wq = at::empty({C, C}, f32(x)), grad_bq = at::empty({C}, f32(x));
  if (fake(x))  // the k and v gradients are slices of joint ones below: (C, C) and (C) again
    return {grad_x, grad_wq, grad_bq, at::empty_like(grad_wq), at::empty_like(grad_bq),
            at::empty_like(grad_wq), at::empty_like(grad_bq)};
  c10::hip::HIPGuard g(x.device().index());
  if (G == 0) {
    grad_wq.zero_();
    grad_bq.zero_();
    return {grad_x, grad_wq, grad_bq, at::zeros({C, C}, f32(x)), at::zeros({C}, f32(x)),
            at::zeros({C, C}, f32(x)), at::zeros({C}, f32(x))};
  }
  Tensor grad_q = at::empty(q.sizes(), f32(x)), grad_kv = at::empty(kv.sizes(), f32(x));
  check_rc(pn2_attn_kv_reduce_grad(F(q), F(kv), F(go), G, ns, C, grad_q.data_ptr<float>(),
                                   grad_kv.data_ptr<float>(), stream_of(x)), op);
  // [grad_wk | grad_wv] = x^T grad_kv: one weight-gradient GEMM; grad_wq over the G query rows
  Tensor grad_wkv = at::empty({C, 2 * C}, f32(x)), grad_bkv = at::empty({2 * C}, f32(x));
  wgrad(x, grad_kv, rows, C, 2 * C, grad_wkv, op);
  wgrad(x.select(-2, 0).contiguous(), grad_q, G, C, C, grad_wq, op);
  col_sum(grad_kv, rows, 2 * C, grad_bkv, op);
  col_sum(grad_q, G, C, grad_bq, op);
  if (need_grad_x) {
    // grad_x = grad_kv [wk | wv]^T, written once, then patched at 2 G C elements
    linear_rows(grad_kv, at::cat({wk, wv}, 1).t().contiguous(), Tensor(), rows, grad_x, op);
    Tensor grad_xq = at::empty(q.sizes(), f32(x));
    linear_rows(grad_q, wq.t().contiguous(), Tensor(), G, grad_xq, op);
    check_rc(pn2_attn_dx_scatter(grad_x.data_ptr<float>(), F(grad_xq), F(gp),
                                 gp.defined() ? Ii(arg) : nullptr, G, ns, C, stream_of(x)), op);
  }
  return {grad_x, grad_wq, grad_bq,
          grad_wkv.slice(1, 0, C).contiguous(), grad_bkv.slice(0, 0, C).clone(),
          grad_wkv.slice(1, C, 2 * C).contiguous(), grad_bkv.slice(0, C, 2 * C).clone()};
}

// ---- batch-statistics batch norm on its own (the batch norm after the attention,
// attention_layer.py:261): pn2_bn_stats + pn2_bn_act_fwd, pn2_bn_act_bwd on x (..., C)
void chk_bn(const Tensor& x, const Tensor& gamma, const Tensor& beta, const char* op) {
  TORCH_CHECK_VALUE(x.dim() >= 1 && x.size(-1) > 0, op, " expects (..., C) x");
  TORCH_CHECK_VALUE(gamma.dim() == 1 && gamma.size(0) == x.size(-1) && beta.dim() == 1 &&
                        beta.size(0) == x.size(-1),
                    op, " expects (C) gamma and beta for (..., C) x");
}

std::tuple<Tensor, Tensor, Tensor> bn_train_hip(const Tensor& x_, const Tensor& gamma_,
                                                const Tensor& beta_, double eps, bool relu) {
  const char* op = "bn_train";
  chk_bn(x_, gamma_, beta_, op);
  Tensor x = dev(x_, "x", at::kFloat), gamma = dev(gamma_, "gamma", at::kFloat);
  Tensor beta = dev(beta_, "beta", at::kFloat);
  const int C = I(x.size(-1));
  const int64_t rows = x.numel() / C;
  Tensor out = at::empty(x.sizes(), f32(x));
  Tensor mean = at::empty({C}, f32(x)), var = at::empty({C}, f32(x));
  if (fake(x)) return {out, mean, var};
  c10::hip::HIPGuard g(x.device().index());
  if (no_rows(rows, {&mean, &var})) return {out, mean, var};
  bn_stats(x, rows, C, mean, var, op);
  check_rc(pn2_bn_act_fwd(F(x), rows, C, F(mean), F(var), F(gamma), F(beta),
                          static_cast<float>(eps), relu ? 1 : 0, out.data_ptr<float>(),
                          stream_of(x)), op);
  return {out, mean, var};
}

std::tuple<Tensor, Tensor, Tensor> bn_train_grad_hip(const Tensor& grad_out_, const Tensor& x_,
                                                     const Tensor& mean_, const Tensor& var_,
                                                     const Tensor& gamma_, const Tensor& beta_,
                                                     double eps, bool relu) {
  const char* op = "bn_train_grad";
  chk_bn(x_, gamma_, beta_, op);
  TORCH_CHECK_VALUE(grad_out_.sizes() == x_.sizes(), op, " expects grad_out shaped like x");
  TORCH_CHECK_VALUE(mean_.sizes() == gamma_.sizes() && var_.sizes() == gamma_.sizes(), op,
                    " expects (C) mean and var");
  Tensor go = dev(grad_out_, "grad_out", at::kFloat), x = dev(x_, "x", at::kFloat);
  Tensor mean = dev(mean_, "mean", at::kFloat), var = dev(var_, "var", at::kFloat);
  Tensor gamma = dev(gamma_, "gamma", at::kFloat), beta = dev(beta_, "beta", at::kFloat);
  const int C = I(x.size(-1));
  const int64_t rows = x.numel() / C;
  Tensor grad_x = at::empty(x.sizes(), f32(x));
  Tensor grad_gamma = at::empty({C}, f32(x)), grad_beta = at::empty({C}, f32(x));
  if (fake(x)) return {grad_x, grad_gamma, grad_beta};
  c10::hip::HIPGuard g(x.device().index());
  if (no_rows(rows, {&grad_gamma, &grad_beta})) return {grad_x, grad_gamma, grad_beta};
  bn_act_bwd(go, nullptr, x, rows, 1, C, mean, var, gamma, beta, eps, relu, grad_x, grad_gamma,
             grad_beta, op);
  return {grad_x, grad_gamma, grad_beta};
}

// ---- training-mode segmentation head (csrc/head_train.hip): tf_util.dropout with is_training
// (tf_util.py:594-612) and get_loss's weighted sparse softmax cross-entropy
// (pointnet2_sem_seg.py:62-69, tf.losses' SUM_BY_NONZERO_WEIGHTS)
void chk_dropout(const Tensor& x, double keep_prob) {
  TORCH_CHECK_VALUE(keep_prob > 0.0 && keep_prob <= 1.0 && static_cast<float>(keep_prob) > 0.f,
                    "dropout expects keep_prob in (0, 1], got ", keep_prob);
  TORCH_CHECK_VALUE(x.scalar_type() == at::kFloat, "dropout expects a float32 x, got ",
                    x.scalar_type());
}
// logits (..., C), labels (...) int32, weights (...) float32 or absent
void chk_xent(const Tensor& logits, const Tensor& labels, const std::optional<Tensor>& weights,
              const char* op) {
  TORCH_CHECK_VALUE(logits.dim() >= 1 && logits.size(-1) > 0 && logits.size(-1) <= 65535, op,
                    " expects (..., C) logits with 0 < C <= 65535");
  TORCH_CHECK_VALUE(logits.scalar_type() == at::kFloat, op, " expects float32 logits, got ",
                    logits.scalar_type());
  TORCH_CHECK_VALUE(labels.scalar_type() == at::kInt, op, " expects int32 labels, got ",
                    labels.scalar_type());
  const c10::IntArrayRef lead = logits.sizes().slice(0, logits.dim() - 1);
  TORCH_CHECK_VALUE(labels.sizes() == lead, op, " expects labels shaped like logits without its ",
                    "last axis: logits ", logits.sizes(), ", labels ", labels.sizes());
  if (has(weights)) {
    TORCH_CHECK_VALUE(weights->scalar_type() == at::kFloat, op, " expects float32 weights, got ",
                      weights->scalar_type());
    TORCH_CHECK_VALUE(weights->sizes() == lead, op, " expects weights shaped like labels: labels ",
                      labels.sizes(), ", weights ", weights->sizes());
  }
}
void chk_xent_grad(const Tensor& grad_loss, const Tensor& logits, const Tensor& labels,
                   const std::optional<Tensor>& weights, const Tensor& lse,
                   const Tensor& num_present, const char* op) {
  chk_xent(logits, labels, weights, op);
  TORCH_CHECK_VALUE(grad_loss.numel() == 1 && grad_loss.scalar_type() == at::kFloat, op,
                    " expects a float32 scalar grad_loss");
  TORCH_CHECK_VALUE(lse.sizes() == labels.sizes() && lse.scalar_type() == at::kFloat, op,
                    " expects float32 lse shaped like labels");
  TORCH_CHECK_VALUE(num_present.numel() == 1 && num_present.scalar_type() == at::kInt, op,
                    " expects an int32 scalar num_present");
}

Tensor dropout_hip(const Tensor& x_, double keep_prob, int64_t seed) {
  chk_dropout(x_, keep_prob);
  Tensor x = dev(x_, "x", at::kFloat);
  Tensor out = at::empty(x.sizes(), f32(x));
  if (fake(x) || x.numel() == 0) return out;
  c10::hip::HIPGuard g(x.device().index());
  check_rc(pn2_dropout(F(x), x.numel(), static_cast<float>(keep_prob),
                       static_cast<uint64_t>(seed), out.data_ptr<float>(), stream_of(x)),
           "dropout");
  return out;
}

std::tuple<Tensor, Tensor, Tensor, Tensor> softmax_xent_hip(const Tensor& logits_,
                                                            const Tensor& labels_,
                                                            const std::optional<Tensor>& weights_) {
  const char* op = "softmax_xent";
  chk_xent(logits_, labels_, weights_, op);
  Tensor logits = dev(logits_, "logits", at::kFloat), labels = dev(labels_, "labels", at::kInt);
  Tensor weights;
  if (has(weights_)) weights = dev(*weights_, "weights", at::kFloat);
  const int C = I(logits.size(-1));
  const int64_t rows = labels.numel();
  Tensor lse = at::empty(labels.sizes(), f32(logits));
  Tensor pred = at::empty(labels.sizes(), i32(logits));
  Tensor loss = at::empty({}, f32(logits)), num_present = at::empty({}, i32(logits));
  if (fake(logits)) return {loss, lse, pred, num_present};
  c10::hip::HIPGuard g(logits.device().index());
  if (rows == 0)  // no rows: TF's safe division gives 0
    return {loss.zero_(), lse, pred, num_present.zero_()};
  const size_t ws = pn2_softmax_xent_workspace_size(rows);
  Tensor w = workspace(logits, ws);
  check_rc(pn2_softmax_xent_fwd(F(logits), Ii(labels), F(weights), rows, C, lse.data_ptr<float>(),
                                pred.data_ptr<int32_t>(), loss.data_ptr<float>(),
                                num_present.data_ptr<int32_t>(), P(w), ws, stream_of(logits)), op);
  return {loss, lse, pred, num_present};
}

Tensor softmax_xent_grad_hip(const Tensor& grad_loss_, const Tensor& logits_, const Tensor& labels_,
                             const std::optional<Tensor>& weights_, const Tensor& lse_,
                             const Tensor& num_present_) {
  const char* op = "softmax_xent_grad";
  chk_xent_grad(grad_loss_, logits_, labels_, weights_, lse_, num_present_, op);
  Tensor gl = dev(grad_loss_, "grad_loss", at::kFloat);
  Tensor logits = dev(logits_, "logits", at::kFloat), labels = dev(labels_, "labels", at::kInt);
  Tensor lse = dev(lse_, "lse", at::kFloat), np = dev(num_present_, "num_present", at::kInt);
  Tensor weights;
  if (has(weights_)) weights = dev(*weights_, "weights", at::kFloat);
  Tensor grad = at::empty(logits.sizes(), f32(logits));
  const int64_t rows = labels.numel();
  if (fake(logits) || rows == 0) return grad;
  c10::hip::HIPGuard g(logits.device().index());
  check_rc(pn2_softmax_xent_bwd(F(gl), F(logits), Ii(labels), F(weights), F(lse), Ii(np), rows,
                                I(logits.size(-1)), grad.data_ptr<float>(), stream_of(logits)), op);
  return grad;
}

// ---- optimiser and metrics (csrc/optim.hip): tf.train.AdamOptimizer's ApplyAdam over every
// variable in ceil(n / PN2_ADAM_SLOTS) launches, get_metrics' confusion matrix and counts, and
// tf.metrics.mean_iou's value (attention_points/train.py:145-163, :337). None is differentiable.
void chk_adam(at::TensorList params, at::TensorList grads, at::TensorList exp_avg,
              at::TensorList exp_avg_sq) {
  const size_t n = params.size();
  TORCH_CHECK_VALUE(grads.size() == n && exp_avg.size() == n && exp_avg_sq.size() == n,
                    "adam_step expects four lists of one length, got ", n, ", ", grads.size(), ", ",
                    exp_avg.size(), ", ", exp_avg_sq.size());
  for (size_t i = 0; i < n; ++i) {
    const Tensor* t[4] = {&params[i], &grads[i], &exp_avg[i], &exp_avg_sq[i]};
    const char* name[4] = {"params", "grads", "exp_avg", "exp_avg_sq"};
    for (int k = 0; k < 4; ++k) {
      TORCH_CHECK_VALUE(t[k]->scalar_type() == at::kFloat, "adam_step expects float32 tensors, got ",
                        t[k]->scalar_type(), " in ", name[k], "[", i, "]");
      TORCH_CHECK_VALUE(t[k]->is_contiguous(), "adam_step expects contiguous tensors: ", name[k],
                        "[", i, "] is not");
      TORCH_CHECK_VALUE(t[k]->numel() == params[i].numel(), "adam_step expects ", name[k], "[", i,
                        "] with the ", params[i].numel(), " elements of params[", i, "], got ",
                        t[k]->numel());
      TORCH_CHECK_VALUE(t[k]->device() == params[0].device(),
                        "adam_step expects every tensor on one device: ", name[k], "[", i,
                        "] is on ", t[k]->device(), ", params[0] on ", params[0].device());
    }
  }
}
int64_t chk_confusion(const Tensor& confusion, const char* op) {
  TORCH_CHECK_VALUE(confusion.scalar_type() == at::kLong && confusion.dim() == 2 &&
                        confusion.size(0) == confusion.size(1) && confusion.size(0) > 0 &&
                        confusion.size(0) <= PN2_METRICS_MAX_C && confusion.is_contiguous(),
                    op, " expects a contiguous int64 (C, C) confusion with 0 < C <= ",
                    PN2_METRICS_MAX_C, ", got ", confusion.scalar_type(), " ", confusion.sizes());
  return confusion.size(0);
}
void chk_seg_confusion(const Tensor& labels, const Tensor& pred, const Tensor& confusion,
                       const Tensor& counts) {
  const char* op = "seg_confusion";
  TORCH_CHECK_VALUE(labels.scalar_type() == at::kInt && pred.scalar_type() == at::kInt, op,
                    " expects int32 labels and pred, got ", labels.scalar_type(), " and ",
                    pred.scalar_type());
  TORCH_CHECK_VALUE(labels.sizes() == pred.sizes(), op, " expects labels and pred of one shape: ",
                    "labels ", labels.sizes(), ", pred ", pred.sizes());
  chk_confusion(confusion, op);
  TORCH_CHECK_VALUE(counts.scalar_type() == at::kLong && counts.dim() == 1 && counts.size(0) == 2 &&
                        counts.is_contiguous(),
                    op, " expects int64 (2,) counts, got ", counts.scalar_type(), " ",
                    counts.sizes());
  TORCH_CHECK_VALUE(pred.device() == labels.device() && confusion.device() == labels.device() &&
                        counts.device() == labels.device(),
                    op, " expects every tensor on one device");
}

// the mutated tensors' in-place version counters advance, as for torch's own in-place ops
// (tf_util.ParamStore.stamp keys the packed inference layers on them)
void bump(const Tensor& t) { t.unsafeGetTensorImpl()->bump_version(); }

void adam_step_hip(at::TensorList params, at::TensorList grads, at::TensorList exp_avg,
                   at::TensorList exp_avg_sq, double alpha, double beta1, double beta2,
                   double epsilon) {
  chk_adam(params, grads, exp_avg, exp_avg_sq);
  if (params.empty() || fake(params[0])) return;  // (chk_adam: all on params[0]'s device)
  std::vector<pn2_adam_slot> slots(params.size());
  for (size_t i = 0; i < params.size(); ++i) {
    TORCH_CHECK(params[i].is_cuda(), "params[", i, "] is on ", params[i].device(),
                ": pn2hip ops run on the MI355X only (no CPU fallback)");
    slots[i] = {params[i].data_ptr<float>(), grads[i].data_ptr<float>(),
                exp_avg[i].data_ptr<float>(), exp_avg_sq[i].data_ptr<float>(), params[i].numel()};
  }
  c10::hip::HIPGuard g(params[0].device().index());
  check_rc(pn2_adam_step(slots.data(), I(static_cast<int64_t>(slots.size())),
                         static_cast<float>(alpha), static_cast<float>(beta1),
                         static_cast<float>(beta2), static_cast<float>(epsilon),
                         stream_of(params[0])), "adam_step");
  for (size_t i = 0; i < params.size(); ++i) {
    bump(params[i]);
    bump(exp_avg[i]);
    bump(exp_avg_sq[i]);
  }
}

void seg_confusion_hip(const Tensor& labels_, const Tensor& pred_, const Tensor& confusion,
                       const Tensor& counts) {
  chk_seg_confusion(labels_, pred_, confusion, counts);
  Tensor labels = dev(labels_, "labels", at::kInt), pred = dev(pred_, "pred", at::kInt);
  if (fake(labels)) return;
  c10::hip::HIPGuard g(labels.device().index());
  check_rc(pn2_seg_confusion(Ii(labels), Ii(pred), labels.numel(), I(confusion.size(0)),
                             reinterpret_cast<long long*>(confusion.data_ptr<int64_t>()),
                             reinterpret_cast<long long*>(counts.data_ptr<int64_t>()),
                             stream_of(labels)), "seg_confusion");
  bump(confusion);
  bump(counts);
}

std::tuple<Tensor, Tensor> mean_iou_hip(const Tensor& confusion) {
  const int64_t C = chk_confusion(confusion, "mean_iou");
  TORCH_CHECK(confusion.is_cuda() || fake(confusion), "confusion is on ", confusion.device(),
              ": pn2hip ops run on the MI355X only (no CPU fallback)");
  Tensor iou = at::empty({}, f32(confusion)), per_class = at::empty({C}, f32(confusion));
  if (fake(confusion)) return {iou, per_class};
  c10::hip::HIPGuard g(confusion.device().index());
  check_rc(pn2_mean_iou(reinterpret_cast<const long long*>(confusion.data_ptr<int64_t>()), I(C),
                        iou.data_ptr<float>(), per_class.data_ptr<float>(), stream_of(confusion)),
           "mean_iou");
  return {iou, per_class};
}

// ---- whole-scene prediction (csrc/predict.hip): the argmax + map_back of
// attention_points/benchmark/generate_predictions.py as a 64-bit atomic max per scene point, and
// the label look-ups of map_to_nyu40, label_map and benchmark/evaluate.py. These four ops have
// CPU kernels too (the host twins of csrc/cpu_predict.cpp: equal bits), so the path from chunk
// rows to a score runs and is tested without a GPU. `keys` is int64; the kernels read its bits
// as unsigned (they stay below 2^63).
const long long* KeysC(const Tensor& t) { return reinterpret_cast<const long long*>(t.data_ptr<int64_t>()); }
long long* Keys(const Tensor& t) { return reinterpret_cast<long long*>(t.data_ptr<int64_t>()); }

void chk_keys(const Tensor& keys, const char* op) {
  TORCH_CHECK_VALUE(keys.scalar_type() == at::kLong && keys.dim() == 1 && keys.is_contiguous(), op,
                    " expects contiguous int64 (n_scene,) keys, got ", keys.scalar_type(), " ",
                    keys.sizes());
}
bool is_byte(const Tensor& t) { return t.scalar_type() == at::kByte || t.scalar_type() == at::kBool; }
void chk_scene_vote(const std::optional<Tensor>& logits, const Tensor& mask, const Tensor& orig,
                    int64_t row0, const Tensor& keys) {
  const char* op = "scene_vote";
  TORCH_CHECK_VALUE(is_byte(mask) && orig.scalar_type() == at::kInt, op,
                    " expects uint8 or bool mask and int32 orig, got ", mask.scalar_type(), " and ",
                    orig.scalar_type());
  TORCH_CHECK_VALUE(mask.sizes() == orig.sizes(), op, " expects mask and orig of one shape: mask ",
                    mask.sizes(), ", orig ", orig.sizes());
  chk_keys(keys, op);
  TORCH_CHECK_VALUE(row0 >= 0, op, " expects row0 >= 0, got ", row0);
  TORCH_CHECK_VALUE(orig.device() == mask.device() && keys.device() == mask.device(), op,
                    " expects every tensor on one device");
  if (logits.has_value()) {
    const Tensor& l = *logits;
    TORCH_CHECK_VALUE(l.scalar_type() == at::kFloat && l.dim() >= 1 && l.size(-1) >= 1 &&
                          l.size(-1) <= (1 << PN2_VOTE_LABEL_BITS) &&
                          l.numel() == mask.numel() * l.size(-1),
                      op, " expects float32 logits (rows, C) with 1 <= C <= ",
                      (1 << PN2_VOTE_LABEL_BITS), " and mask's ", mask.numel(), " rows, got ",
                      l.scalar_type(), " ", l.sizes());
    TORCH_CHECK_VALUE(l.device() == mask.device(), op, " expects every tensor on one device");
  }
}
void chk_lut(const Tensor& lut, const Tensor& like, const char* op) {
  TORCH_CHECK_VALUE(lut.scalar_type() == at::kInt && lut.dim() == 1, op,
                    " expects an int32 (nlut,) lut, got ", lut.scalar_type(), " ", lut.sizes());
  TORCH_CHECK_VALUE(lut.device() == like.device(), op, " expects every tensor on one device");
}
void chk_i32_dflt(int64_t dflt, const char* op) {
  TORCH_CHECK_VALUE(dflt >= INT32_MIN && dflt <= INT32_MAX, op, " expects an int32 dflt, got ", dflt);
}
// bytes of one row of values (rows, ...) / out (n_scene, ...)
int64_t chk_map_back(const Tensor& values, int64_t row0, const Tensor& keys, const Tensor& out) {
  const char* op = "map_back_rows";
  chk_keys(keys, op);
  TORCH_CHECK_VALUE(row0 >= 0, op, " expects row0 >= 0, got ", row0);
  TORCH_CHECK_VALUE(values.dim() >= 1 && out.dim() == values.dim() &&
                        out.scalar_type() == values.scalar_type() &&
                        out.sizes().slice(1) == values.sizes().slice(1) &&
                        out.size(0) == keys.size(0) && out.is_contiguous(),
                    op, " expects values (rows, ...) and a contiguous out (n_scene, ...) of one ",
                    "dtype and row shape, got ", values.scalar_type(), " ", values.sizes(), " and ",
                    out.scalar_type(), " ", out.sizes(), " for ", keys.size(0), " keys");
  int64_t row = static_cast<int64_t>(values.element_size());
  for (int64_t d = 1; d < values.dim(); ++d) row *= values.size(d);
  TORCH_CHECK_VALUE(row > 0 && row % 4 == 0 && row <= INT32_MAX, op,
                    " expects rows of a multiple of 4 bytes, got ", row);
  TORCH_CHECK_VALUE(keys.device() == values.device() && out.device() == values.device(), op,
                    " expects every tensor on one device");
  return row;
}
const uint8_t* Bytes(const Tensor& t) { return static_cast<const uint8_t*>(t.data_ptr()); }

template <bool HIP>
Tensor scene_vote_impl(const std::optional<Tensor>& logits_, const Tensor& mask_,
                       const Tensor& orig_, int64_t row0, const Tensor& keys) {
  chk_scene_vote(logits_, mask_, orig_, row0, keys);
  TORCH_CHECK(HIP ? mask_.is_cuda() || fake(mask_) : mask_.device().is_cpu(),
              "scene_vote: mask is on ", mask_.device());
  Tensor mask = mask_.contiguous(), orig = orig_.contiguous(), logits;
  int C = 0;
  if (logits_.has_value()) {
    logits = logits_->contiguous();
    C = I(logits.size(-1));
  }
  Tensor pred = at::empty(mask.sizes(), i32(mask));
  if (fake(mask)) return pred;
  const long long rows = mask.numel(), n = keys.size(0);
  if (HIP) {
    c10::hip::HIPGuard g(mask.device().index());
    check_rc(pn2_scene_vote(F(logits), rows, C, Bytes(mask), Ii(orig), row0, n, Keys(keys),
                            pred.data_ptr<int32_t>(), stream_of(mask)), "scene_vote");
  } else {
    check_rc(pn2cpu_scene_vote(F(logits), rows, C, Bytes(mask), Ii(orig), row0, n, Keys(keys),
                               pred.data_ptr<int32_t>()), "scene_vote");
  }
  bump(keys);
  return pred;
}

template <bool HIP>
std::tuple<Tensor, Tensor, Tensor> scene_labels_impl(const Tensor& keys,
                                                     const std::optional<Tensor>& lut_,
                                                     int64_t dflt) {
  const char* op = "scene_labels";
  chk_keys(keys, op);
  chk_i32_dflt(dflt, op);
  TORCH_CHECK(HIP ? keys.is_cuda() || fake(keys) : keys.device().is_cpu(),
              "scene_labels: keys is on ", keys.device());
  Tensor lut;
  if (lut_.has_value()) {
    chk_lut(*lut_, keys, op);
    lut = lut_->contiguous();
  }
  const long long n = keys.size(0);
  Tensor labels = at::empty({n}, i32(keys)), winner = at::empty({n}, keys.options());
  Tensor mapped = at::empty({lut.defined() ? n : 0}, i32(keys));
  if (fake(keys)) return {labels, mapped, winner};
  const int32_t* lp = lut.defined() ? Ii(lut) : nullptr;
  const int nlut = lut.defined() ? I(lut.numel()) : 0;
  int32_t* mp = lut.defined() ? mapped.data_ptr<int32_t>() : nullptr;
  if (HIP) {
    c10::hip::HIPGuard g(keys.device().index());
    check_rc(pn2_scene_labels(KeysC(keys), n, lp, nlut, static_cast<int32_t>(dflt),
                              labels.data_ptr<int32_t>(), mp, Keys(winner), stream_of(keys)), op);
  } else {
    check_rc(pn2cpu_scene_labels(KeysC(keys), n, lp, nlut, static_cast<int32_t>(dflt),
                                 labels.data_ptr<int32_t>(), mp, Keys(winner)), op);
  }
  return {labels, mapped, winner};
}

template <bool HIP>
void map_back_rows_impl(const Tensor& values_, int64_t row0, const Tensor& keys,
                        const Tensor& out) {
  const int64_t row = chk_map_back(values_, row0, keys, out);
  TORCH_CHECK(HIP ? keys.is_cuda() || fake(keys) : keys.device().is_cpu(),
              "map_back_rows: keys is on ", keys.device());
  Tensor values = values_.contiguous();
  if (fake(keys)) return;
  const long long rows = values.size(0), n = keys.size(0);
  if (HIP) {
    c10::hip::HIPGuard g(keys.device().index());
    check_rc(pn2_map_back_rows(values.data_ptr(), I(row), row0, rows, KeysC(keys), n,
                               out.data_ptr(), stream_of(keys)), "map_back_rows");
  } else {
    check_rc(pn2cpu_map_back_rows(values.data_ptr(), I(row), row0, rows, KeysC(keys), n,
                                  out.data_ptr()), "map_back_rows");
  }
  bump(out);
}

template <bool HIP>
Tensor label_lut_impl(const Tensor& inp_, const Tensor& lut_, int64_t dflt) {
  const char* op = "label_lut";
  TORCH_CHECK_VALUE(inp_.scalar_type() == at::kInt, op, " expects int32 inp, got ",
                    inp_.scalar_type());
  chk_lut(lut_, inp_, op);
  chk_i32_dflt(dflt, op);
  TORCH_CHECK(HIP ? inp_.is_cuda() || fake(inp_) : inp_.device().is_cpu(),
              "label_lut: inp is on ", inp_.device());
  Tensor inp = inp_.contiguous(), lut = lut_.contiguous();
  Tensor out = at::empty(inp.sizes(), i32(inp));
  if (fake(inp)) return out;
  if (HIP) {
    c10::hip::HIPGuard g(inp.device().index());
    check_rc(pn2_label_lut(Ii(inp), inp.numel(), Ii(lut), I(lut.numel()),
                           static_cast<int32_t>(dflt), out.data_ptr<int32_t>(), stream_of(inp)), op);
  } else {
    check_rc(pn2cpu_label_lut(Ii(inp), inp.numel(), Ii(lut), I(lut.numel()),
                              static_cast<int32_t>(dflt), out.data_ptr<int32_t>()), op);
  }
  return out;
}

// ---- the training feed (csrc/feed.hip, pn2_val_select in csrc/scene.hip): get_data_tensors and
// random_rotate in one launch, and the validation chunker. CUDA, Meta and CPU (the host twins
// of csrc/cpu_feed.cpp: equal bits) from one body each, as the prediction ops above.
// an argument of the feed ops: on the body's device, of dtype dt, made contiguous
Tensor feed_arg(const Tensor& t, const Tensor& like, at::ScalarType dt, const char* op,
                const char* name) {
  TORCH_CHECK_VALUE(t.scalar_type() == dt, op, " expects ", dt, " ", name, ", got ",
                    t.scalar_type());
  TORCH_CHECK_VALUE(t.device() == like.device(), op, " expects every tensor on one device");
  return t.contiguous();
}
template <bool HIP>
void feed_device(const Tensor& t, const char* op) {
  TORCH_CHECK(HIP ? t.is_cuda() || fake(t) : t.device().is_cpu(), op, ": points is on ",
              t.device());
}

template <bool HIP>
std::tuple<Tensor, Tensor, Tensor> feed_batch_impl(
    const Tensor& points_, const Tensor& labels_, const std::optional<Tensor>& colors_,
    const std::optional<Tensor>& normals_, const Tensor& sample_weight_,
    const std::optional<Tensor>& cs_, const Tensor& class_weights_, bool use_color,
    bool use_normal) {
  const char* op = "feed_batch";
  TORCH_CHECK_VALUE(points_.dim() == 3 && points_.size(2) == 3, op,
                    " expects (B,N,3) points, got ", points_.sizes());
  const int64_t B = points_.size(0), N = points_.size(1);
  TORCH_CHECK_VALUE(B <= INT32_MAX && N <= INT32_MAX, op, " expects B and N below 2^31");
  feed_device<HIP>(points_, op);
  Tensor points = feed_arg(points_, points_, at::kFloat, op, "points");
  Tensor labels = feed_arg(labels_, points_, at::kInt, op, "labels");
  Tensor sw = feed_arg(sample_weight_, points_, at::kFloat, op, "sample_weight");
  Tensor cw = feed_arg(class_weights_, points_, at::kFloat, op, "class_weights");
  TORCH_CHECK_VALUE(labels.dim() == 2 && labels.size(0) == B && labels.size(1) == N &&
                        sw.sizes() == labels.sizes(),
                    op, " expects (B,N) labels and sample_weight, got ", labels.sizes(), " and ",
                    sw.sizes());
  TORCH_CHECK_VALUE(cw.dim() == 1, op, " expects (L) class_weights, got ", cw.sizes());
  Tensor colors, normals, cs;
  if (use_color) {
    TORCH_CHECK_VALUE(has(colors_), op, ": use_color needs colors");
    colors = feed_arg(*colors_, points_, at::kInt, op, "colors");
    TORCH_CHECK_VALUE(colors.sizes() == points.sizes(), op, " expects (B,N,3) colors, got ",
                      colors.sizes());
  }
  if (use_normal) {
    TORCH_CHECK_VALUE(has(normals_), op, ": use_normal needs normals");
    normals = feed_arg(*normals_, points_, at::kFloat, op, "normals");
    TORCH_CHECK_VALUE(normals.sizes() == points.sizes(), op, " expects (B,N,3) normals, got ",
                      normals.sizes());
  }
  if (has(cs_)) {
    cs = feed_arg(*cs_, points_, at::kFloat, op, "cs");
    TORCH_CHECK_VALUE(cs.dim() == 2 && cs.size(0) == B && cs.size(1) == 2, op,
                      " expects (B,2) cs, got ", cs.sizes());
  }
  const int64_t nf = (use_color ? 3 : 0) + (use_normal ? 3 : 0);
  Tensor xyz = at::empty({B, N, 3}, f32(points)), features = at::empty({B, N, nf}, f32(points));
  Tensor smpw = at::empty({B, N}, f32(points));
  if (fake(points) || B * N == 0) return {xyz, features, smpw};
  const int32_t* cp = colors.defined() ? Ii(colors) : nullptr;
  float* fp = nf ? features.data_ptr<float>() : nullptr;
  if (HIP) {
    c10::hip::HIPGuard g(points.device().index());
    check_rc(pn2_feed_batch(F(points), Ii(labels), cp, F(normals), F(sw), F(cs), F(cw),
                            I(cw.numel()), I(B), I(N), use_color, use_normal,
                            xyz.data_ptr<float>(), fp, smpw.data_ptr<float>(), stream_of(points)),
             op);
  } else {
    check_rc(pn2cpu_feed_batch(F(points), Ii(labels), cp, F(normals), F(sw), F(cs), F(cw),
                               I(cw.numel()), I(B), I(N), use_color, use_normal,
                               xyz.data_ptr<float>(), fp, smpw.data_ptr<float>()), op);
  }
  return {xyz, features, smpw};
}

template <bool HIP>
std::tuple<Tensor, Tensor, Tensor> val_select_impl(const Tensor& points_, const Tensor& bounds_,
                                                   double margin, double inner_margin) {
  const char* op = "val_select";
  TORCH_CHECK_VALUE(points_.dim() == 2 && points_.size(1) == 3, op, " expects (N,3) points, got ",
                    points_.sizes());
  TORCH_CHECK_VALUE(bounds_.dim() == 2 && bounds_.size(1) == 6, op,
                    " expects (S,6) float64 bounds, got ", bounds_.sizes());
  feed_device<HIP>(points_, op);
  Tensor points = feed_arg(points_, points_, at::kFloat, op, "points");
  Tensor bounds = feed_arg(bounds_, points_, at::kDouble, op, "bounds");
  const int64_t N = points.size(0), S = bounds.size(0);
  TORCH_CHECK_VALUE(S <= 65535 && N * S <= INT32_MAX, op, " expects S <= 65535 and S * N <= 2^31 - 1, got S = ",
                    S, ", N = ", N);
  Tensor counts = at::empty({S}, i32(points)), sel = at::empty({S, N}, i32(points));
  Tensor inner = at::empty({S, N}, points.options().dtype(at::kByte));
  if (HIP) {
    Tensor ws = at::empty({static_cast<int64_t>(pn2_val_select_workspace_size(I(N), I(S)) / 4)},
                          i32(points));
    if (fake(points) || S == 0) return {counts, sel, inner};
    c10::hip::HIPGuard g(points.device().index());
    check_rc(pn2_val_select(F(points), I(N), bounds.data_ptr<double>(), I(S), margin, inner_margin,
                            ws.data_ptr(), ws.numel() * 4, counts.data_ptr<int32_t>(),
                            sel.data_ptr<int32_t>(), inner.data_ptr<uint8_t>(),
                            stream_of(points)), op);
  } else {
    if (S == 0) return {counts, sel, inner};
    check_rc(pn2cpu_val_select(F(points), I(N), bounds.data_ptr<double>(), I(S), margin,
                               inner_margin, counts.data_ptr<int32_t>(), sel.data_ptr<int32_t>(),
                               inner.data_ptr<uint8_t>()), op);
  }
  return {counts, sel, inner};
}

using Tensor7 = std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor>;
template <bool HIP>
Tensor7 val_chunks_impl(const Tensor& points_, const Tensor& labels_,
                        const std::optional<Tensor>& colors_,
                        const std::optional<Tensor>& normals_, const Tensor& counts_,
                        const Tensor& sel_, const Tensor& inner_,
                        const std::optional<Tensor>& choice_, const std::optional<Tensor>& u_,
                        int64_t K, const Tensor& label_weights_, double min_inside) {
  const char* op = "val_chunks";
  TORCH_CHECK_VALUE(points_.dim() == 2 && points_.size(1) == 3, op, " expects (N,3) points, got ",
                    points_.sizes());
  TORCH_CHECK_VALUE(K >= 0 && K <= INT32_MAX, op, " expects 0 <= npoints < 2^31, got ", K);
  feed_device<HIP>(points_, op);
  Tensor points = feed_arg(points_, points_, at::kFloat, op, "points");
  Tensor labels = feed_arg(labels_, points_, at::kInt, op, "labels");
  Tensor counts = feed_arg(counts_, points_, at::kInt, op, "counts");
  Tensor sel = feed_arg(sel_, points_, at::kInt, op, "sel");
  Tensor inner = feed_arg(inner_, points_, at::kByte, op, "inner");
  Tensor lw = feed_arg(label_weights_, points_, at::kFloat, op, "label_weights");
  const int64_t N = points.size(0), S = counts.numel();
  TORCH_CHECK_VALUE(labels.dim() == 1 && labels.size(0) == N, op, " expects (N) labels, got ",
                    labels.sizes());
  TORCH_CHECK_VALUE(counts.dim() == 1 && sel.dim() == 2 && sel.size(0) == S && sel.size(1) == N &&
                        inner.sizes() == sel.sizes(),
                    op, " expects counts (S), sel (S,N) and inner (S,N), got ", counts.sizes(), ", ",
                    sel.sizes(), " and ", inner.sizes());
  TORCH_CHECK_VALUE(lw.dim() == 1, op, " expects (L) label_weights, got ", lw.sizes());
  TORCH_CHECK_VALUE(S <= 65535 && N * S <= INT32_MAX && K * S <= INT32_MAX, op,
                    " expects S <= 65535, S * N <= 2^31 - 1 and S * npoints <= 2^31 - 1");
  Tensor colors, normals, choice, u;
  if (has(colors_)) {
    colors = feed_arg(*colors_, points_, at::kInt, op, "colors");
    TORCH_CHECK_VALUE(colors.sizes() == points.sizes(), op, " expects (N,3) colors, got ",
                      colors.sizes());
  }
  if (has(normals_)) {
    normals = feed_arg(*normals_, points_, at::kFloat, op, "normals");
    TORCH_CHECK_VALUE(normals.sizes() == points.sizes(), op, " expects (N,3) normals, got ",
                      normals.sizes());
  }
  if (has(choice_)) {
    choice = feed_arg(*choice_, points_, at::kInt, op, "choice");
    TORCH_CHECK_VALUE(choice.dim() == 2 && choice.size(0) == S && choice.size(1) == K, op,
                      " expects (S,npoints) choice, got ", choice.sizes());
  } else {
    TORCH_CHECK_VALUE(has(u_), op, " expects choice or u");
    u = feed_arg(*u_, points_, at::kFloat, op, "u");
    TORCH_CHECK_VALUE(u.dim() == 2 && u.size(0) == S && u.size(1) == K, op,
                      " expects (S,npoints) u, got ", u.sizes());
  }
  Tensor op_ = at::empty({S, K, 3}, f32(points)), ol = at::empty({S, K}, i32(points));
  Tensor oc = colors.defined() ? at::empty({S, K, 3}, i32(points)) : at::empty({0}, i32(points));
  Tensor on = normals.defined() ? at::empty({S, K, 3}, f32(points)) : at::empty({0}, f32(points));
  Tensor ow = at::empty({S, K}, f32(points)), column = at::empty({S}, i32(points));
  Tensor kept = at::empty({1}, i32(points));
  if (fake(points)) return {op_, ol, oc, on, ow, column, kept};
  const int32_t* cp = colors.defined() ? Ii(colors) : nullptr;
  const int32_t* chp = choice.defined() ? Ii(choice) : nullptr;
  int32_t* ocp = colors.defined() ? oc.data_ptr<int32_t>() : nullptr;
  float* onp = normals.defined() ? on.data_ptr<float>() : nullptr;
  if (HIP) {
    Tensor ws = at::empty({static_cast<int64_t>(pn2_val_chunks_workspace_size(I(S)) / 4)},
                          i32(points));
    c10::hip::HIPGuard g(points.device().index());
    check_rc(pn2_val_chunks(F(points), Ii(labels), cp, F(normals), I(N), Ii(counts), Ii(sel),
                            inner.data_ptr<uint8_t>(), I(S), chp, F(u), I(K), F(lw),
                            I(lw.numel()), min_inside, ws.data_ptr(), ws.numel() * 4,
                            op_.data_ptr<float>(), ol.data_ptr<int32_t>(), ocp, onp,
                            ow.data_ptr<float>(), column.data_ptr<int32_t>(),
                            kept.data_ptr<int32_t>(), stream_of(points)), op);
  } else {
    check_rc(pn2cpu_val_chunks(F(points), Ii(labels), cp, F(normals), I(N), Ii(counts), Ii(sel),
                               inner.data_ptr<uint8_t>(), I(S), chp, F(u), I(K), F(lw),
                               I(lw.numel()), min_inside, op_.data_ptr<float>(),
                               ol.data_ptr<int32_t>(), ocp, onp, ow.data_ptr<float>(),
                               column.data_ptr<int32_t>(), kept.data_ptr<int32_t>()), op);
  }
  return {op_, ol, oc, on, ow, column, kept};
}

// ---- scene rendering (csrc/render.hip): the reference's render_ball as a 64-bit atomic max per
// pixel and a resolve pass, and the viewer's projection. CUDA, Meta and CPU (the host twins of
// csrc/cpu_render.cpp: equal bits) from one body each. No autograd.
// an fp64 argument: the kernels read it with 8-byte loads, so a view at an odd offset is copied
Tensor f64_arg(const Tensor& t) {
  Tensor c = t.contiguous();
  if (!fake(c) && reinterpret_cast<uintptr_t>(c.data_ptr()) % 8 != 0) c = c.clone();
  return c;
}

template <bool HIP>
Tensor render_ball_impl(const Tensor& ixyz_, const std::optional<Tensor>& c0_,
                        const std::optional<Tensor>& c1_, const std::optional<Tensor>& c2_,
                        const std::optional<Tensor>& labels_, const std::optional<Tensor>& palette_,
                        int64_t r, int64_t h, int64_t w, at::IntArrayRef background) {
  const char* op = "render_ball";
  TORCH_CHECK_VALUE(ixyz_.dim() == 3 && ixyz_.size(2) == 3, op, " expects (F,n,3) int32 ixyz, got ",
                    ixyz_.sizes());
  feed_device<HIP>(ixyz_, op);
  Tensor ixyz = feed_arg(ixyz_, ixyz_, at::kInt, op, "ixyz");
  const int64_t nf = ixyz.size(0), n = ixyz.size(1);
  TORCH_CHECK_VALUE(nf <= 65535 && n <= INT32_MAX, op, " expects F <= 65535 and n below 2^31");
  TORCH_CHECK_VALUE(h >= 0 && w >= 0 && h * w <= INT32_MAX, op,
                    " expects 0 <= h, w and h * w below 2^31, got ", h, " x ", w);
  TORCH_CHECK_VALUE(r <= PN2_RENDER_MAX_RADIUS, op, " expects r <= ", PN2_RENDER_MAX_RADIUS,
                    ", got ", r);
  TORCH_CHECK_VALUE(background.size() == 3, op, " expects three background bytes");
  for (int64_t b : background)
    TORCH_CHECK_VALUE(b >= 0 && b <= 255, op, " expects background bytes in [0, 255], got ", b);
  Tensor c0, c1, c2, labels, palette;
  if (has(labels_)) {
    TORCH_CHECK_VALUE(has(palette_) && !has(c0_) && !has(c1_) && !has(c2_), op,
                      " expects labels with a palette and without colour channels");
    labels = feed_arg(*labels_, ixyz_, at::kInt, op, "labels");
    palette = feed_arg(*palette_, ixyz_, at::kFloat, op, "palette");
    TORCH_CHECK_VALUE(labels.dim() == 1 && labels.size(0) == n, op, " expects (n) labels, got ",
                      labels.sizes());
    TORCH_CHECK_VALUE(palette.dim() == 2 && palette.size(0) >= 1 && palette.size(1) == 3 &&
                          palette.size(0) <= INT32_MAX,
                      op, " expects (npal,3) palette with npal >= 1, got ", palette.sizes());
  } else {
    TORCH_CHECK_VALUE(has(c0_) && has(c1_) && has(c2_) && !has(palette_), op,
                      " expects three colour channels, or labels and a palette");
    c0 = feed_arg(*c0_, ixyz_, at::kFloat, op, "c0");
    c1 = feed_arg(*c1_, ixyz_, at::kFloat, op, "c1");
    c2 = feed_arg(*c2_, ixyz_, at::kFloat, op, "c2");
    TORCH_CHECK_VALUE(c0.dim() == 1 && c0.size(0) == n && c1.sizes() == c0.sizes() &&
                          c2.sizes() == c0.sizes(),
                      op, " expects (n) c0, c1 and c2, got ", c0.sizes(), ", ", c1.sizes(), " and ",
                      c2.sizes());
  }
  Tensor images = at::empty({nf, h, w, 3}, ixyz.options().dtype(at::kByte));
  if (fake(ixyz) || images.numel() == 0) return images;
  const int bg0 = I(background[0]), bg1 = I(background[1]), bg2 = I(background[2]);
  const int npal = palette.defined() ? I(palette.size(0)) : 0;
  const int32_t* lp = labels.defined() ? Ii(labels) : nullptr;
  if (HIP) {
    c10::hip::HIPGuard g(ixyz.device().index());
    const size_t ws = pn2_render_ball_workspace_size(I(nf), I(h), I(w));
    Tensor work = at::empty({static_cast<int64_t>(ws / 8)}, ixyz.options().dtype(at::kLong));
    check_rc(pn2_render_ball(Ii(ixyz), I(nf), n, F(c0), F(c1), F(c2), lp, F(palette), npal, I(r),
                             I(h), I(w), bg0, bg1, bg2, images.data_ptr<uint8_t>(),
                             work.data_ptr(), ws, stream_of(ixyz)), op);
  } else {
    check_rc(pn2cpu_render_ball(Ii(ixyz), I(nf), n, F(c0), F(c1), F(c2), lp, F(palette), npal,
                                I(r), I(h), I(w), bg0, bg1, bg2, images.data_ptr<uint8_t>()), op);
  }
  return images;
}

template <bool HIP>
Tensor render_project_impl(const Tensor& xyz_, const Tensor& mats_) {
  const char* op = "render_project";
  TORCH_CHECK_VALUE(xyz_.dim() == 2 && xyz_.size(1) == 3 && xyz_.size(0) <= INT32_MAX, op,
                    " expects (n,3) xyz, got ", xyz_.sizes());
  TORCH_CHECK_VALUE(xyz_.scalar_type() == at::kFloat || xyz_.scalar_type() == at::kDouble, op,
                    " expects float32 or float64 xyz, got ", xyz_.scalar_type());
  TORCH_CHECK_VALUE(mats_.dim() == 2 && mats_.size(1) == 12 && mats_.size(0) <= INT32_MAX, op,
                    " expects (F,12) float64 mats, got ", mats_.sizes());
  feed_device<HIP>(xyz_, op);
  const bool f64 = xyz_.scalar_type() == at::kDouble;
  Tensor xyz = f64 ? f64_arg(xyz_) : xyz_.contiguous();
  Tensor mats = f64_arg(feed_arg(mats_, xyz_, at::kDouble, op, "mats"));
  const int64_t nf = mats.size(0), n = xyz.size(0);
  Tensor ixyz = at::empty({nf, n, 3}, i32(xyz));
  if (fake(xyz) || ixyz.numel() == 0) return ixyz;
  if (HIP) {
    c10::hip::HIPGuard g(xyz.device().index());
    check_rc(pn2_render_project(xyz.data_ptr(), f64, n, mats.data_ptr<double>(), I(nf),
                                ixyz.data_ptr<int32_t>(), stream_of(xyz)), op);
  } else {
    check_rc(pn2cpu_render_project(xyz.data_ptr(), f64, n, mats.data_ptr<double>(), I(nf),
                                   ixyz.data_ptr<int32_t>()), op);
  }
  return ixyz;
}

// ---- training-mode geometry (csrc/geom_train.hip): the fused forward kernels of the SA and FP
// modules with their gradients as ordered gathers (no float atomics, no zero fill, no slices)
void chk_group_concat_grad(const Tensor& grad, const Tensor& idx, int64_t N, int64_t C,
                           int64_t col0) {
  TORCH_CHECK_VALUE(grad.dim() == 4 && idx.dim() == 3 && grad.size(0) == idx.size(0) &&
                        grad.size(1) == idx.size(1) && grad.size(2) == idx.size(2),
                    "group_concat_train_grad expects grad_new_points (B,M,ns,Cout), idx (B,M,ns)");
  TORCH_CHECK_VALUE(N >= 0 && C >= 0 && col0 >= 0 && col0 + C <= grad.size(3),
                    "group_concat_train_grad expects columns [col0, col0 + C) inside Cout");
}
void chk_fp_apply_train(const Tensor& dist, const Tensor& idx, const std::optional<Tensor>& points1,
                        const Tensor& points2) {
  TORCH_CHECK_VALUE(dist.dim() == 3 && dist.size(2) == 3 && idx.dim() == 3 &&
                        idx.sizes() == dist.sizes(),
                    "fp_apply_train expects (b,n,3) dist and idx");
  TORCH_CHECK_VALUE(points2.dim() == 3 && points2.size(0) == dist.size(0),
                    "fp_apply_train expects (b,m,c2) points2");
  if (points1.has_value() && points1->numel() > 0)
    TORCH_CHECK_VALUE(points1->dim() == 3 && points1->size(0) == dist.size(0) &&
                          points1->size(1) == dist.size(1),
                      "fp_apply_train expects (b,n,c1) points1");
}
void chk_fp_apply_train_grad(const Tensor& grad_out, const Tensor& dist, const Tensor& idx,
                             int64_t m, int64_t C2, int64_t C1) {
  TORCH_CHECK_VALUE(dist.dim() == 3 && dist.size(2) == 3 && idx.dim() == 3 &&
                        idx.sizes() == dist.sizes(),
                    "fp_apply_train_grad expects (b,n,3) dist and idx");
  TORCH_CHECK_VALUE(m >= 0 && C2 >= 0 && C1 >= 0 && grad_out.dim() == 3 &&
                        grad_out.size(0) == dist.size(0) && grad_out.size(1) == dist.size(1) &&
                        grad_out.size(2) == C2 + C1,
                    "fp_apply_train_grad expects (b,n,C2+C1) grad_out");
}

// the inverse index of keys (B, S) over K rows per cloud (pn2_inverse_index_build)
Tensor inverse_index(const Tensor& keys, int B, int S, int K, const char* op) {
  const size_t bytes = pn2_inverse_index_size(B, S, K);
  Tensor inv = workspace(keys, bytes);
  check_rc(pn2_inverse_index_build(Ii(keys), B, S, K, P(inv), bytes, stream_of(keys)), op);
  return inv;
}

Tensor group_concat_train_hip(const Tensor& xyz, const std::optional<Tensor>& points,
                              const Tensor& new_xyz, const Tensor& idx, bool use_xyz,
                              bool xyz_last) {
  return std::get<1>(group_concat_impl(xyz, points, new_xyz, idx, use_xyz, xyz_last, false));
}

Tensor group_concat_train_grad_hip(const Tensor& grad_, const Tensor& idx_, int64_t N, int64_t C,
                                   int64_t col0) {
  const char* op = "group_concat_train_grad";
  chk_group_concat_grad(grad_, idx_, N, C, col0);
  Tensor grad = dev(grad_, "grad_new_points", at::kFloat), idx = dev(idx_, "idx", at::kInt);
  const int B = I(idx.size(0)), M = I(idx.size(1)), ns = I(idx.size(2));
  TORCH_CHECK_VALUE(idx.size(1) * idx.size(2) <= PN2_INV_MAX_SLOTS && N <= PN2_INV_MAX_KEYS, op,
                    ": more slots or points per cloud than the inverse index takes");
  Tensor gp = at::empty({B, N, C}, f32(grad));
  if (fake(grad) || gp.numel() == 0) return gp;
  c10::hip::HIPGuard g(grad.device().index());
  Tensor inv = inverse_index(idx, B, M * ns, I(N), op);
  check_rc(pn2_group_point_grad_ordered(F(grad), I(grad.size(3)), I(col0), P(inv), B, I(N), I(C),
                                        M, ns, gp.data_ptr<float>(), stream_of(grad)), op);
  return gp;
}

Tensor fp_apply_train_hip(const Tensor& dist_, const Tensor& idx_,
                          const std::optional<Tensor>& points1_, const Tensor& points2_) {
  chk_fp_apply_train(dist_, idx_, points1_, points2_);
  Tensor dist = dev(dist_, "dist", at::kFloat), idx = dev(idx_, "idx", at::kInt);
  Tensor points2 = dev(points2_, "points2", at::kFloat);
  Tensor points1;
  if (points1_.has_value() && points1_->numel() > 0) points1 = dev(*points1_, "points1", at::kFloat);
  const int B = I(dist.size(0)), n = I(dist.size(1)), m = I(points2.size(1));
  const int C2 = I(points2.size(2)), C1 = points1.defined() ? I(points1.size(2)) : 0;
  Tensor out = at::empty({B, n, C2 + C1}, f32(dist));
  if (fake(dist)) return out;
  c10::hip::HIPGuard g(dist.device().index());
  check_rc(pn2_fp_apply(F(dist), Ii(idx), nullptr, F(points1), C1, F(points2), C2, B, n, m,
                        out.data_ptr<float>(), stream_of(dist)), "fp_apply_train");
  return out;
}

std::tuple<Tensor, Tensor> fp_apply_train_grad_hip(const Tensor& grad_out_, const Tensor& dist_,
                                                   const Tensor& idx_, int64_t m, int64_t C2,
                                                   int64_t C1) {
  const char* op = "fp_apply_train_grad";
  chk_fp_apply_train_grad(grad_out_, dist_, idx_, m, C2, C1);
  Tensor grad = dev(grad_out_, "grad_out", at::kFloat), dist = dev(dist_, "dist", at::kFloat);
  Tensor idx = dev(idx_, "idx", at::kInt);
  const int B = I(dist.size(0)), n = I(dist.size(1));
  TORCH_CHECK_VALUE(3 * dist.size(1) <= PN2_INV_MAX_SLOTS && m <= PN2_INV_MAX_KEYS, op,
                    ": more unknown or known points per cloud than the inverse index takes");
  Tensor g1 = grad.narrow(2, C2, C1).contiguous();  // the points1 columns: one strided copy
  Tensor g2 = at::empty({B, m, C2}, f32(grad));
  if (fake(grad) || g2.numel() == 0) return {g2, g1};
  c10::hip::HIPGuard g(grad.device().index());
  Tensor weight = at::empty_like(dist);  // the bits of pn2_idw_weights: the forward's weights
  if (n > 0) check_rc(pn2_idw_weights(F(dist), B, n, weight.data_ptr<float>(), stream_of(grad)), op);
  Tensor inv = inverse_index(idx, B, 3 * n, I(m), op);
  check_rc(pn2_three_interpolate_grad_ordered(F(grad), I(C2 + C1), 0, P(inv), F(weight), B, n,
                                              I(C2), I(m), g2.data_ptr<float>(), stream_of(grad)),
           op);
  return {g2, g1};
}

// ------------------------------------------------------------------------- autograd (C++)
// The two ops of the training head carry their autograd here instead of in _torch_ops.py: the
// head is bound by launches and host time, and a Python-registered backward
// costs more host time per call than both kernels take on the device. Forward and backward go
// back through the dispatcher, so the bodies above serve both, on the device and under Meta.
using torch::autograd::AutogradContext;
using torch::autograd::variable_list;

struct DropoutFn : public torch::autograd::Function<DropoutFn> {
  static Tensor forward(AutogradContext* ctx, const Tensor& x, double keep_prob, int64_t seed) {
    at::AutoDispatchBelowADInplaceOrView guard;
    ctx->saved_data["keep_prob"] = keep_prob;  // the mask is a function of (seed, element)
    ctx->saved_data["seed"] = seed;
    static auto op = c10::Dispatcher::singleton()
                         .findSchemaOrThrow("pn2::dropout", "")
                         .typed<Tensor(const Tensor&, double, int64_t)>();
    return op.call(x, keep_prob, seed);
  }
  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    if (!grads[0].defined()) return {Tensor(), Tensor(), Tensor()};
    static auto op = c10::Dispatcher::singleton()
                         .findSchemaOrThrow("pn2::dropout", "")
                         .typed<Tensor(const Tensor&, double, int64_t)>();
    return {op.call(grads[0].contiguous(), ctx->saved_data["keep_prob"].toDouble(),
                    ctx->saved_data["seed"].toInt()),
            Tensor(), Tensor()};
  }
};
Tensor dropout_autograd(const Tensor& x, double keep_prob, int64_t seed) {
  return DropoutFn::apply(x, keep_prob, seed);
}

struct SoftmaxXentFn : public torch::autograd::Function<SoftmaxXentFn> {
  static variable_list forward(AutogradContext* ctx, const Tensor& logits, const Tensor& labels,
                               const std::optional<Tensor>& weights) {
    at::AutoDispatchBelowADInplaceOrView guard;
    static auto op =
        c10::Dispatcher::singleton()
            .findSchemaOrThrow("pn2::softmax_xent", "")
            .typed<std::tuple<Tensor, Tensor, Tensor, Tensor>(
                const Tensor&, const Tensor&, const std::optional<Tensor>&)>();
    auto [loss, lse, pred, num_present] = op.call(logits, labels, weights);
    ctx->mark_non_differentiable({lse, pred, num_present});
    ctx->save_for_backward({logits, labels, has(weights) ? *weights : Tensor(), lse, num_present});
    return {loss, lse, pred, num_present};
  }
  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    // the weights get no gradient: the reference feeds them from a placeholder
    if (!grads[0].defined()) return {Tensor(), Tensor(), Tensor()};
    const variable_list saved = ctx->get_saved_variables();
    static auto op = c10::Dispatcher::singleton()
                         .findSchemaOrThrow("pn2::softmax_xent_grad", "")
                         .typed<Tensor(const Tensor&, const Tensor&, const Tensor&,
                                       const std::optional<Tensor>&, const Tensor&,
                                       const Tensor&)>();
    const std::optional<Tensor> weights =
        saved[2].defined() ? std::optional<Tensor>(saved[2]) : std::nullopt;
    return {op.call(grads[0].contiguous(), saved[0], saved[1], weights, saved[3], saved[4]),
            Tensor(), Tensor()};
  }
};
std::tuple<Tensor, Tensor, Tensor, Tensor> softmax_xent_autograd(
    const Tensor& logits, const Tensor& labels, const std::optional<Tensor>& weights) {
  variable_list o = SoftmaxXentFn::apply(logits, labels, weights);
  return {o[0], o[1], o[2], o[3]};
}

// The training-mode geometry ops (csrc/geom_train.hip) likewise: `points` (group_concat_train),
// `points1` and `points2` (fp_apply_train) get gradients, the coordinates, distances and indices
// none (pointnet_util keeps the composition of reference ops when xyz asks for one).
struct GroupConcatTrainFn : public torch::autograd::Function<GroupConcatTrainFn> {
  static Tensor forward(AutogradContext* ctx, const Tensor& xyz,
                        const std::optional<Tensor>& points, const Tensor& new_xyz,
                        const Tensor& idx, bool use_xyz, bool xyz_last) {
    at::AutoDispatchBelowADInplaceOrView guard;
    const bool has_points = points.has_value() && points->defined() && points->numel() > 0;
    ctx->saved_data["N"] = xyz.dim() == 3 ? xyz.size(1) : int64_t(0);
    ctx->saved_data["C"] = has_points && points->dim() == 3 ? points->size(2) : int64_t(0);
    ctx->saved_data["col0"] = int64_t(has_points && use_xyz && !xyz_last ? 3 : 0);
    ctx->saved_data["has_points"] = has_points;
    ctx->save_for_backward({idx});
    static auto op = c10::Dispatcher::singleton()
                         .findSchemaOrThrow("pn2::group_concat_train", "")
                         .typed<Tensor(const Tensor&, const std::optional<Tensor>&, const Tensor&,
                                       const Tensor&, bool, bool)>();
    return op.call(xyz, points, new_xyz, idx, use_xyz, xyz_last);
  }
  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    variable_list out(6);
    if (!grads[0].defined() || !ctx->saved_data["has_points"].toBool() ||
        !ctx->needs_input_grad(1))
      return out;
    static auto op = c10::Dispatcher::singleton()
                         .findSchemaOrThrow("pn2::group_concat_train_grad", "")
                         .typed<Tensor(const Tensor&, const Tensor&, int64_t, int64_t, int64_t)>();
    // (a gradient that is not contiguous is made so once; the kernel reads rows in place)
    out[1] = op.call(grads[0].contiguous(), ctx->get_saved_variables()[0],
                     ctx->saved_data["N"].toInt(), ctx->saved_data["C"].toInt(),
                     ctx->saved_data["col0"].toInt());
    return out;
  }
};
Tensor group_concat_train_autograd(const Tensor& xyz, const std::optional<Tensor>& points,
                                   const Tensor& new_xyz, const Tensor& idx, bool use_xyz,
                                   bool xyz_last) {
  return GroupConcatTrainFn::apply(xyz, points, new_xyz, idx, use_xyz, xyz_last);
}

struct FpApplyTrainFn : public torch::autograd::Function<FpApplyTrainFn> {
  static Tensor forward(AutogradContext* ctx, const Tensor& dist, const Tensor& idx,
                        const std::optional<Tensor>& points1, const Tensor& points2) {
    at::AutoDispatchBelowADInplaceOrView guard;
    const bool has1 = points1.has_value() && points1->defined() && points1->numel() > 0;
    ctx->saved_data["m"] = points2.dim() == 3 ? points2.size(1) : int64_t(0);
    ctx->saved_data["C2"] = points2.dim() == 3 ? points2.size(2) : int64_t(0);
    ctx->saved_data["C1"] = has1 && points1->dim() == 3 ? points1->size(2) : int64_t(0);
    ctx->saved_data["has1"] = has1;
    // (an absent optional tensor is no autograd input: points2's edge index moves down)
    ctx->saved_data["p2_edge"] = int64_t(points1.has_value() && points1->defined() ? 3 : 2);
    ctx->save_for_backward({dist, idx});
    static auto op = c10::Dispatcher::singleton()
                         .findSchemaOrThrow("pn2::fp_apply_train", "")
                         .typed<Tensor(const Tensor&, const Tensor&, const std::optional<Tensor>&,
                                       const Tensor&)>();
    return op.call(dist, idx, points1, points2);
  }
  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    variable_list out(4);
    if (!grads[0].defined()) return out;
    const int64_t C2 = ctx->saved_data["C2"].toInt(), C1 = ctx->saved_data["C1"].toInt();
    const bool need1 = ctx->saved_data["has1"].toBool() && ctx->needs_input_grad(2);
    if (!ctx->needs_input_grad(ctx->saved_data["p2_edge"].toInt())) {  // points1 alone
      if (need1) out[2] = grads[0].narrow(2, C2, C1).contiguous();
      return out;
    }
    const variable_list saved = ctx->get_saved_variables();
    static auto op = c10::Dispatcher::singleton()
                         .findSchemaOrThrow("pn2::fp_apply_train_grad", "")
                         .typed<std::tuple<Tensor, Tensor>(const Tensor&, const Tensor&,
                                                           const Tensor&, int64_t, int64_t,
                                                           int64_t)>();
    auto [g2, g1] = op.call(grads[0].contiguous(), saved[0], saved[1],
                            ctx->saved_data["m"].toInt(), C2, C1);
    out[3] = g2;
    if (need1) out[2] = g1;
    return out;
  }
};
Tensor fp_apply_train_autograd(const Tensor& dist, const Tensor& idx,
                               const std::optional<Tensor>& points1, const Tensor& points2) {
  return FpApplyTrainFn::apply(dist, idx, points1, points2);
}

}  // namespace

// Schemas: the reference op names and argument order (tf_sampling.py, tf_grouping.py,
// tf_interpolate.py), plus the fused / extension ops of the C ABI.
TORCH_LIBRARY(pn2, m) {
  m.def("farthest_point_sample(int npoint, Tensor inp) -> Tensor");
  m.def("farthest_point_sample_and_gather(int npoint, Tensor inp) -> (Tensor, Tensor)");
  m.def("gather_point(Tensor inp, Tensor idx) -> Tensor");
  m.def("gather_point_grad(Tensor inp, Tensor idx, Tensor out_g) -> Tensor");
  m.def("prob_sample(Tensor inp, Tensor inpr) -> Tensor");
  m.def("query_ball_point(float radius, int nsample, Tensor xyz1, Tensor xyz2) -> (Tensor, Tensor)");
  m.def("select_top_k(int k, Tensor dist) -> (Tensor, Tensor)");
  m.def("knn_point(int k, Tensor xyz1, Tensor xyz2) -> (Tensor, Tensor)");
  m.def("group_point(Tensor points, Tensor idx) -> Tensor");
  m.def("group_point_grad(Tensor points, Tensor idx, Tensor grad_out) -> Tensor");
  m.def("group_concat(Tensor xyz, Tensor? points, Tensor new_xyz, Tensor idx, bool use_xyz=True, "
        "bool xyz_last=False) -> (Tensor, Tensor)");
  m.def("three_nn(Tensor xyz1, Tensor xyz2) -> (Tensor, Tensor)");
  m.def("three_interpolate(Tensor points, Tensor idx, Tensor weight) -> Tensor");
  m.def("three_interpolate_grad(Tensor points, Tensor idx, Tensor weight, Tensor grad_out) -> Tensor");
  m.def("idw_weights(Tensor dist) -> Tensor");
  m.def("fp_fused(Tensor xyz1, Tensor xyz2, Tensor? points1, Tensor points2) -> Tensor");
  m.def("attn_reduce(Tensor Q, Tensor K, Tensor V) -> Tensor");
  m.def("attn_reduce_grad(Tensor Q, Tensor K, Tensor V, Tensor grad_out) -> (Tensor, Tensor, Tensor)");
  m.def("attn_reduce_kd(Tensor Q, Tensor K, Tensor V, int key_dim) -> Tensor");
  m.def("attn_reduce_kd_grad(Tensor Q, Tensor K, Tensor V, Tensor grad_out, int key_dim) -> "
        "(Tensor, Tensor, Tensor)");
  m.def("head_mix(Tensor qkv, int heads, int key_dim) -> Tensor");
  m.def("dense_wide(Tensor x, Tensor packed, int cin, int cout, bool relu) -> Tensor");
  m.def("head_mix_grad(Tensor qkv, Tensor grad_out, int heads, int key_dim) -> Tensor");
  m.def("group_pool(Tensor x, Tensor? grouped_xyz, int mode) -> Tensor");
  m.def("mlp_layer_train(Tensor x, Tensor weight, Tensor? bias, Tensor? gamma, Tensor? beta, "
        "float eps, bool relu) -> (Tensor out, Tensor y, Tensor mean, Tensor var)");
  m.def("mlp_layer_train_grad(Tensor grad_out, Tensor x, Tensor weight, Tensor y, Tensor? mean, "
        "Tensor? var, Tensor? gamma, Tensor? beta, float eps, bool relu, bool need_grad_x) -> "
        "(Tensor grad_x, Tensor grad_w, Tensor grad_b, Tensor grad_gamma, Tensor grad_beta)");
  m.def("mlp_layer_train_pool(Tensor x, Tensor weight, Tensor? bias, Tensor? gamma, Tensor? beta, "
        "float eps, bool relu) -> (Tensor out, Tensor y, Tensor mean, Tensor var, Tensor arg)");
  m.def("mlp_layer_train_pool_grad(Tensor grad_out, Tensor arg, Tensor x, Tensor weight, Tensor y, "
        "Tensor? mean, Tensor? var, Tensor? gamma, Tensor? beta, float eps, bool relu, "
        "bool need_grad_x) -> "
        "(Tensor grad_x, Tensor grad_w, Tensor grad_b, Tensor grad_gamma, Tensor grad_beta)");
  // the training layer's bf16 mode (include/pn2hip.h, at pn2_mlp_pack_bf16): the schemas of the
  // four ops above, the GEMMs on the bf16 matrix cores
  m.def("mlp_layer_train_bf16(Tensor x, Tensor weight, Tensor? bias, Tensor? gamma, Tensor? beta, "
        "float eps, bool relu) -> (Tensor out, Tensor y, Tensor mean, Tensor var)");
  m.def("mlp_layer_train_bf16_grad(Tensor grad_out, Tensor x, Tensor weight, Tensor y, "
        "Tensor? mean, Tensor? var, Tensor? gamma, Tensor? beta, float eps, bool relu, "
        "bool need_grad_x) -> "
        "(Tensor grad_x, Tensor grad_w, Tensor grad_b, Tensor grad_gamma, Tensor grad_beta)");
  m.def("mlp_layer_train_pool_bf16(Tensor x, Tensor weight, Tensor? bias, Tensor? gamma, "
        "Tensor? beta, float eps, bool relu) -> "
        "(Tensor out, Tensor y, Tensor mean, Tensor var, Tensor arg)");
  m.def("mlp_layer_train_pool_bf16_grad(Tensor grad_out, Tensor arg, Tensor x, Tensor weight, "
        "Tensor y, Tensor? mean, Tensor? var, Tensor? gamma, Tensor? beta, float eps, bool relu, "
        "bool need_grad_x) -> "
        "(Tensor grad_x, Tensor grad_w, Tensor grad_b, Tensor grad_gamma, Tensor grad_beta)");
  m.def("attn_kv_train(Tensor x, Tensor wq, Tensor bq, Tensor wk, Tensor bk, Tensor wv, Tensor bv, "
        "bool add_max) -> (Tensor att, Tensor pmax, Tensor arg, Tensor q, Tensor kv)");
  m.def("attn_kv_train_grad(Tensor grad_att, Tensor? grad_pmax, Tensor arg, Tensor x, Tensor wq, "
        "Tensor wk, Tensor wv, Tensor q, Tensor kv, bool need_grad_x) -> "
        "(Tensor grad_x, Tensor grad_wq, Tensor grad_bq, Tensor grad_wk, Tensor grad_bk, "
        "Tensor grad_wv, Tensor grad_bv)");
  m.def("bn_train(Tensor x, Tensor gamma, Tensor beta, float eps, bool relu) -> "
        "(Tensor out, Tensor mean, Tensor var)");
  m.def("bn_train_grad(Tensor grad_out, Tensor x, Tensor mean, Tensor var, Tensor gamma, "
        "Tensor beta, float eps, bool relu) -> (Tensor grad_x, Tensor grad_gamma, Tensor grad_beta)");
  m.def("dropout(Tensor x, float keep_prob, int seed) -> Tensor");
  m.def("softmax_xent(Tensor logits, Tensor labels, Tensor? weights) -> "
        "(Tensor loss, Tensor lse, Tensor pred, Tensor num_present)");
  m.def("softmax_xent_grad(Tensor grad_loss, Tensor logits, Tensor labels, Tensor? weights, "
        "Tensor lse, Tensor num_present) -> Tensor");
  m.def("adam_step(Tensor(a!)[] params, Tensor[] grads, Tensor(b!)[] exp_avg, "
        "Tensor(c!)[] exp_avg_sq, float alpha, float beta1, float beta2, float epsilon) -> ()");
  m.def("seg_confusion(Tensor labels, Tensor pred, Tensor(a!) confusion, Tensor(b!) counts) -> ()");
  m.def("mean_iou(Tensor confusion) -> (Tensor, Tensor)");
  m.def("group_concat_train(Tensor xyz, Tensor? points, Tensor new_xyz, Tensor idx, bool use_xyz, "
        "bool xyz_last) -> Tensor");
  m.def("group_concat_train_grad(Tensor grad_new_points, Tensor idx, int N, int C, int col0) -> "
        "Tensor");
  m.def("fp_apply_train(Tensor dist, Tensor idx, Tensor? points1, Tensor points2) -> Tensor");
  m.def("fp_apply_train_grad(Tensor grad_out, Tensor dist, Tensor idx, int m, int C2, int C1) -> "
        "(Tensor, Tensor)");
  m.def("scene_vote(Tensor? logits, Tensor mask, Tensor orig, int row0, Tensor(a!) keys) -> Tensor");
  m.def("scene_labels(Tensor keys, Tensor? lut, int dflt) -> "
        "(Tensor labels, Tensor mapped, Tensor winner)");
  m.def("map_back_rows(Tensor values, int row0, Tensor keys, Tensor(a!) out) -> ()");
  m.def("label_lut(Tensor inp, Tensor lut, int dflt) -> Tensor");
  m.def("feed_batch(Tensor points, Tensor labels, Tensor? colors, Tensor? normals, "
        "Tensor sample_weight, Tensor? cs, Tensor class_weights, bool use_color, bool use_normal) "
        "-> (Tensor xyz, Tensor features, Tensor smpw)");
  m.def("val_select(Tensor points, Tensor bounds, float margin, float inner_margin) -> "
        "(Tensor counts, Tensor sel, Tensor inner)");
  m.def("render_ball(Tensor ixyz, Tensor? c0, Tensor? c1, Tensor? c2, Tensor? labels, "
        "Tensor? palette, int r, int h, int w, int[] background) -> Tensor");
  m.def("render_project(Tensor xyz, Tensor mats) -> Tensor");
  m.def("val_chunks(Tensor points, Tensor labels, Tensor? colors, Tensor? normals, Tensor counts, "
        "Tensor sel, Tensor inner, Tensor? choice, Tensor? u, int npoints, Tensor label_weights, "
        "float min_inside) -> (Tensor points, Tensor labels, Tensor colors, Tensor normals, "
        "Tensor weights, Tensor column, Tensor kept)");
}

// Each op's one body, registered under CUDA (ROCm builds of PyTorch dispatch HIP tensors under
// the CUDA key) and under Meta.
static void register_bodies(torch::Library& m) {
  m.impl("farthest_point_sample", &fps_hip);
  m.impl("farthest_point_sample_and_gather", &fps_and_gather_hip);
  m.impl("gather_point", &gather_point_hip);
  m.impl("gather_point_grad", &gather_point_grad_hip);
  m.impl("prob_sample", &prob_sample_hip);
  m.impl("query_ball_point", &query_ball_point_hip);
  m.impl("select_top_k", &select_top_k_hip);
  m.impl("knn_point", &knn_point_hip);
  m.impl("group_point", &group_point_hip);
  m.impl("group_point_grad", &group_point_grad_hip);
  m.impl("group_concat", &group_concat_hip);
  m.impl("three_nn", &three_nn_impl<true>);
  m.impl("three_interpolate", &three_interpolate_impl<true>);
  m.impl("three_interpolate_grad", &three_interpolate_grad_impl<true>);
  m.impl("idw_weights", &idw_weights_hip);
  m.impl("fp_fused", &fp_fused_hip);
  m.impl("attn_reduce", &attn_reduce_hip);
  m.impl("attn_reduce_grad", &attn_reduce_grad_hip);
  m.impl("attn_reduce_kd", &attn_reduce_kd_hip);
  m.impl("attn_reduce_kd_grad", &attn_reduce_kd_grad_hip);
  m.impl("head_mix", &head_mix_hip);
  m.impl("head_mix_grad", &head_mix_grad_hip);
  m.impl("group_pool", &group_pool_hip);
  m.impl("dense_wide", &dense_wide_hip);
  m.impl("mlp_layer_train", &mlp_layer_train_hip<false>);
  m.impl("mlp_layer_train_grad", &mlp_layer_train_grad_hip<false>);
  m.impl("mlp_layer_train_pool", &mlp_layer_train_pool_hip<false>);
  m.impl("mlp_layer_train_pool_grad", &mlp_layer_train_pool_grad_hip<false>);
  m.impl("mlp_layer_train_bf16", &mlp_layer_train_hip<true>);
  m.impl("mlp_layer_train_bf16_grad", &mlp_layer_train_grad_hip<true>);
  m.impl("mlp_layer_train_pool_bf16", &mlp_layer_train_pool_hip<true>);
  m.impl("mlp_layer_train_pool_bf16_grad", &mlp_layer_train_pool_grad_hip<true>);
  m.impl("attn_kv_train", &attn_kv_train_hip);
  m.impl("attn_kv_train_grad", &attn_kv_train_grad_hip);
  m.impl("bn_train", &bn_train_hip);
  m.impl("bn_train_grad", &bn_train_grad_hip);
  m.impl("dropout", &dropout_hip);
  m.impl("softmax_xent", &softmax_xent_hip);
  m.impl("softmax_xent_grad", &softmax_xent_grad_hip);
  m.impl("adam_step", &adam_step_hip);
  m.impl("seg_confusion", &seg_confusion_hip);
  m.impl("mean_iou", &mean_iou_hip);
  m.impl("group_concat_train", &group_concat_train_hip);
  m.impl("group_concat_train_grad", &group_concat_train_grad_hip);
  m.impl("fp_apply_train", &fp_apply_train_hip);
  m.impl("fp_apply_train_grad", &fp_apply_train_grad_hip);
  m.impl("scene_vote", &scene_vote_impl<true>);
  m.impl("scene_labels", &scene_labels_impl<true>);
  m.impl("map_back_rows", &map_back_rows_impl<true>);
  m.impl("label_lut", &label_lut_impl<true>);
  m.impl("feed_batch", &feed_batch_impl<true>);
  m.impl("val_select", &val_select_impl<true>);
  m.impl("val_chunks", &val_chunks_impl<true>);
  m.impl("render_ball", &render_ball_impl<true>);
  m.impl("render_project", &render_project_impl<true>);
}
TORCH_LIBRARY_IMPL(pn2, CUDA, m) { register_bodies(m); }
TORCH_LIBRARY_IMPL(pn2, Meta, m) { register_bodies(m); }

TORCH_LIBRARY_IMPL(pn2, Autograd, m) {
  m.impl("dropout", &dropout_autograd);
  m.impl("softmax_xent", &softmax_xent_autograd);
  m.impl("group_concat_train", &group_concat_train_autograd);
  m.impl("fp_apply_train", &fp_apply_train_autograd);
}

TORCH_LIBRARY_IMPL(pn2, CPU, m) {
  m.impl("three_nn", &three_nn_impl<false>);
  m.impl("three_interpolate", &three_interpolate_impl<false>);
  m.impl("three_interpolate_grad", &three_interpolate_grad_impl<false>);
  // the prediction ops' host twins (csrc/cpu_predict.cpp)
  m.impl("scene_vote", &scene_vote_impl<false>);
  m.impl("scene_labels", &scene_labels_impl<false>);
  m.impl("map_back_rows", &map_back_rows_impl<false>);
  m.impl("label_lut", &label_lut_impl<false>);
  // the training feed's host twins (csrc/cpu_feed.cpp)
  m.impl("feed_batch", &feed_batch_impl<false>);
  m.impl("val_select", &val_select_impl<false>);
  m.impl("val_chunks", &val_chunks_impl<false>);
  // scene rendering's host twins (csrc/cpu_render.cpp)
  m.impl("render_ball", &render_ball_impl<false>);
  m.impl("render_project", &render_project_impl<false>);
}
