// What stands between a stored crop and train_step (attention_points/train.py:74-109,
// scannet_dataset/data_transformation.py:270-352), gfx950.
//
//  - pn2_feed_batch: get_data_tensors (train.py:94-108) and random_rotate
//    (data_transformation.py:334-352) of a whole batch in ONE launch: colours / 255, the
//    colour ++ normal concatenation, the class-weight look-up times the stored weight's
//    non-zero mask, and the rotation about z of the points and the normals. One thread per row,
//    grid-stride over B * N rows with 64-bit offsets. Every access is one 4-byte element, so
//    any 4-byte aligned pointer is taken and the bits do not depend on the alignment.
//  - pn2_val_chunks: the part of get_all_subsets_for_scene_numpy (:270-331) after the column
//    selection (pn2_val_select, scene.hip): the npoints draws of every non-empty column, the
//    mask sum that decides whether the chunk is kept (:317), and the gathers of the kept chunks,
//    compacted in column order. Three launches: per-column mask sums (integer adds), one scan
//    over the S columns, the gather into each chunk's slot. No float atomics and nothing that
//    depends on the launch order: the output is reproducible bit for bit.
// The arithmetic is fixed operation by operation (no contraction), so the host twins of
// cpu_feed.cpp give the same bits.
#include "common.h"

namespace pn2 {
namespace {

constexpr int kBlock = 256;
constexpr int kFeedMaxBlocks = 1024;

// label_weights[label], 0 outside the table (crop_gather_kernel's rule, scene.hip)
PN2_DEV float weight_of(int lab, const float* __restrict__ w, int L) {
  return lab >= 0 && lab < L ? w[lab] : 0.0f;
}

// row vector times [[c, -s, 0], [s, c, 0], [0, 0, 1]] (:348-351): x' = x c + y s,
// y' = y c - x s, each product rounded, then the sum
PN2_DEV void rotate_z(float x, float y, float c, float s, float* ox, float* oy) {
  const float xc = __fmul_rn(x, c), ys = __fmul_rn(y, s);
  const float yc = __fmul_rn(y, c), xs = __fmul_rn(x, s);
  *ox = __fadd_rn(xc, ys);
  *oy = __fsub_rn(yc, xs);
}

__global__ __launch_bounds__(kBlock) void feed_batch_kernel(
    const float* __restrict__ points, const int32_t* __restrict__ labels,
    const int32_t* __restrict__ colors, const float* __restrict__ normals,
    const float* __restrict__ sample_weight, const float* __restrict__ cs,
    const float* __restrict__ class_weights, int L, long long rows, int N, int use_color,
    int use_normal, float* __restrict__ xyz, float* __restrict__ features,
    float* __restrict__ smpw) {
  const int F = (use_color ? 3 : 0) + (use_normal ? 3 : 0);
  for (long long r = (long long)blockIdx.x * kBlock + threadIdx.x; r < rows;
       r += (long long)gridDim.x * kBlock) {
    float c = 1.0f, s = 0.0f;
    if (cs) {
      const long long b = r / N;
      c = cs[b * 2];
      s = cs[b * 2 + 1];
    }
    float x = points[r * 3], y = points[r * 3 + 1];
    if (cs) rotate_z(x, y, c, s, &x, &y);
    xyz[r * 3] = x;
    xyz[r * 3 + 1] = y;
    xyz[r * 3 + 2] = points[r * 3 + 2];
    float* f = features + r * F;
    if (use_color) {
#pragma unroll
      for (int k = 0; k < 3; ++k) f[k] = __fdiv_rn((float)colors[r * 3 + k], 255.0f);
      f += 3;
    }
    if (use_normal) {
      float nx = normals[r * 3], ny = normals[r * 3 + 1];
      if (cs) rotate_z(nx, ny, c, s, &nx, &ny);
      f[0] = nx;
      f[1] = ny;
      f[2] = normals[r * 3 + 2];
    }
    // tf.not_equal(sample_weight, 0.0) (train.py:106): -0.0 equals 0, NaN does not
    const float m = sample_weight[r] != 0.0f ? 1.0f : 0.0f;
    smpw[r] = __fmul_rn(weight_of(labels[r], class_weights, L), m);
  }
}

// a column's point count; never more than the scene has, whatever `counts` holds
PN2_DEV int col_n(const int32_t* __restrict__ counts, int s, int N) { return min(counts[s], N); }

// draw r of a column with n points: choice[r] clamped, or the crop sampler's int(u * n)
PN2_DEV int draw_of(const int32_t* __restrict__ choice, const float* __restrict__ u, size_t at,
                    int n) {
  const int k = choice ? choice[at] : (int)__fmul_rn(u[at], (float)n);
  return min(max(k, 0), n - 1);
}

// msum[s] = the number of column s's K draws that land inside the column (mask = inner)
__global__ __launch_bounds__(kBlock) void val_mask_sum_kernel(
    const int32_t* __restrict__ counts, const uint8_t* __restrict__ inner, int N,
    const int32_t* __restrict__ choice, const float* __restrict__ u, int K,
    int32_t* __restrict__ msum) {
  const int s = blockIdx.x;
  const int n = col_n(counts, s, N);
  __shared__ int sh;
  if (threadIdx.x == 0) sh = 0;
  __syncthreads();
  int m = 0;
  if (n > 0)
    for (int r = threadIdx.x; r < K; r += kBlock)
      m += inner[(size_t)s * N + draw_of(choice, u, (size_t)s * K + r, n)] ? 1 : 0;
  atomicAdd(&sh, m);  // integers: any order gives the same sum
  __syncthreads();
  if (threadIdx.x == 0) msum[s] = sh;
}

// One thread walks the S columns in order: column[j] = the j-th kept column, -1 past the kept
// ones. A column is kept when it has points and not sum(mask) / K < min_inside (:307, :317).
__global__ void val_scan_kernel(const int32_t* __restrict__ counts,
                                const int32_t* __restrict__ msum, int S, int N, int K,
                                double min_inside,
                                int32_t* __restrict__ column, int32_t* __restrict__ kept) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int j = 0;
  for (int s = 0; s < S; ++s)
    if (col_n(counts, s, N) > 0 && !((double)msum[s] / (double)K < min_inside)) column[j++] = s;
  *kept = j;
  for (; j < S; ++j) column[j] = -1;
}

// Slot j of the output: the gathered chunk of column[j], zeros past the kept chunks.
__global__ __launch_bounds__(kBlock) void val_gather_kernel(
    const float* __restrict__ p, const int32_t* __restrict__ labels,
    const int32_t* __restrict__ colors, const float* __restrict__ normals, int N,
    const int32_t* __restrict__ counts, const int32_t* __restrict__ sel,
    const uint8_t* __restrict__ inner, const int32_t* __restrict__ choice,
    const float* __restrict__ u, int K, const float* __restrict__ label_weights, int L,
    const int32_t* __restrict__ column, float* __restrict__ op, int32_t* __restrict__ ol,
    int32_t* __restrict__ oc, float* __restrict__ on, float* __restrict__ ow) {
  const int j = blockIdx.y;
  const int r = blockIdx.x * kBlock + threadIdx.x;
  if (r >= K) return;
  const size_t o = (size_t)j * K + r;
  const int s = column[j];
  if (s < 0) {
    for (int c = 0; c < 3; ++c) {
      op[o * 3 + c] = 0.0f;
      if (oc) oc[o * 3 + c] = 0;
      if (on) on[o * 3 + c] = 0.0f;
    }
    ol[o] = 0;
    ow[o] = 0.0f;
    return;
  }
  const int k = draw_of(choice, u, (size_t)s * K + r, col_n(counts, s, N));
  int i = sel[(size_t)s * N + k];
  i = min(max(i, 0), N - 1);  // sel comes from pn2_val_select; a foreign one cannot index out
  for (int c = 0; c < 3; ++c) {
    op[o * 3 + c] = p[(size_t)i * 3 + c];
    if (oc) oc[o * 3 + c] = colors[(size_t)i * 3 + c];
    if (on) on[o * 3 + c] = normals[(size_t)i * 3 + c];
  }
  const int lab = labels[i];
  ol[o] = lab;
  const float m = inner[(size_t)s * N + k] ? 1.0f : 0.0f;
  ow[o] = __fmul_rn(weight_of(lab, label_weights, L), m);
}

}  // namespace
}  // namespace pn2

extern "C" {

int pn2_feed_batch(const float* points, const int32_t* labels, const int32_t* colors,
                   const float* normals, const float* sample_weight, const float* cs,
                   const float* class_weights, int L, int B, int N, int use_color,
                   int use_normal, float* xyz, float* features, float* smpw,
                   pn2_stream_t stream) {
  using namespace pn2;
  if (B < 0 || N < 0 || L < 0) return PN2_EINVAL;
  const long long rows = (long long)B * N;
  if (rows == 0) return PN2_OK;
  if (!points || !labels || !sample_weight || !xyz || !smpw) return PN2_EINVAL;
  if ((L > 0 && !class_weights) || (use_color && !colors) || (use_normal && !normals))
    return PN2_EINVAL;
  if ((use_color || use_normal) && !features) return PN2_EINVAL;
  long long blocks = (rows + kBlock - 1) / kBlock;
  if (blocks > kFeedMaxBlocks) blocks = kFeedMaxBlocks;
  hipLaunchKernelGGL(feed_batch_kernel, dim3((unsigned)blocks), dim3(kBlock), 0,
                     (hipStream_t)stream, points, labels, colors, normals, sample_weight, cs,
                     class_weights, L, rows, N, use_color ? 1 : 0, use_normal ? 1 : 0, xyz,
                     features, smpw);
  PN2_RETURN_LAUNCH();
}

size_t pn2_val_chunks_workspace_size(int S) { return S > 0 ? (size_t)S * sizeof(int32_t) : 0; }

int pn2_val_chunks(const float* points, const int32_t* labels, const int32_t* colors,
                   const float* normals, int N, const int32_t* counts, const int32_t* sel,
                   const uint8_t* inner, int S, const int32_t* choice, const float* u, int K,
                   const float* label_weights, int L, double min_inside, void* workspace,
                   size_t workspace_bytes, float* out_points, int32_t* out_labels,
                   int32_t* out_colors, float* out_normals, float* out_weights, int32_t* column,
                   int32_t* kept, pn2_stream_t stream) {
  using namespace pn2;
  if (N < 0 || S < 0 || K < 0 || L < 0) return PN2_EINVAL;
  if ((long long)N * S > 0x7fffffffLL || (long long)K * S > 0x7fffffffLL || S > 65535)
    return PN2_EINVAL;
  if (!kept) return PN2_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (S == 0) {
    if (hipMemsetAsync(kept, 0, sizeof(int32_t), st) != hipSuccess) return (int)hipGetLastError();
    return PN2_OK;
  }
  if (!counts || !column || !workspace || (L > 0 && !label_weights)) return PN2_EINVAL;
  if (workspace_bytes < pn2_val_chunks_workspace_size(S)) return PN2_EINVAL;
  if (N > 0 && (!points || !labels || !sel || !inner)) return PN2_EINVAL;
  if (K > 0 && ((!choice && !u) || !out_points || !out_labels || !out_weights))
    return PN2_EINVAL;
  if ((colors && !out_colors) || (normals && !out_normals)) return PN2_EINVAL;
  int32_t* msum = static_cast<int32_t*>(workspace);
  hipLaunchKernelGGL(val_mask_sum_kernel, dim3((unsigned)S), dim3(kBlock), 0, st, counts, inner, N,
                     choice, u, K, msum);
  hipLaunchKernelGGL(val_scan_kernel, dim3(1), dim3(kWave), 0, st, counts, msum, S, N, K, min_inside,
                     column, kept);
  if (K > 0)
    hipLaunchKernelGGL(val_gather_kernel, dim3((unsigned)((K + kBlock - 1) / kBlock), (unsigned)S),
                       dim3(kBlock), 0, st, points, labels, colors, normals, N, counts, sel, inner,
                       choice, u, K, label_weights, L, column, out_points, out_labels,
                       colors ? out_colors : nullptr, normals ? out_normals : nullptr,
                       out_weights);
  PN2_RETURN_LAUNCH();
}

}  // extern "C"
