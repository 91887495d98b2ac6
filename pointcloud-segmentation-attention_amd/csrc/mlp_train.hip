// Training-mode shared-MLP layer (tf_util.conv2d / conv1d with is_training=True,
// tf_util.py:165-185; batch norm on batch statistics, :512-531), gfx950.
//
//   forward    y = x W + b            pn2_shared_mlp (mlp.hip) over a pn2_mlp_pack of W, b
//              mean, var = stats(y)   pn2_bn_stats     (biased variance)
//              out = act(bn(y))       pn2_bn_act_fwd
//   backward   grad_y, grad_gamma, grad_beta = pn2_bn_act_bwd(grad_out, y, ...)
//              grad_w = x^T grad_y    pn2_mlp_wgrad    (fp32 matrix cores)
//              grad_x = grad_y W^T    pn2_shared_mlp over a pn2_mlp_pack of W^T
//   last layer of a set-abstraction MLP, fused with the max pool over the ns samples of a group
//   (y is (groups, ns, C)):
//              out, arg = max_j act(bn(y))                        pn2_bn_act_pool_fwd
//              grad_y, grad_gamma, grad_beta from (groups, C) grad_out  pn2_bn_act_pool_bwd
//
// Reductions are two-stage and ordered: stage 1 writes one partial per workgroup, stage 2
// combines the partials in a fixed order in double precision. No floating-point atomics, so
// two runs give the same bits.
//
// Per-channel kernels (stats, activation, its backward) share one layout: a workgroup owns 32
// channels and a block of rows; thread (cl = tid & 31, rl = tid >> 5) walks rows rl, rl + 8,
// ... of channel cl, eight rows per step (eight independent loads), so a wave's load covers
// two 128-byte row segments and the channel's constants stay in registers.
//
// pn2_mlp_wgrad: v_mfma_f32_32x32x2_f32 takes A[i = lane & 31][k = lane >> 5] and
// B[k = lane >> 5][j = lane & 31]; with i = input channel, j = output channel and k = row, a
// wave that owns a 32x32 (cin, cout) tile loads x[r + (lane >> 5)][ci0 + (lane & 31)] and
// grad_y[r + (lane >> 5)][co0 + (lane & 31)]: two row segments straight from the row-major
// tensors, no transpose. The four waves of a workgroup interleave the row pairs of a slab and
// their accumulators are added through LDS in wave order.
#include "common.h"

namespace pn2 {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kBlock = 256;
constexpr int kCols = 32;                    // channels per workgroup
constexpr int kRowLanes = kBlock / kCols;    // 8
constexpr int kBatch = 8;                    // rows per thread per step
constexpr int kStep = kRowLanes * kBatch;    // 64 rows per workgroup step
constexpr int kStatRows = PN2_BN_BLOCK_ROWS;  // rows per stage-1 partial (stats, bwd sums)
constexpr int kActRows = 256;                 // rows per workgroup of the element-wise passes
constexpr int kPoolGroups = PN2_BN_POOL_BLOCK_GROUPS;  // groups per stage-1 partial (pool bwd)
constexpr int kPoolSplit = 64;                // above this ns a group is split across row lanes
constexpr int kSlab = PN2_WGRAD_SLAB_ROWS;
constexpr int kTile = 32 * 32;

// gamma / sqrt(var + eps) and the pre-activation, written once: the forward pass and the
// backward mask must round identically.
PN2_DEV float bn_scale(float gamma, float var, float eps) {
  return __fdiv_rn(gamma, __fsqrt_rn(__fadd_rn(var, eps)));
}
PN2_DEV float bn_pre(float y, float mean, float s, float beta) {
  return __fadd_rn(__fmul_rn(__fsub_rn(y, mean), s), beta);
}

// Chan et al.: (na, ma, M2a) <- (na, ma, M2a) + (nb, mb, M2b)
template <typename T>
PN2_DEV void chan_merge(T& na, T& ma, T& M2a, T nb, T mb, T M2b) {
  if (nb == T(0)) return;
  const T n = na + nb;
  const T d = mb - ma;
  const T f = nb / n;
  ma = ma + d * f;
  M2a = M2a + M2b + d * d * (na * f);
  na = n;
}

PN2_DEV int block_rows(long long rows, long long r0, int per) {
  const long long left = rows - r0;
  return left < per ? (int)left : per;
}

// ---------------------------------------------------------------- batch statistics ------
// stage 1: part[(blk * 2 + 0) * C + c] = mean, [(blk * 2 + 1) * C + c] = M2 of block blk
__global__ __launch_bounds__(kBlock) void bn_stats_partial(const float* __restrict__ y,
                                                           long long rows, int C,
                                                           float* __restrict__ part) {
  __shared__ float sh[3][kRowLanes][kCols];
  const int cl = threadIdx.x & (kCols - 1), rl = threadIdx.x / kCols;
  const int c = blockIdx.y * kCols + cl;
  const long long r0 = (long long)blockIdx.x * kStatRows;
  const int nr = block_rows(rows, r0, kStatRows);
  float n = 0.f, mean = 0.f, m2 = 0.f;
  if (c < C) {
    const float* p = y + r0 * C + c;
    for (int base = 0; base + rl < nr; base += kStep) {
      float v[kBatch];
      int cnt = 0;
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const int r = base + rl + kRowLanes * u;
        const bool ok = r < nr;
        v[u] = ok ? p[(long long)r * C] : 0.f;
        cnt += ok ? 1 : 0;
      }
      float s = 0.f;
#pragma unroll
      for (int u = 0; u < kBatch; ++u) s += v[u];
      const float mb = s / (float)cnt;
      float qb = 0.f;
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const float d = v[u] - mb;
        qb += (base + rl + kRowLanes * u < nr) ? d * d : 0.f;
      }
      chan_merge(n, mean, m2, (float)cnt, mb, qb);
    }
  }
  sh[0][rl][cl] = n;
  sh[1][rl][cl] = mean;
  sh[2][rl][cl] = m2;
  __syncthreads();
  if (rl == 0 && c < C) {
    for (int g = 1; g < kRowLanes; ++g) chan_merge(n, mean, m2, sh[0][g][cl], sh[1][g][cl], sh[2][g][cl]);
    part[((size_t)blockIdx.x * 2 + 0) * C + c] = mean;
    part[((size_t)blockIdx.x * 2 + 1) * C + c] = m2;
  }
}

// stage 2: one workgroup per 32 channels; row lane g merges blocks g, g + 8, ... in double,
// then lane 0 merges the eight.
__global__ __launch_bounds__(kBlock) void bn_stats_final(const float* __restrict__ part,
                                                         long long rows, int C, int nblk,
                                                         float* __restrict__ mean_out,
                                                         float* __restrict__ var_out) {
  __shared__ double sh[3][kRowLanes][kCols];
  const int cl = threadIdx.x & (kCols - 1), g = threadIdx.x / kCols;
  const int c = blockIdx.x * kCols + cl;
  double n = 0.0, mean = 0.0, m2 = 0.0;
  if (c < C) {
    for (int b = g; b < nblk; b += kRowLanes) {
      const double nb = (double)block_rows(rows, (long long)b * kStatRows, kStatRows);
      chan_merge(n, mean, m2, nb, (double)part[((size_t)b * 2 + 0) * C + c],
                 (double)part[((size_t)b * 2 + 1) * C + c]);
    }
  }
  sh[0][g][cl] = n;
  sh[1][g][cl] = mean;
  sh[2][g][cl] = m2;
  __syncthreads();
  if (g == 0 && c < C) {
    for (int k = 1; k < kRowLanes; ++k) chan_merge(n, mean, m2, sh[0][k][cl], sh[1][k][cl], sh[2][k][cl]);
    mean_out[c] = (float)mean;
    var_out[c] = (float)(m2 / n);
  }
}

// ---------------------------------------------------------------- activation forward ----
template <bool BN>
__global__ __launch_bounds__(kBlock) void bn_act_fwd_kernel(
    const float* __restrict__ y, long long rows, int C, const float* __restrict__ mean,
    const float* __restrict__ var, const float* __restrict__ gamma,
    const float* __restrict__ beta, float eps, int relu, float* __restrict__ out) {
  const int cl = threadIdx.x & (kCols - 1), rl = threadIdx.x / kCols;
  const int c = blockIdx.y * kCols + cl;
  if (c >= C) return;
  const long long r0 = (long long)blockIdx.x * kActRows;
  const int nr = block_rows(rows, r0, kActRows);
  float m = 0.f, s = 1.f, b = 0.f;
  if (BN) {
    m = mean[c];
    s = bn_scale(gamma[c], var[c], eps);
    b = beta[c];
  }
  const float* p = y + r0 * C + c;
  float* o = out + r0 * C + c;
  for (int base = 0; base + rl < nr; base += kStep) {
    float v[kBatch];
#pragma unroll
    for (int u = 0; u < kBatch; ++u) {
      const int r = base + rl + kRowLanes * u;
      v[u] = r < nr ? p[(long long)r * C] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < kBatch; ++u) {
      const int r = base + rl + kRowLanes * u;
      const float pre = BN ? bn_pre(v[u], m, s, b) : v[u];
      if (r < nr) o[(long long)r * C] = relu ? fmaxf(pre, 0.f) : pre;
    }
  }
}

// ---------------------------------------------------------------- activation backward ---
// stage 1 of the sums: part[(blk * 2 + 0) * C + c] = sum dz, [(blk * 2 + 1) * C + c] =
// sum dz * xhat over block blk. Without batch norm grad_y = dz is written here.
template <bool BN>
__global__ __launch_bounds__(kBlock) void bn_bwd_partial(
    const float* __restrict__ go, const float* __restrict__ y, long long rows, int C,
    const float* __restrict__ mean, const float* __restrict__ var,
    const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int relu,
    float* __restrict__ grad_y, float* __restrict__ part) {
  __shared__ float sh[2][kRowLanes][kCols];
  const int cl = threadIdx.x & (kCols - 1), rl = threadIdx.x / kCols;
  const int c = blockIdx.y * kCols + cl;
  const long long r0 = (long long)blockIdx.x * kStatRows;
  const int nr = block_rows(rows, r0, kStatRows);
  float db = 0.f, dg = 0.f;
  if (c < C) {
    float m = 0.f, s = 1.f, b = 0.f, rstd = 1.f;
    if (BN) {
      m = mean[c];
      s = bn_scale(gamma[c], var[c], eps);
      b = beta[c];
      rstd = __fdiv_rn(1.f, __fsqrt_rn(__fadd_rn(var[c], eps)));
    }
    const float* py = y + r0 * C + c;
    const float* pg = go + r0 * C + c;
    float* pd = BN ? nullptr : grad_y + r0 * C + c;
    const bool need_y = BN || relu;  // no batch norm, no ReLU: grad_y = grad_out, y is not read
    for (int base = 0; base + rl < nr; base += kStep) {
      float v[kBatch], g[kBatch];
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const int r = base + rl + kRowLanes * u;
        const bool ok = r < nr;
        v[u] = (ok && need_y) ? py[(long long)r * C] : 0.f;
        g[u] = ok ? pg[(long long)r * C] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const int r = base + rl + kRowLanes * u;
        const float pre = BN ? bn_pre(v[u], m, s, b) : v[u];
        const float dz = (r < nr && (!relu || pre > 0.f)) ? g[u] : 0.f;
        db += dz;
        if (BN) dg += dz * ((v[u] - m) * rstd);
        else if (r < nr) pd[(long long)r * C] = dz;
      }
    }
  }
  sh[0][rl][cl] = db;
  sh[1][rl][cl] = dg;
  __syncthreads();
  if (rl == 0 && c < C) {
    for (int k = 1; k < kRowLanes; ++k) {
      db += sh[0][k][cl];
      dg += sh[1][k][cl];
    }
    part[((size_t)blockIdx.x * 2 + 0) * C + c] = db;
    part[((size_t)blockIdx.x * 2 + 1) * C + c] = dg;
  }
}

// stage 2: block sums added in double, in the order of bn_stats_final
__global__ __launch_bounds__(kBlock) void bn_bwd_final(const float* __restrict__ part, int C,
                                                       int nblk, float* __restrict__ grad_gamma,
                                                       float* __restrict__ grad_beta) {
  __shared__ double sh[2][kRowLanes][kCols];
  const int cl = threadIdx.x & (kCols - 1), g = threadIdx.x / kCols;
  const int c = blockIdx.x * kCols + cl;
  double db = 0.0, dg = 0.0;
  if (c < C) {
    for (int b = g; b < nblk; b += kRowLanes) {
      db += (double)part[((size_t)b * 2 + 0) * C + c];
      dg += (double)part[((size_t)b * 2 + 1) * C + c];
    }
  }
  sh[0][g][cl] = db;
  sh[1][g][cl] = dg;
  __syncthreads();
  if (g == 0 && c < C) {
    for (int k = 1; k < kRowLanes; ++k) {
      db += sh[0][k][cl];
      dg += sh[1][k][cl];
    }
    grad_beta[c] = (float)db;
    if (grad_gamma) grad_gamma[c] = (float)dg;
  }
}

// grad_y = gamma / sigma * (dz - grad_beta / R - xhat * grad_gamma / R)
__global__ __launch_bounds__(kBlock) void bn_bwd_apply(
    const float* __restrict__ go, const float* __restrict__ y, long long rows, int C,
    const float* __restrict__ mean, const float* __restrict__ var,
    const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int relu,
    const float* __restrict__ grad_gamma, const float* __restrict__ grad_beta,
    float* __restrict__ grad_y) {
  const int cl = threadIdx.x & (kCols - 1), rl = threadIdx.x / kCols;
  const int c = blockIdx.y * kCols + cl;
  if (c >= C) return;
  const long long r0 = (long long)blockIdx.x * kActRows;
  const int nr = block_rows(rows, r0, kActRows);
  const float m = mean[c], b = beta[c];
  const float s = bn_scale(gamma[c], var[c], eps);
  const float rstd = __fdiv_rn(1.f, __fsqrt_rn(__fadd_rn(var[c], eps)));
  const float inv_rows = (float)(1.0 / (double)rows);
  const float mb = grad_beta[c] * inv_rows, mg = grad_gamma[c] * inv_rows;
  const float* py = y + r0 * C + c;
  const float* pg = go + r0 * C + c;
  float* pd = grad_y + r0 * C + c;
  for (int base = 0; base + rl < nr; base += kStep) {
    float v[kBatch], g[kBatch];
#pragma unroll
    for (int u = 0; u < kBatch; ++u) {
      const int r = base + rl + kRowLanes * u;
      const bool ok = r < nr;
      v[u] = ok ? py[(long long)r * C] : 0.f;
      g[u] = ok ? pg[(long long)r * C] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < kBatch; ++u) {
      const int r = base + rl + kRowLanes * u;
      const float pre = bn_pre(v[u], m, s, b);
      const float dz = (!relu || pre > 0.f) ? g[u] : 0.f;
      const float xhat = (v[u] - m) * rstd;
      if (r < nr) pd[(long long)r * C] = s * ((dz - mb) - xhat * mg);
    }
  }
}

// ---------------------------------------------------------------- activation + max pool --
// The last layer of a set-abstraction MLP: out[g][c] = max_j act(bn(y[g][j][c])) over the ns
// samples of group g, arg = the lowest j that attains it. The max is taken over the
// activation, never over y: gamma may be negative, so bn can be decreasing in y. Candidates are
// visited in ascending j and replace the best only on a strict >, so ties keep the lowest j:
// an all-zero group gives arg 0, and the rows a ball query pads with copies of its first
// neighbour (j = 0) never win.
//
// Two layouts, picked by ns on the host:
//   groups (ns <= kPoolSplit): thread (cl, rl) owns whole groups rl, rl + 8, ... of the
//     workgroup's block and walks their samples eight at a time; nothing crosses lanes.
//   split  (ns >  kPoolSplit): a workgroup owns one group; row lane rl walks samples rl,
//     rl + 8, ... and the eight lanes' (value, j) pairs are combined through LDS by
//     (value descending, j ascending). Parallelism is groups x channel tiles x 256 threads, so
//     group_all (groups = B, ns = N) still fills the row lanes.
PN2_DEV float pool_act(float pre, int relu) { return relu ? fmaxf(pre, 0.f) : pre; }

template <bool BN>
__global__ __launch_bounds__(kBlock) void bn_act_pool_fwd_groups(
    const float* __restrict__ y, long long groups, int ns, int C, int gpt,
    const float* __restrict__ mean, const float* __restrict__ var,
    const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int relu,
    float* __restrict__ out, int* __restrict__ arg) {
  const int cl = threadIdx.x & (kCols - 1), rl = threadIdx.x / kCols;
  const int c = blockIdx.y * kCols + cl;
  if (c >= C) return;
  float m = 0.f, s = 1.f, b = 0.f;
  if (BN) {
    m = mean[c];
    s = bn_scale(gamma[c], var[c], eps);
    b = beta[c];
  }
  const long long g0 = (long long)blockIdx.x * (kRowLanes * gpt);
  for (int t = 0; t < gpt; ++t) {
    const long long g = g0 + rl + kRowLanes * t;
    if (g >= groups) break;
    const float* p = y + g * ns * C + c;
    float best = 0.f;
    int bj = 0;
    for (int base = 0; base < ns; base += kBatch) {
      float v[kBatch];
#pragma unroll
      for (int u = 0; u < kBatch; ++u) v[u] = base + u < ns ? p[(long long)(base + u) * C] : 0.f;
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const int j = base + u;
        const float a = pool_act(BN ? bn_pre(v[u], m, s, b) : v[u], relu);
        if (j < ns && (j == 0 || a > best)) {
          best = a;
          bj = j;
        }
      }
    }
    out[g * C + c] = best;
    arg[g * C + c] = bj;
  }
}

template <bool BN>
__global__ __launch_bounds__(kBlock) void bn_act_pool_fwd_split(
    const float* __restrict__ y, int ns, int C, const float* __restrict__ mean,
    const float* __restrict__ var, const float* __restrict__ gamma,
    const float* __restrict__ beta, float eps, int relu, float* __restrict__ out,
    int* __restrict__ arg) {
  __shared__ float shv[kRowLanes][kCols];
  __shared__ int shj[kRowLanes][kCols];
  const int cl = threadIdx.x & (kCols - 1), rl = threadIdx.x / kCols;
  const int c = blockIdx.y * kCols + cl;
  const long long g = blockIdx.x;
  float best = 0.f;
  int bj = -1;  // no sample seen yet
  if (c < C) {
    float m = 0.f, s = 1.f, b = 0.f;
    if (BN) {
      m = mean[c];
      s = bn_scale(gamma[c], var[c], eps);
      b = beta[c];
    }
    const float* p = y + g * ns * C + c;
    for (int base = 0; base + rl < ns; base += kStep) {
      float v[kBatch];
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const int j = base + rl + kRowLanes * u;
        v[u] = j < ns ? p[(long long)j * C] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const int j = base + rl + kRowLanes * u;
        const float a = pool_act(BN ? bn_pre(v[u], m, s, b) : v[u], relu);
        if (j < ns && (bj < 0 || a > best)) {
          best = a;
          bj = j;
        }
      }
    }
  }
  shv[rl][cl] = best;
  shj[rl][cl] = bj;
  __syncthreads();
  if (rl == 0 && c < C) {  // row lane 0 holds j = 0, so bj >= 0 here
    for (int k = 1; k < kRowLanes; ++k) {
      const float v = shv[k][cl];
      const int j = shj[k][cl];
      if (j >= 0 && (v > best || (v == best && j < bj))) {
        best = v;
        bj = j;
      }
    }
    out[g * C + c] = best;
    arg[g * C + c] = bj;
  }
}

// backward, stage 1 of the sums: dz is grad_out[g][c] at j = arg[g][c] (masked by the
// recomputed pre-activation) and 0 elsewhere, so the sums read one gathered y element per
// (group, channel). part[(blk * 2 + 0) * C + c] = sum dz, [(blk * 2 + 1) * C + c] = sum dz *
// xhat over the kPoolGroups groups of block blk; stage 2 is bn_bwd_final. An arg outside
// [0, ns) selects nothing.
template <bool BN>
__global__ __launch_bounds__(kBlock) void bn_pool_bwd_partial(
    const float* __restrict__ go, const int* __restrict__ arg, const float* __restrict__ y,
    long long groups, int ns, int C, const float* __restrict__ mean,
    const float* __restrict__ var, const float* __restrict__ gamma,
    const float* __restrict__ beta, float eps, int relu, float* __restrict__ part) {
  __shared__ float sh[2][kRowLanes][kCols];
  const int cl = threadIdx.x & (kCols - 1), rl = threadIdx.x / kCols;
  const int c = blockIdx.y * kCols + cl;
  const long long g0 = (long long)blockIdx.x * kPoolGroups;
  const int ng = block_rows(groups, g0, kPoolGroups);
  float db = 0.f, dg = 0.f;
  if (c < C) {
    float m = 0.f, s = 1.f, b = 0.f, rstd = 1.f;
    if (BN) {
      m = mean[c];
      s = bn_scale(gamma[c], var[c], eps);
      b = beta[c];
      rstd = __fdiv_rn(1.f, __fsqrt_rn(__fadd_rn(var[c], eps)));
    }
    const bool need_y = BN || relu;
    for (int base = 0; base + rl < ng; base += kStep) {
      float v[kBatch], gr[kBatch];
      int a[kBatch];
      bool ok[kBatch];
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const int r = base + rl + kRowLanes * u;
        const bool in = r < ng;
        a[u] = in ? arg[(g0 + r) * C + c] : -1;
        gr[u] = in ? go[(g0 + r) * C + c] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const int r = base + rl + kRowLanes * u;
        ok[u] = a[u] >= 0 && a[u] < ns;
        v[u] = (ok[u] && need_y) ? y[((g0 + r) * ns + a[u]) * C + c] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const float pre = BN ? bn_pre(v[u], m, s, b) : v[u];
        const float dz = (ok[u] && (!relu || pre > 0.f)) ? gr[u] : 0.f;
        db += dz;
        if (BN) dg += dz * ((v[u] - m) * rstd);
      }
    }
  }
  sh[0][rl][cl] = db;
  sh[1][rl][cl] = dg;
  __syncthreads();
  if (rl == 0 && c < C) {
    for (int k = 1; k < kRowLanes; ++k) {
      db += sh[0][k][cl];
      dg += sh[1][k][cl];
    }
    part[((size_t)blockIdx.x * 2 + 0) * C + c] = db;
    part[((size_t)blockIdx.x * 2 + 1) * C + c] = dg;
  }
}

// per-channel constants of the apply pass and its element: bn_bwd_apply's expression with dz
// non-zero only at j = arg; without batch norm grad_y = dz
struct PoolApply {
  float m, s, b, rstd, mb, mg;
};
template <bool BN>
PN2_DEV PoolApply pool_apply_consts(int c, long long rows, const float* mean, const float* var,
                                    const float* gamma, const float* beta, float eps,
                                    const float* grad_gamma, const float* grad_beta) {
  PoolApply k = {0.f, 1.f, 0.f, 1.f, 0.f, 0.f};
  if (BN) {
    k.m = mean[c];
    k.b = beta[c];
    k.s = bn_scale(gamma[c], var[c], eps);
    k.rstd = __fdiv_rn(1.f, __fsqrt_rn(__fadd_rn(var[c], eps)));
    const float inv_rows = (float)(1.0 / (double)rows);
    k.mb = grad_beta[c] * inv_rows;
    k.mg = grad_gamma[c] * inv_rows;
  }
  return k;
}
template <bool BN>
PN2_DEV float pool_apply(const PoolApply& k, float v, bool hit, float g, int relu) {
  const float pre = BN ? bn_pre(v, k.m, k.s, k.b) : v;
  const float dz = (hit && (!relu || pre > 0.f)) ? g : 0.f;
  if (!BN) return dz;
  const float xhat = (v - k.m) * k.rstd;
  return k.s * ((dz - k.mb) - xhat * k.mg);
}

// backward, apply pass, the forward's two layouts. split: blockIdx.x = group * nchunk + chunk
// of kActRows samples (no combine here, so a group may span workgroups).
template <bool BN>
__global__ __launch_bounds__(kBlock) void bn_pool_bwd_apply_groups(
    const float* __restrict__ go, const int* __restrict__ arg, const float* __restrict__ y,
    long long groups, int ns, int C, int gpt, const float* __restrict__ mean,
    const float* __restrict__ var, const float* __restrict__ gamma,
    const float* __restrict__ beta, float eps, int relu, const float* __restrict__ grad_gamma,
    const float* __restrict__ grad_beta, float* __restrict__ grad_y) {
  const int cl = threadIdx.x & (kCols - 1), rl = threadIdx.x / kCols;
  const int c = blockIdx.y * kCols + cl;
  if (c >= C) return;
  const PoolApply k = pool_apply_consts<BN>(c, groups * ns, mean, var, gamma, beta, eps,
                                            grad_gamma, grad_beta);
  const bool need_y = BN || relu;
  const long long g0 = (long long)blockIdx.x * (kRowLanes * gpt);
  for (int t = 0; t < gpt; ++t) {
    const long long g = g0 + rl + kRowLanes * t;
    if (g >= groups) break;
    const float gr = go[g * C + c];
    const int a = arg[g * C + c];
    const float* p = y + g * ns * C + c;
    float* pd = grad_y + g * ns * C + c;
    for (int base = 0; base < ns; base += kBatch) {
      float v[kBatch];
#pragma unroll
      for (int u = 0; u < kBatch; ++u)
        v[u] = (base + u < ns && need_y) ? p[(long long)(base + u) * C] : 0.f;
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const int j = base + u;
        if (j < ns) pd[(long long)j * C] = pool_apply<BN>(k, v[u], j == a, gr, relu);
      }
    }
  }
}

template <bool BN>
__global__ __launch_bounds__(kBlock) void bn_pool_bwd_apply_split(
    const float* __restrict__ go, const int* __restrict__ arg, const float* __restrict__ y,
    long long groups, int ns, int C, int nchunk, const float* __restrict__ mean,
    const float* __restrict__ var, const float* __restrict__ gamma,
    const float* __restrict__ beta, float eps, int relu, const float* __restrict__ grad_gamma,
    const float* __restrict__ grad_beta, float* __restrict__ grad_y) {
  const int cl = threadIdx.x & (kCols - 1), rl = threadIdx.x / kCols;
  const int c = blockIdx.y * kCols + cl;
  if (c >= C) return;
  const PoolApply k = pool_apply_consts<BN>(c, groups * ns, mean, var, gamma, beta, eps,
                                            grad_gamma, grad_beta);
  const bool need_y = BN || relu;
  const long long g = blockIdx.x / nchunk;
  const int j0 = (int)(blockIdx.x % nchunk) * kActRows;
  const int nr = block_rows(ns, j0, kActRows);
  const float gr = go[g * C + c];
  const int a = arg[g * C + c] - j0;  // the winner's row within this chunk, if it is here
  const float* p = y + (g * ns + j0) * C + c;
  float* pd = grad_y + (g * ns + j0) * C + c;
  for (int base = 0; base + rl < nr; base += kStep) {
    float v[kBatch];
#pragma unroll
    for (int u = 0; u < kBatch; ++u) {
      const int r = base + rl + kRowLanes * u;
      v[u] = (r < nr && need_y) ? p[(long long)r * C] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < kBatch; ++u) {
      const int r = base + rl + kRowLanes * u;
      if (r < nr) pd[(long long)r * C] = pool_apply<BN>(k, v[u], r == a, gr, relu);
    }
  }
}

// ---------------------------------------------------------------- weight gradient -------
// blockIdx.x = part p (slabs p, p + nparts, ...), blockIdx.y = (ti, tjg): input-channel tile
// ti and output-channel tiles tjg * NJ .. + NJ - 1. Partial tiles are stored in accumulator
// order e = reg * 64 + lane: ci = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5), co = lane & 31.
template <int NJ>
__global__ __launch_bounds__(kBlock) void wgrad_partial(const float* __restrict__ x,
                                                        const float* __restrict__ gy,
                                                        long long rows, int cin, int cout,
                                                        int cout32, int nslabs, int nparts,
                                                        float* __restrict__ part) {
  constexpr int U = 8;
  __shared__ float sh[4][kTile];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int tjn = (cout32 + NJ - 1) / NJ;
  const int ti = blockIdx.y / tjn, tjg = blockIdx.y % tjn;
  const int p = blockIdx.x;
  const int kh = lane >> 5;
  const int ci = ti * 32 + (lane & 31);
  const bool ci_ok = ci < cin;
  int co[NJ];
  bool co_ok[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    co[j] = (tjg * NJ + j) * 32 + (lane & 31);
    co_ok[j] = co[j] < cout;
  }
  // output tiles of this group that exist (the last group may hold fewer than NJ): uniform
  const int nj = min(NJ, cout32 - tjg * NJ);
  double tot[NJ][4];
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int q = 0; q < 4; ++q) tot[j][q] = 0.0;

  for (int s = p; s < nslabs; s += nparts) {
    const long long r0 = (long long)s * kSlab;
    const int nr = block_rows(rows, r0, kSlab);
    f32x16 acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int k = 0; k < 16; ++k) acc[j][k] = 0.f;
    // wave w takes row pairs w, w + 4, ...: rows 2 (w + 4 t) + kh
    for (int t0 = 0; 8 * t0 < nr; t0 += U) {
      float a[U], b[NJ][U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int r = 2 * (w + 4 * (t0 + u)) + kh;
        const bool ok = r < nr;
        const long long row = r0 + r;
        a[u] = (ok && ci_ok) ? x[row * cin + ci] : 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j)
          b[j][u] = (j < nj && ok && co_ok[j]) ? gy[row * cout + co[j]] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
          if (j < nj) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], b[j][u], acc[j], 0, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      if (j >= nj) break;  // uniform over the workgroup
      __syncthreads();
#pragma unroll
      for (int k = 0; k < 16; ++k) sh[w][k * 64 + lane] = acc[j][k];
      __syncthreads();
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int e = threadIdx.x + kBlock * q;
        tot[j][q] += (double)(((sh[0][e] + sh[1][e]) + sh[2][e]) + sh[3][e]);
      }
    }
  }
  const int ntiles = gridDim.y / tjn * cout32;  // cin32 * cout32
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int tj = tjg * NJ + j;
    if (tj >= cout32) continue;
    float* dst = part + ((size_t)p * ntiles + (size_t)ti * cout32 + tj) * kTile;
#pragma unroll
    for (int q = 0; q < 4; ++q) dst[threadIdx.x + kBlock * q] = (float)tot[j][q];
  }
}

// stage 2: grad_w[ci][co] = sum over parts (double, part order)
__global__ __launch_bounds__(kBlock) void wgrad_final(const float* __restrict__ part, int cin,
                                                      int cout, int cout32, int ntiles,
                                                      int nparts, float* __restrict__ grad_w) {
  const long long idx = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (idx >= (long long)ntiles * kTile) return;
  const int tile = (int)(idx / kTile), e = (int)(idx % kTile);
  const int ti = tile / cout32, tj = tile % cout32;
  const int reg = e >> 6, lane = e & 63;
  const int ci = ti * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
  const int co = tj * 32 + (lane & 31);
  if (ci >= cin || co >= cout) return;
  double s = 0.0;
  for (int p = 0; p < nparts; ++p) s += (double)part[((size_t)p * ntiles + tile) * kTile + e];
  grad_w[(size_t)ci * cout + co] = (float)s;
}

long long ceil_div(long long a, long long b) { return (a + b - 1) / b; }

// rows of one launch: the row-block index is blockIdx.x (< 2^31), the channel tile blockIdx.y
constexpr long long kMaxRows = 0x7fffffffLL;
constexpr int kMaxC = 65535 * kCols;

int wgrad_parts(long long rows, int cin, int cout) {
  const long long ntiles = ceil_div(cin, 32) * ceil_div(cout, 32);
  long long cap = (long long)PN2_WGRAD_MAX_WS_BYTES / (ntiles * kTile * (long long)sizeof(float));
  if (cap > PN2_WGRAD_MAX_PARTS) cap = PN2_WGRAD_MAX_PARTS;
  if (cap < 1) cap = 1;
  const long long nslabs = ceil_div(rows, kSlab);
  return (int)(nslabs < cap ? nslabs : cap);
}

int wgrad_nj(int cout32) { return cout32 >= 4 ? 4 : (cout32 >= 2 ? 2 : 1); }

// groups per thread of the pooled kernels' groups layout: about kActRows rows per workgroup
int pool_gpt(int ns) {
  const int g = kActRows / kRowLanes / ns;
  return g < 1 ? 1 : g;
}

// the argument checks the pooled forward and backward share; rows = groups * ns on success
bool pool_shape_ok(long long groups, int ns, int C, long long* rows) {
  if (groups <= 0 || ns <= 0 || C <= 0 || C > kMaxC || groups > kMaxRows) return false;
  *rows = groups * ns;  // both below 2^31: no overflow
  return *rows <= kMaxRows;
}

}  // namespace
}  // namespace pn2

extern "C" {

size_t pn2_bn_workspace_size(long long rows, int C) {
  if (rows <= 0 || C <= 0) return 0;
  return (size_t)pn2::ceil_div(rows, pn2::kStatRows) * 2 * (size_t)C * sizeof(float);
}

int pn2_bn_stats(const float* y, long long rows, int C, float* mean, float* var, void* workspace,
                 size_t workspace_bytes, pn2_stream_t stream) {
  using namespace pn2;
  if (rows <= 0 || C <= 0 || rows > kMaxRows || C > kMaxC) return PN2_EINVAL;
  if (!y || !mean || !var || !workspace) return PN2_EINVAL;
  if (workspace_bytes < pn2_bn_workspace_size(rows, C)) return PN2_EINVAL;
  const int nblk = (int)ceil_div(rows, kStatRows), ct = (int)ceil_div(C, kCols);
  float* part = static_cast<float*>(workspace);
  hipLaunchKernelGGL(bn_stats_partial, dim3(nblk, ct), dim3(kBlock), 0, (hipStream_t)stream, y,
                     rows, C, part);
  hipLaunchKernelGGL(bn_stats_final, dim3(ct), dim3(kBlock), 0, (hipStream_t)stream, part, rows,
                     C, nblk, mean, var);
  PN2_RETURN_LAUNCH();
}

int pn2_bn_act_fwd(const float* y, long long rows, int C, const float* mean, const float* var,
                   const float* gamma, const float* beta, float eps, int relu, float* out,
                   pn2_stream_t stream) {
  using namespace pn2;
  if (rows <= 0 || C <= 0 || rows > kMaxRows || C > kMaxC || !y || !out) return PN2_EINVAL;
  const int given = (mean ? 1 : 0) + (var ? 1 : 0) + (gamma ? 1 : 0) + (beta ? 1 : 0);
  if (given != 0 && given != 4) return PN2_EINVAL;
  if (given && !(eps >= 0.f)) return PN2_EINVAL;
  const dim3 grid((unsigned)ceil_div(rows, kActRows), (unsigned)ceil_div(C, kCols));
  if (given)
    hipLaunchKernelGGL(bn_act_fwd_kernel<true>, grid, dim3(kBlock), 0, (hipStream_t)stream, y,
                       rows, C, mean, var, gamma, beta, eps, relu ? 1 : 0, out);
  else
    hipLaunchKernelGGL(bn_act_fwd_kernel<false>, grid, dim3(kBlock), 0, (hipStream_t)stream, y,
                       rows, C, mean, var, gamma, beta, eps, relu ? 1 : 0, out);
  PN2_RETURN_LAUNCH();
}

int pn2_bn_act_bwd(const float* grad_out, const float* y, long long rows, int C,
                   const float* mean, const float* var, const float* gamma, const float* beta,
                   float eps, int relu, float* grad_y, float* grad_gamma, float* grad_beta,
                   void* workspace, size_t workspace_bytes, pn2_stream_t stream) {
  using namespace pn2;
  if (rows <= 0 || C <= 0 || rows > kMaxRows || C > kMaxC) return PN2_EINVAL;
  if (!grad_out || !y || !grad_y || !grad_beta || !workspace) return PN2_EINVAL;
  const int given = (mean ? 1 : 0) + (var ? 1 : 0) + (gamma ? 1 : 0) + (beta ? 1 : 0);
  if (given != 0 && given != 4) return PN2_EINVAL;
  if ((given != 0) != (grad_gamma != nullptr)) return PN2_EINVAL;
  if (given && !(eps >= 0.f)) return PN2_EINVAL;
  if (workspace_bytes < pn2_bn_workspace_size(rows, C)) return PN2_EINVAL;
  const int nblk = (int)ceil_div(rows, kStatRows), ct = (int)ceil_div(C, kCols);
  float* part = static_cast<float*>(workspace);
  hipStream_t s = (hipStream_t)stream;
  if (given) {
    hipLaunchKernelGGL(bn_bwd_partial<true>, dim3(nblk, ct), dim3(kBlock), 0, s, grad_out, y, rows,
                       C, mean, var, gamma, beta, eps, relu ? 1 : 0, grad_y, part);
    hipLaunchKernelGGL(bn_bwd_final, dim3(ct), dim3(kBlock), 0, s, part, C, nblk, grad_gamma,
                       grad_beta);
    hipLaunchKernelGGL(bn_bwd_apply, dim3((unsigned)ceil_div(rows, kActRows), ct), dim3(kBlock), 0,
                       s, grad_out, y, rows, C, mean, var, gamma, beta, eps, relu ? 1 : 0,
                       grad_gamma, grad_beta, grad_y);
  } else {
    hipLaunchKernelGGL(bn_bwd_partial<false>, dim3(nblk, ct), dim3(kBlock), 0, s, grad_out, y,
                       rows, C, mean, var, gamma, beta, eps, relu ? 1 : 0, grad_y, part);
    hipLaunchKernelGGL(bn_bwd_final, dim3(ct), dim3(kBlock), 0, s, part, C, nblk, grad_gamma,
                       grad_beta);
  }
  PN2_RETURN_LAUNCH();
}

int pn2_bn_act_pool_fwd(const float* y, long long groups, int ns, int C, const float* mean,
                        const float* var, const float* gamma, const float* beta, float eps,
                        int relu, float* out, int* arg, pn2_stream_t stream) {
  using namespace pn2;
  long long rows;
  if (!pool_shape_ok(groups, ns, C, &rows) || !y || !out || !arg) return PN2_EINVAL;
  const int given = (mean ? 1 : 0) + (var ? 1 : 0) + (gamma ? 1 : 0) + (beta ? 1 : 0);
  if (given != 0 && given != 4) return PN2_EINVAL;
  if (given && !(eps >= 0.f)) return PN2_EINVAL;
  const unsigned ct = (unsigned)ceil_div(C, kCols);
  hipStream_t s = (hipStream_t)stream;
  const int r = relu ? 1 : 0;
  if (ns <= kPoolSplit) {
    const int gpt = pool_gpt(ns);
    const dim3 grid((unsigned)ceil_div(groups, (long long)kRowLanes * gpt), ct);
    if (given)
      hipLaunchKernelGGL(bn_act_pool_fwd_groups<true>, grid, dim3(kBlock), 0, s, y, groups, ns, C,
                         gpt, mean, var, gamma, beta, eps, r, out, arg);
    else
      hipLaunchKernelGGL(bn_act_pool_fwd_groups<false>, grid, dim3(kBlock), 0, s, y, groups, ns, C,
                         gpt, mean, var, gamma, beta, eps, r, out, arg);
  } else {
    const dim3 grid((unsigned)groups, ct);
    if (given)
      hipLaunchKernelGGL(bn_act_pool_fwd_split<true>, grid, dim3(kBlock), 0, s, y, ns, C, mean,
                         var, gamma, beta, eps, r, out, arg);
    else
      hipLaunchKernelGGL(bn_act_pool_fwd_split<false>, grid, dim3(kBlock), 0, s, y, ns, C, mean,
                         var, gamma, beta, eps, r, out, arg);
  }
  PN2_RETURN_LAUNCH();
}

size_t pn2_bn_pool_workspace_size(long long groups, int C) {
  if (groups <= 0 || C <= 0) return 0;
  return (size_t)pn2::ceil_div(groups, pn2::kPoolGroups) * 2 * (size_t)C * sizeof(float);
}

int pn2_bn_act_pool_bwd(const float* grad_out, const int* arg, const float* y, long long groups,
                        int ns, int C, const float* mean, const float* var, const float* gamma,
                        const float* beta, float eps, int relu, float* grad_y, float* grad_gamma,
                        float* grad_beta, void* workspace, size_t workspace_bytes,
                        pn2_stream_t stream) {
  using namespace pn2;
  long long rows;
  if (!pool_shape_ok(groups, ns, C, &rows)) return PN2_EINVAL;
  if (!grad_out || !arg || !y || !grad_y || !grad_beta || !workspace) return PN2_EINVAL;
  const int given = (mean ? 1 : 0) + (var ? 1 : 0) + (gamma ? 1 : 0) + (beta ? 1 : 0);
  if (given != 0 && given != 4) return PN2_EINVAL;
  if ((given != 0) != (grad_gamma != nullptr)) return PN2_EINVAL;
  if (given && !(eps >= 0.f)) return PN2_EINVAL;
  if (workspace_bytes < pn2_bn_pool_workspace_size(groups, C)) return PN2_EINVAL;
  const int nblk = (int)ceil_div(groups, kPoolGroups);
  const unsigned ct = (unsigned)ceil_div(C, kCols);
  float* part = static_cast<float*>(workspace);
  hipStream_t s = (hipStream_t)stream;
  const int r = relu ? 1 : 0;
  if (given)
    hipLaunchKernelGGL(bn_pool_bwd_partial<true>, dim3(nblk, ct), dim3(kBlock), 0, s, grad_out,
                       arg, y, groups, ns, C, mean, var, gamma, beta, eps, r, part);
  else
    hipLaunchKernelGGL(bn_pool_bwd_partial<false>, dim3(nblk, ct), dim3(kBlock), 0, s, grad_out,
                       arg, y, groups, ns, C, mean, var, gamma, beta, eps, r, part);
  hipLaunchKernelGGL(bn_bwd_final, dim3(ct), dim3(kBlock), 0, s, part, C, nblk, grad_gamma,
                     grad_beta);
  if (ns <= kPoolSplit) {
    const int gpt = pool_gpt(ns);
    const dim3 grid((unsigned)ceil_div(groups, (long long)kRowLanes * gpt), ct);
    if (given)
      hipLaunchKernelGGL(bn_pool_bwd_apply_groups<true>, grid, dim3(kBlock), 0, s, grad_out, arg,
                         y, groups, ns, C, gpt, mean, var, gamma, beta, eps, r, grad_gamma,
                         grad_beta, grad_y);
    else
      hipLaunchKernelGGL(bn_pool_bwd_apply_groups<false>, grid, dim3(kBlock), 0, s, grad_out, arg,
                         y, groups, ns, C, gpt, mean, var, gamma, beta, eps, r, grad_gamma,
                         grad_beta, grad_y);
  } else {
    const int nchunk = (int)ceil_div(ns, kActRows);
    const dim3 grid((unsigned)(groups * nchunk), ct);
    if (given)
      hipLaunchKernelGGL(bn_pool_bwd_apply_split<true>, grid, dim3(kBlock), 0, s, grad_out, arg, y,
                         groups, ns, C, nchunk, mean, var, gamma, beta, eps, r, grad_gamma,
                         grad_beta, grad_y);
    else
      hipLaunchKernelGGL(bn_pool_bwd_apply_split<false>, grid, dim3(kBlock), 0, s, grad_out, arg,
                         y, groups, ns, C, nchunk, mean, var, gamma, beta, eps, r, grad_gamma,
                         grad_beta, grad_y);
  }
  PN2_RETURN_LAUNCH();
}

size_t pn2_mlp_wgrad_workspace_size(long long rows, int cin, int cout) {
  if (rows <= 0 || cin <= 0 || cout <= 0) return 0;
  const size_t ntiles = (size_t)pn2::ceil_div(cin, 32) * (size_t)pn2::ceil_div(cout, 32);
  return (size_t)pn2::wgrad_parts(rows, cin, cout) * ntiles * pn2::kTile * sizeof(float);
}

int pn2_mlp_wgrad(const float* x, const float* grad_y, long long rows, int cin, int cout,
                  float* grad_w, void* workspace, size_t workspace_bytes, pn2_stream_t stream) {
  using namespace pn2;
  if (rows <= 0 || cin <= 0 || cout <= 0 || rows > kMaxRows) return PN2_EINVAL;
  if (!x || !grad_y || !grad_w || !workspace) return PN2_EINVAL;
  if (workspace_bytes < pn2_mlp_wgrad_workspace_size(rows, cin, cout)) return PN2_EINVAL;
  const int cin32 = (int)ceil_div(cin, 32), cout32 = (int)ceil_div(cout, 32);
  const int nj = wgrad_nj(cout32);
  const long long gy = (long long)cin32 * ceil_div(cout32, nj);
  const long long ntiles = (long long)cin32 * cout32;
  if (gy > 65535 || ntiles * kTile / kBlock > 0x7fffffffLL) return PN2_EINVAL;
  const int nslabs = (int)ceil_div(rows, kSlab), nparts = wgrad_parts(rows, cin, cout);
  float* part = static_cast<float*>(workspace);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(nparts, (unsigned)gy);
  if (nj == 4)
    hipLaunchKernelGGL(wgrad_partial<4>, grid, dim3(kBlock), 0, s, x, grad_y, rows, cin, cout,
                       cout32, nslabs, nparts, part);
  else if (nj == 2)
    hipLaunchKernelGGL(wgrad_partial<2>, grid, dim3(kBlock), 0, s, x, grad_y, rows, cin, cout,
                       cout32, nslabs, nparts, part);
  else
    hipLaunchKernelGGL(wgrad_partial<1>, grid, dim3(kBlock), 0, s, x, grad_y, rows, cin, cout,
                       cout32, nslabs, nparts, part);
  hipLaunchKernelGGL(wgrad_final, dim3((unsigned)(ntiles * kTile / kBlock)), dim3(kBlock), 0, s,
                     part, cin, cout, cout32, (int)ntiles, nparts, grad_w);
  PN2_RETURN_LAUNCH();
}

}  // extern "C"
