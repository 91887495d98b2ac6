// Training-mode shared-MLP layer (tf_util.conv2d / conv1d with is_training=True,
// tf_util.py:165-185; batch norm on batch statistics, :512-531), gfx950.
//
//   forward    y = x W + b            pn2_shared_mlp (mlp.hip) over a pn2_mlp_pack of W, b
//              mean, var = stats(y)   pn2_bn_stats     (biased variance)
//              out = act(bn(y))       pn2_bn_act_fwd
//   backward   grad_y, grad_gamma, grad_beta = pn2_bn_act_bwd(grad_out, y, ...)
//              grad_w = x^T grad_y    pn2_mlp_wgrad    (fp32 matrix cores)
//              grad_x = grad_y W^T    pn2_shared_mlp over a pn2_mlp_pack of W^T
//   bf16 mode (opt-in, the contract is at pn2_mlp_pack_bf16 in include/pn2hip.h): the three GEMMs
//              on the bf16 matrix cores, pn2_shared_mlp with PN2_MLP_BF16 over a
//              pn2_mlp_pack_bf16 of W, b / of W^T, and pn2_mlp_wgrad_bf16; all else as above
//   last layer of a set-abstraction MLP, fused with the max pool over the ns samples of a group
//   (y is (groups, ns, C)):
//              out, arg = max_j act(bn(y))                        pn2_bn_act_pool_fwd
//              grad_y, grad_gamma, grad_beta from (groups, C) grad_out  pn2_bn_act_pool_bwd
//
//   column sum (the attention layer's bias gradients): out = sum_r x[r]   pn2_col_sum
//
// Reductions are two-stage and ordered: stage 1 writes one partial per workgroup, stage 2
// combines the partials in a fixed order in double precision. No floating-point atomics, so
// two runs give the same bits.
//
// Per-channel kernels (stats, activation, its backward, the pooled pair, the column sum) share
// the layout, the batch-norm element expressions and the ordered sum of chan_rows.h.
//
// pn2_mlp_wgrad: v_mfma_f32_32x32x2_f32 takes A[i = lane & 31][k = lane >> 5] and
// B[k = lane >> 5][j = lane & 31]; with i = input channel, j = output channel and k = row, a
// wave that owns a 32x32 (cin, cout) tile loads x[r + (lane >> 5)][ci0 + (lane & 31)] and
// grad_y[r + (lane >> 5)][co0 + (lane & 31)]: two row segments straight from the row-major
// tensors, no transpose. The four waves of a workgroup interleave the row pairs of a slab and
// their accumulators are added through LDS in wave order. pn2_mlp_wgrad_bf16 is the same kernel
// on v_mfma_f32_32x32x16_bf16 (wgrad_partial<NJ, true>), 16 rows per MFMA.
#include "chan_rows.h"
#include "common.h"

namespace pn2 {
namespace {

using namespace chan_rows;

constexpr int kStatRows = PN2_BN_BLOCK_ROWS;  // rows per stage-1 partial (stats, sums)
constexpr int kActRows = 256;                 // rows per workgroup of the element-wise passes
constexpr int kPoolGroups = PN2_BN_POOL_BLOCK_GROUPS;  // groups per stage-1 partial (pool bwd)
constexpr int kPoolSplit = 64;                // above this ns a group is split across row lanes
constexpr int kSlab = PN2_WGRAD_SLAB_ROWS;
constexpr int kTile = 32 * 32;

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

// ---------------------------------------------------------------- batch statistics ------
// stage 1: part[(blk * 2 + 0) * C + c] = mean, [(blk * 2 + 1) * C + c] = M2 of block blk
__global__ __launch_bounds__(kBlock) void bn_stats_partial(const float* __restrict__ y,
                                                           long long rows, int C,
                                                           float* __restrict__ part) {
  __shared__ float sh[3][kRowLanes][kCols];
  const Lane t = lane_of(blockIdx.y);
  const int cl = t.cl, rl = t.rl, c = t.c;
  const long long r0 = (long long)blockIdx.x * kStatRows;
  const int nr = block_rows(rows, r0, kStatRows);
  float n = 0.f, mean = 0.f, m2 = 0.f;
  if (c < C) {
    const float* p = y + r0 * C + c;
    for (int base = 0; base + rl < nr; base += kStep) {
      float v[kBatch];
      load_rows(v, p, C, base + rl, nr);
      int cnt = 0;
      float s = 0.f;
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        cnt += step_row(base + rl, u) < nr ? 1 : 0;
        s += v[u];
      }
      const float mb = s / (float)cnt;
      float qb = 0.f;
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const float d = v[u] - mb;
        qb += (step_row(base + rl, u) < nr) ? d * d : 0.f;
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
  const Lane t = lane_of(blockIdx.x);
  const int cl = t.cl, g = t.rl, c = t.c;
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
__global__ __launch_bounds__(kBlock) void bn_act_fwd_kernel(const float* __restrict__ y,
                                                            long long rows, int C, BnArgs bn,
                                                            int relu, float* __restrict__ out) {
  const Lane t = lane_of(blockIdx.y);
  if (t.c >= C) return;
  const long long r0 = (long long)blockIdx.x * kActRows;
  const int nr = block_rows(rows, r0, kActRows);
  const BnConsts k = bn_consts<BN>(t.c, bn);
  const float* p = y + r0 * C + t.c;
  float* o = out + r0 * C + t.c;
  for (int base = 0; base + t.rl < nr; base += kStep) {
    float v[kBatch];
    load_rows(v, p, C, base + t.rl, nr);
#pragma unroll
    for (int u = 0; u < kBatch; ++u) {
      const int r = step_row(base + t.rl, u);
      if (r < nr) o[(long long)r * C] = bn_act<BN>(k, v[u], relu);
    }
  }
}

// ---------------------------------------------------------------- activation backward ---
// stage 1 of the sums: part[(blk * 2 + 0) * C + c] = sum dz, [(blk * 2 + 1) * C + c] =
// sum dz * xhat over block blk. Without batch norm grad_y = dz is written here. The second
// launch bound is the occupancy the kernel is built for: the sixteen loads of a step fit 64
// registers with batch norm (8 waves per SIMD) and 72 with the grad_y stores of the other path.
template <bool BN>
__global__ __launch_bounds__(kBlock, BN ? 8 : 7) void bn_bwd_partial(
    const float* __restrict__ go, const float* __restrict__ y, long long rows, int C, BnArgs bn,
    int relu, float* __restrict__ grad_y, float* __restrict__ part) {
  const Lane t = lane_of(blockIdx.y);
  const long long r0 = (long long)blockIdx.x * kStatRows;
  const int nr = block_rows(rows, r0, kStatRows);
  float sum[2] = {0.f, 0.f};  // dz, dz * xhat
  if (t.c < C) {
    const BnConsts k = bn_consts<BN>(t.c, bn);
    const float* py = y + r0 * C + t.c;
    const float* pg = go + r0 * C + t.c;
    float* pd = BN ? nullptr : grad_y + r0 * C + t.c;
    const bool need_y = BN || relu;  // no batch norm, no ReLU: grad_y = grad_out, y is not read
    for (int base = 0; base + t.rl < nr; base += kStep) {
      float v[kBatch], g[kBatch];
      load_rows(v, py, C, base + t.rl, nr, need_y);
      load_rows(g, pg, C, base + t.rl, nr);
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const int r = step_row(base + t.rl, u);
        const float dz = bn_dz<BN>(k, v[u], r < nr, g[u], relu);
        sum[0] += dz;
        if (BN) sum[1] += dz * bn_xhat(k, v[u]);
        else if (r < nr) pd[(long long)r * C] = dz;
      }
    }
  }
  lane_sum_store(sum, t, C, part);
}

// grad_y of the apply pass (bn_apply), batch norm only: without it bn_bwd_partial wrote grad_y
__global__ __launch_bounds__(kBlock) void bn_bwd_apply(
    const float* __restrict__ go, const float* __restrict__ y, long long rows, int C, BnArgs bn,
    int relu, const float* __restrict__ grad_gamma, const float* __restrict__ grad_beta,
    float* __restrict__ grad_y) {
  const Lane t = lane_of(blockIdx.y);
  if (t.c >= C) return;
  const long long r0 = (long long)blockIdx.x * kActRows;
  const int nr = block_rows(rows, r0, kActRows);
  const BnConsts k = bn_apply_consts<true>(t.c, bn, rows, grad_gamma, grad_beta);
  const float* py = y + r0 * C + t.c;
  const float* pg = go + r0 * C + t.c;
  float* pd = grad_y + r0 * C + t.c;
  for (int base = 0; base + t.rl < nr; base += kStep) {
    float v[kBatch], g[kBatch];
    load_rows(v, py, C, base + t.rl, nr);
    load_rows(g, pg, C, base + t.rl, nr);
#pragma unroll
    for (int u = 0; u < kBatch; ++u) {
      const int r = step_row(base + t.rl, u);
      if (r < nr) pd[(long long)r * C] = bn_apply<true>(k, v[u], true, g[u], relu);
    }
  }
}

// ---------------------------------------------------------------- column sum -------------
// out[c] = sum of x[r][c] over the rows: stage 1 per block of kStatRows rows, stage 2
// block_sum_final. It writes no rows-sized tensor (the attention layer's bias gradients).
__global__ __launch_bounds__(kBlock) void col_sum_partial(const float* __restrict__ x,
                                                          long long rows, int C,
                                                          float* __restrict__ part) {
  const Lane t = lane_of(blockIdx.y);
  const long long r0 = (long long)blockIdx.x * kStatRows;
  const int nr = block_rows(rows, r0, kStatRows);
  float sum[1] = {0.f};
  if (t.c < C) {
    const float* p = x + r0 * C + t.c;
    for (int base = 0; base + t.rl < nr; base += kStep) {
      float v[kBatch];
      load_rows(v, p, C, base + t.rl, nr);
#pragma unroll
      for (int u = 0; u < kBatch; ++u) sum[0] += v[u];
    }
  }
  lane_sum_store(sum, t, C, part);
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
template <bool BN>
__global__ __launch_bounds__(kBlock) void bn_act_pool_fwd_groups(
    const float* __restrict__ y, long long groups, int ns, int C, int gpt, BnArgs bn, int relu,
    float* __restrict__ out, int* __restrict__ arg) {
  const Lane t = lane_of(blockIdx.y);
  if (t.c >= C) return;
  const BnConsts k = bn_consts<BN>(t.c, bn);
  const long long g0 = (long long)blockIdx.x * (kRowLanes * gpt);
  for (int i = 0; i < gpt; ++i) {
    const long long g = g0 + t.rl + kRowLanes * i;
    if (g >= groups) break;
    const float* p = y + g * ns * C + t.c;
    float best = 0.f;
    int bj = 0;
    for (int base = 0; base < ns; base += kBatch) {
      float v[kBatch];
      load_rows<1>(v, p, C, base, ns);
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const int j = step_row<1>(base, u);
        const float a = bn_act<BN>(k, v[u], relu);
        if (j < ns && (j == 0 || a > best)) {
          best = a;
          bj = j;
        }
      }
    }
    out[g * C + t.c] = best;
    arg[g * C + t.c] = bj;
  }
}

template <bool BN>
__global__ __launch_bounds__(kBlock) void bn_act_pool_fwd_split(
    const float* __restrict__ y, int ns, int C, BnArgs bn, int relu, float* __restrict__ out,
    int* __restrict__ arg) {
  __shared__ float shv[kRowLanes][kCols];
  __shared__ int shj[kRowLanes][kCols];
  const Lane t = lane_of(blockIdx.y);
  const long long g = blockIdx.x;
  float best = 0.f;
  int bj = -1;  // no sample seen yet
  if (t.c < C) {
    const BnConsts k = bn_consts<BN>(t.c, bn);
    const float* p = y + g * ns * C + t.c;
    for (int base = 0; base + t.rl < ns; base += kStep) {
      float v[kBatch];
      load_rows(v, p, C, base + t.rl, ns);
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const int j = step_row(base + t.rl, u);
        const float a = bn_act<BN>(k, v[u], relu);
        if (j < ns && (bj < 0 || a > best)) {
          best = a;
          bj = j;
        }
      }
    }
  }
  shv[t.rl][t.cl] = best;
  shj[t.rl][t.cl] = bj;
  __syncthreads();
  if (t.rl == 0 && t.c < C) {  // row lane 0 holds j = 0, so bj >= 0 here
    for (int l = 1; l < kRowLanes; ++l) {
      const float v = shv[l][t.cl];
      const int j = shj[l][t.cl];
      if (j >= 0 && (v > best || (v == best && j < bj))) {
        best = v;
        bj = j;
      }
    }
    out[g * C + t.c] = best;
    arg[g * C + t.c] = bj;
  }
}

// backward, stage 1 of the sums: dz is grad_out[g][c] at j = arg[g][c] (masked by the
// recomputed pre-activation) and 0 elsewhere, so the sums read one gathered y element per
// (group, channel). part[(blk * 2 + 0) * C + c] = sum dz, [(blk * 2 + 1) * C + c] = sum dz *
// xhat over the kPoolGroups groups of block blk; stage 2 is block_sum_final. An arg outside
// [0, ns) selects nothing.
template <bool BN>
__global__ __launch_bounds__(kBlock) void bn_pool_bwd_partial(
    const float* __restrict__ go, const int* __restrict__ arg, const float* __restrict__ y,
    long long groups, int ns, int C, BnArgs bn, int relu, float* __restrict__ part) {
  const Lane t = lane_of(blockIdx.y);
  const long long g0 = (long long)blockIdx.x * kPoolGroups;
  const int ng = block_rows(groups, g0, kPoolGroups);
  float sum[2] = {0.f, 0.f};  // dz, dz * xhat
  if (t.c < C) {
    const BnConsts k = bn_consts<BN>(t.c, bn);
    const bool need_y = BN || relu;
    for (int base = 0; base + t.rl < ng; base += kStep) {
      float v[kBatch], gr[kBatch];
      int a[kBatch];
      bool ok[kBatch];
      load_rows(a, arg + g0 * C + t.c, C, base + t.rl, ng, true, -1);
      load_rows(gr, go + g0 * C + t.c, C, base + t.rl, ng);
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const int r = step_row(base + t.rl, u);
        ok[u] = a[u] >= 0 && a[u] < ns;
        v[u] = (ok[u] && need_y) ? y[((g0 + r) * ns + a[u]) * C + t.c] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const float dz = bn_dz<BN>(k, v[u], ok[u], gr[u], relu);
        sum[0] += dz;
        if (BN) sum[1] += dz * bn_xhat(k, v[u]);
      }
    }
  }
  lane_sum_store(sum, t, C, part);
}

// backward, apply pass (bn_apply with dz non-zero only at j = arg), the forward's two layouts.
// split: blockIdx.x = group * nchunk + chunk of kActRows samples (no combine here, so a group
// may span workgroups).
template <bool BN>
__global__ __launch_bounds__(kBlock) void bn_pool_bwd_apply_groups(
    const float* __restrict__ go, const int* __restrict__ arg, const float* __restrict__ y,
    long long groups, int ns, int C, int gpt, BnArgs bn, int relu,
    const float* __restrict__ grad_gamma, const float* __restrict__ grad_beta,
    float* __restrict__ grad_y) {
  const Lane t = lane_of(blockIdx.y);
  if (t.c >= C) return;
  const BnConsts k = bn_apply_consts<BN>(t.c, bn, groups * ns, grad_gamma, grad_beta);
  const bool need_y = BN || relu;
  const long long g0 = (long long)blockIdx.x * (kRowLanes * gpt);
  for (int i = 0; i < gpt; ++i) {
    const long long g = g0 + t.rl + kRowLanes * i;
    if (g >= groups) break;
    const float gr = go[g * C + t.c];
    const int a = arg[g * C + t.c];
    const float* p = y + g * ns * C + t.c;
    float* pd = grad_y + g * ns * C + t.c;
    for (int base = 0; base < ns; base += kBatch) {
      float v[kBatch];
      load_rows<1>(v, p, C, base, ns, need_y);
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const int j = step_row<1>(base, u);
        if (j < ns) pd[(long long)j * C] = bn_apply<BN>(k, v[u], j == a, gr, relu);
      }
    }
  }
}

template <bool BN>
__global__ __launch_bounds__(kBlock) void bn_pool_bwd_apply_split(
    const float* __restrict__ go, const int* __restrict__ arg, const float* __restrict__ y,
    long long groups, int ns, int C, int nchunk, BnArgs bn, int relu,
    const float* __restrict__ grad_gamma, const float* __restrict__ grad_beta,
    float* __restrict__ grad_y) {
  const Lane t = lane_of(blockIdx.y);
  if (t.c >= C) return;
  const BnConsts k = bn_apply_consts<BN>(t.c, bn, groups * ns, grad_gamma, grad_beta);
  const bool need_y = BN || relu;
  const long long g = blockIdx.x / nchunk;
  const int j0 = (int)(blockIdx.x % nchunk) * kActRows;
  const int nr = block_rows(ns, j0, kActRows);
  const float gr = go[g * C + t.c];
  const int a = arg[g * C + t.c] - j0;  // the winner's row within this chunk, if it is here
  const float* p = y + (g * ns + j0) * C + t.c;
  float* pd = grad_y + (g * ns + j0) * C + t.c;
  for (int base = 0; base + t.rl < nr; base += kStep) {
    float v[kBatch];
    load_rows(v, p, C, base + t.rl, nr, need_y);
#pragma unroll
    for (int u = 0; u < kBatch; ++u) {
      const int r = step_row(base + t.rl, u);
      if (r < nr) pd[(long long)r * C] = bn_apply<BN>(k, v[u], r == a, gr, relu);
    }
  }
}

// ---------------------------------------------------------------- weight gradient -------
// blockIdx.x = part p (slabs p, p + nparts, ...), blockIdx.y = (ti, tjg): input-channel tile
// ti and output-channel tiles tjg * NJ .. + NJ - 1. Partial tiles are stored in accumulator
// order e = reg * 64 + lane: ci = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5), co = lane & 31.
//
// BF: the same stage 1 on v_mfma_f32_32x32x16_bf16 (pn2_mlp_wgrad_bf16): lane (h = lane >> 5,
// i = lane & 31) holds A[i][8h + j] and B[8h + j][i], j = 0..7, so one MFMA covers 16 rows and a
// lane loads x[r + 8h + j][ci0 + i] and grad_y[r + 8h + j][co0 + i] for eight j: per j two
// 128-byte row segments per wave, straight from the row-major tensors, rounded to bf16 pairs on
// the way in. The four waves interleave the 16-row blocks of a slab (16 MFMAs per wave and tile
// from zero). Only the operand loads and the MFMA differ: the accumulator layout, the LDS sum,
// the double slab sum and the partial tiles are one text, so wgrad_final serves both.
template <int NJ, bool BF>
__global__ __launch_bounds__(kBlock) void wgrad_partial(const float* __restrict__ x,
                                                        const float* __restrict__ gy,
                                                        long long rows, int cin, int cout,
                                                        int cout32, int nslabs, int nparts,
                                                        float* __restrict__ part) {
  // in flight per wave: row pairs (fp32), 16-row blocks (bf16)
  constexpr int U = BF ? (NJ == 4 ? 2 : 4) : 8;
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
    if constexpr (BF) {
      // wave w takes 16-row blocks w, w + 4, ...: rows 16 (w + 4 t) + 8 kh + j
      for (int t0 = 0; 64 * t0 < nr; t0 += U) {
        float a[U][8], b[NJ][U][8];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const int r = 16 * (w + 4 * (t0 + u)) + 8 * kh + k;
            const bool ok = r < nr;
            const long long row = r0 + r;
            a[u][k] = (ok && ci_ok) ? x[row * cin + ci] : 0.f;
#pragma unroll
            for (int j = 0; j < NJ; ++j)
              b[j][u][k] = (j < nj && ok && co_ok[j]) ? gy[row * cout + co[j]] : 0.f;
          }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const bf16x8 av = pack_bf16x8(a[u]);
#pragma unroll
          for (int j = 0; j < NJ; ++j)
            if (j < nj)
              acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, pack_bf16x8(b[j][u]), acc[j],
                                                               0, 0, 0);
        }
      }
    } else {
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
            if (j < nj)
              acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], b[j][u], acc[j], 0, 0, 0);
      }
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

// The batch-norm pointer group: all four or none, eps >= 0 with them, and in a backward pass
// (grad_gamma given) *grad_gamma present exactly when the group is.
bool bn_args_ok(const BnArgs& bn, float* const* grad_gamma = nullptr) {
  const int given = (bn.mean ? 1 : 0) + (bn.var ? 1 : 0) + (bn.gamma ? 1 : 0) + (bn.beta ? 1 : 0);
  if (given != 0 && given != 4) return false;
  if (grad_gamma && (given != 0) != (*grad_gamma != nullptr)) return false;
  return !given || bn.eps >= 0.f;
}

// kernel<true> with the group, kernel<false> without it, on a kBlock-thread grid
#define PN2_LAUNCH_BN(bn, kernel, grid, stream, ...)                                        \
  do {                                                                                      \
    if ((bn).mean)                                                                          \
      hipLaunchKernelGGL(kernel<true>, grid, dim3(kBlock), 0, stream, __VA_ARGS__);         \
    else                                                                                    \
      hipLaunchKernelGGL(kernel<false>, grid, dim3(kBlock), 0, stream, __VA_ARGS__);        \
  } while (0)

int wgrad_parts(long long rows, int cin, int cout) {
  const long long ntiles = ceil_div(cin, 32) * ceil_div(cout, 32);
  long long cap = (long long)PN2_WGRAD_MAX_WS_BYTES / (ntiles * kTile * (long long)sizeof(float));
  if (cap > PN2_WGRAD_MAX_PARTS) cap = PN2_WGRAD_MAX_PARTS;
  if (cap < 1) cap = 1;
  const long long nslabs = ceil_div(rows, kSlab);
  return (int)(nslabs < cap ? nslabs : cap);
}

int wgrad_nj(int cout32) { return cout32 >= 4 ? 4 : (cout32 >= 2 ? 2 : 1); }

size_t wgrad_ws_bytes(long long rows, int cin, int cout) {
  const size_t ntiles = (size_t)ceil_div(cin, 32) * (size_t)ceil_div(cout, 32);
  return (size_t)wgrad_parts(rows, cin, cout) * ntiles * kTile * sizeof(float);
}

// pn2_mlp_wgrad and, with bf16, pn2_mlp_wgrad_bf16: the same checks, grid and stage 2
int wgrad_launch(bool bf16, const float* x, const float* grad_y, long long rows, int cin, int cout,
                 float* grad_w, void* workspace, size_t workspace_bytes, pn2_stream_t stream) {
  if (rows <= 0 || cin <= 0 || cout <= 0 || rows > kMaxRows) return PN2_EINVAL;
  if (!x || !grad_y || !grad_w || !workspace) return PN2_EINVAL;
  if (workspace_bytes < wgrad_ws_bytes(rows, cin, cout)) return PN2_EINVAL;
  const int cin32 = (int)ceil_div(cin, 32), cout32 = (int)ceil_div(cout, 32);
  const int nj = wgrad_nj(cout32);
  const long long gy = (long long)cin32 * ceil_div(cout32, nj);
  const long long ntiles = (long long)cin32 * cout32;
  if (gy > 65535 || ntiles * kTile / kBlock > 0x7fffffffLL) return PN2_EINVAL;
  const int nslabs = (int)ceil_div(rows, kSlab), nparts = wgrad_parts(rows, cin, cout);
  float* part = static_cast<float*>(workspace);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(nparts, (unsigned)gy);
  auto* stage1 = nj == 4 ? (bf16 ? wgrad_partial<4, true> : wgrad_partial<4, false>)
                 : nj == 2 ? (bf16 ? wgrad_partial<2, true> : wgrad_partial<2, false>)
                           : (bf16 ? wgrad_partial<1, true> : wgrad_partial<1, false>);
  hipLaunchKernelGGL(stage1, grid, dim3(kBlock), 0, s, x, grad_y, rows, cin, cout, cout32, nslabs,
                     nparts, part);
  hipLaunchKernelGGL(wgrad_final, dim3((unsigned)(ntiles * kTile / kBlock)), dim3(kBlock), 0, s,
                     part, cin, cout, cout32, (int)ntiles, nparts, grad_w);
  PN2_RETURN_LAUNCH();
}

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
  const BnArgs bn = {mean, var, gamma, beta, eps};
  if (!bn_args_ok(bn)) return PN2_EINVAL;
  const dim3 grid((unsigned)ceil_div(rows, kActRows), (unsigned)ceil_div(C, kCols));
  PN2_LAUNCH_BN(bn, bn_act_fwd_kernel, grid, (hipStream_t)stream, y, rows, C, bn, relu ? 1 : 0,
                out);
  PN2_RETURN_LAUNCH();
}

int pn2_bn_act_bwd(const float* grad_out, const float* y, long long rows, int C,
                   const float* mean, const float* var, const float* gamma, const float* beta,
                   float eps, int relu, float* grad_y, float* grad_gamma, float* grad_beta,
                   void* workspace, size_t workspace_bytes, pn2_stream_t stream) {
  using namespace pn2;
  if (rows <= 0 || C <= 0 || rows > kMaxRows || C > kMaxC) return PN2_EINVAL;
  if (!grad_out || !y || !grad_y || !grad_beta || !workspace) return PN2_EINVAL;
  const BnArgs bn = {mean, var, gamma, beta, eps};
  if (!bn_args_ok(bn, &grad_gamma)) return PN2_EINVAL;
  if (workspace_bytes < pn2_bn_workspace_size(rows, C)) return PN2_EINVAL;
  const int nblk = (int)ceil_div(rows, kStatRows), ct = (int)ceil_div(C, kCols);
  float* part = static_cast<float*>(workspace);
  hipStream_t s = (hipStream_t)stream;
  PN2_LAUNCH_BN(bn, bn_bwd_partial, dim3(nblk, ct), s, grad_out, y, rows, C, bn, relu ? 1 : 0,
                grad_y, part);
  hipLaunchKernelGGL(block_sum_final<2>, dim3(ct), dim3(kBlock), 0, s, part, C, nblk, grad_beta,
                     grad_gamma);
  if (bn.mean)
    hipLaunchKernelGGL(bn_bwd_apply, dim3((unsigned)ceil_div(rows, kActRows), ct), dim3(kBlock), 0,
                       s, grad_out, y, rows, C, bn, relu ? 1 : 0, grad_gamma, grad_beta, grad_y);
  PN2_RETURN_LAUNCH();
}

int pn2_bn_act_pool_fwd(const float* y, long long groups, int ns, int C, const float* mean,
                        const float* var, const float* gamma, const float* beta, float eps,
                        int relu, float* out, int* arg, pn2_stream_t stream) {
  using namespace pn2;
  long long rows;
  if (!pool_shape_ok(groups, ns, C, &rows) || !y || !out || !arg) return PN2_EINVAL;
  const BnArgs bn = {mean, var, gamma, beta, eps};
  if (!bn_args_ok(bn)) return PN2_EINVAL;
  const unsigned ct = (unsigned)ceil_div(C, kCols);
  hipStream_t s = (hipStream_t)stream;
  const int r = relu ? 1 : 0;
  if (ns <= kPoolSplit) {
    const int gpt = pool_gpt(ns);
    const dim3 grid((unsigned)ceil_div(groups, (long long)kRowLanes * gpt), ct);
    PN2_LAUNCH_BN(bn, bn_act_pool_fwd_groups, grid, s, y, groups, ns, C, gpt, bn, r, out, arg);
  } else {
    PN2_LAUNCH_BN(bn, bn_act_pool_fwd_split, dim3((unsigned)groups, ct), s, y, ns, C, bn, r, out,
                  arg);
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
  const BnArgs bn = {mean, var, gamma, beta, eps};
  if (!bn_args_ok(bn, &grad_gamma)) return PN2_EINVAL;
  if (workspace_bytes < pn2_bn_pool_workspace_size(groups, C)) return PN2_EINVAL;
  const int nblk = (int)ceil_div(groups, kPoolGroups);
  const unsigned ct = (unsigned)ceil_div(C, kCols);
  float* part = static_cast<float*>(workspace);
  hipStream_t s = (hipStream_t)stream;
  const int r = relu ? 1 : 0;
  PN2_LAUNCH_BN(bn, bn_pool_bwd_partial, dim3(nblk, ct), s, grad_out, arg, y, groups, ns, C, bn, r,
                part);
  hipLaunchKernelGGL(block_sum_final<2>, dim3(ct), dim3(kBlock), 0, s, part, C, nblk, grad_beta,
                     grad_gamma);
  if (ns <= kPoolSplit) {
    const int gpt = pool_gpt(ns);
    const dim3 grid((unsigned)ceil_div(groups, (long long)kRowLanes * gpt), ct);
    PN2_LAUNCH_BN(bn, bn_pool_bwd_apply_groups, grid, s, grad_out, arg, y, groups, ns, C, gpt, bn,
                  r, grad_gamma, grad_beta, grad_y);
  } else {
    const int nchunk = (int)ceil_div(ns, kActRows);
    PN2_LAUNCH_BN(bn, bn_pool_bwd_apply_split, dim3((unsigned)(groups * nchunk), ct), s, grad_out,
                  arg, y, groups, ns, C, nchunk, bn, r, grad_gamma, grad_beta, grad_y);
  }
  PN2_RETURN_LAUNCH();
}

size_t pn2_col_sum_workspace_size(long long rows, int C) {
  if (rows <= 0 || C <= 0) return 0;
  return (size_t)pn2::ceil_div(rows, pn2::kStatRows) * (size_t)C * sizeof(float);
}

int pn2_col_sum(const float* x, long long rows, int C, float* out, void* workspace,
                size_t workspace_bytes, pn2_stream_t stream) {
  using namespace pn2;
  if (rows <= 0 || C <= 0 || rows > kMaxRows || C > kMaxC) return PN2_EINVAL;
  if (!x || !out || !workspace) return PN2_EINVAL;
  if (workspace_bytes < pn2_col_sum_workspace_size(rows, C)) return PN2_EINVAL;
  const int nblk = (int)ceil_div(rows, kStatRows), ct = (int)ceil_div(C, kCols);
  float* part = static_cast<float*>(workspace);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(col_sum_partial, dim3(nblk, ct), dim3(kBlock), 0, s, x, rows, C, part);
  hipLaunchKernelGGL(block_sum_final<1>, dim3(ct), dim3(kBlock), 0, s, part, C, nblk, out,
                     (float*)nullptr);
  PN2_RETURN_LAUNCH();
}

size_t pn2_mlp_wgrad_workspace_size(long long rows, int cin, int cout) {
  if (rows <= 0 || cin <= 0 || cout <= 0) return 0;
  return pn2::wgrad_ws_bytes(rows, cin, cout);
}

int pn2_mlp_wgrad(const float* x, const float* grad_y, long long rows, int cin, int cout,
                  float* grad_w, void* workspace, size_t workspace_bytes, pn2_stream_t stream) {
  return pn2::wgrad_launch(false, x, grad_y, rows, cin, cout, grad_w, workspace, workspace_bytes,
                           stream);
}

int pn2_mlp_wgrad_bf16(const float* x, const float* grad_y, long long rows, int cin, int cout,
                       float* grad_w, void* workspace, size_t workspace_bytes,
                       pn2_stream_t stream) {
  return pn2::wgrad_launch(true, x, grad_y, rows, cin, cout, grad_w, workspace, workspace_bytes,
                           stream);
}

}  // extern "C"
