// The per-channel layout of the training kernels and the ordered sum on top of it, gfx950.
//
// Layout: a workgroup of 256 threads owns 32 channels and a block of rows; thread
// (cl = tid & 31, rl = tid >> 5) walks rows rl, rl + 8, ... of channel cl, eight rows per step
// (eight independent guarded loads), so a wave's load covers two 128-byte row segments and the
// channel's constants stay in registers. The row-block index is blockIdx.x, the channel tile
// blockIdx.y.
//
// Ordered sum, two stages, no floating-point atomics: stage 1 (lane_sum_store) adds the eight
// row lanes' partials through LDS in lane order and writes one partial per workgroup; stage 2
// (block_sum_final) gives row lane g the blocks g, g + 8, ... in double, then adds the lanes in
// order. Grid and order depend on the shape alone, so two runs give the same bits.
//
// Beside them: the per-channel batch-norm constants and the element expressions the forward,
// the backward mask and the apply pass must round identically.
#pragma once
#include "common.h"

namespace pn2 {
namespace chan_rows {

constexpr int kBlock = 256;
constexpr int kCols = 32;                    // channels per workgroup
constexpr int kRowLanes = kBlock / kCols;    // 8
constexpr int kBatch = 8;                    // rows per thread per step
constexpr int kStep = kRowLanes * kBatch;    // 64 rows per workgroup step
// rows of one launch: the row-block index is blockIdx.x (< 2^31), the channel tile blockIdx.y
constexpr long long kMaxRows = 0x7fffffffLL;
constexpr int kMaxC = 65535 * kCols;

struct Lane {
  int cl, rl, c;  // channel within the tile, row lane, channel
};
PN2_DEV Lane lane_of(int tile) {
  const int cl = threadIdx.x & (kCols - 1);
  return {cl, (int)threadIdx.x / kCols, tile * kCols + cl};
}

PN2_DEV int block_rows(long long rows, long long r0, int per) {
  const long long left = rows - r0;
  return left < per ? (int)left : per;
}

// row u of the step that starts at row `first` (= base + rl; the per-group kernels walk one
// group's samples with STRIDE 1)
template <int STRIDE = kRowLanes>
PN2_DEV int step_row(int first, int u) { return first + STRIDE * u; }

// v[u] = p[row u * C] for the step's rows below nr (and only if `on`), `fill` elsewhere
template <int STRIDE = kRowLanes, typename T>
PN2_DEV void load_rows(T (&v)[kBatch], const T* p, int C, int first, int nr, bool on = true,
                       T fill = T(0)) {
#pragma unroll
  for (int u = 0; u < kBatch; ++u) {
    const int r = step_row<STRIDE>(first, u);
    v[u] = (r < nr && on) ? p[(long long)r * C] : fill;
  }
}

// ---------------------------------------------------------------- batch norm ------------
// the optional batch-norm pointer group of every entry point: all four or none
struct BnArgs {
  const float *mean, *var, *gamma, *beta;
  float eps;
};

// gamma / sqrt(var + eps) and the pre-activation, written once: the forward pass and the
// backward mask must round identically.
PN2_DEV float bn_scale(float gamma, float var, float eps) {
  return __fdiv_rn(gamma, __fsqrt_rn(__fadd_rn(var, eps)));
}
PN2_DEV float bn_pre(float y, float mean, float s, float beta) {
  return __fadd_rn(__fmul_rn(__fsub_rn(y, mean), s), beta);
}

// a channel's constants; mb, mg = grad_beta / rows, grad_gamma / rows of the apply pass
struct BnConsts {
  float m, s, b, rstd, mb, mg;
};
template <bool BN>
PN2_DEV BnConsts bn_consts(int c, const BnArgs& bn) {
  BnConsts k = {0.f, 1.f, 0.f, 1.f, 0.f, 0.f};
  if (BN) {
    k.m = bn.mean[c];
    k.b = bn.beta[c];
    k.s = bn_scale(bn.gamma[c], bn.var[c], bn.eps);
    k.rstd = __fdiv_rn(1.f, __fsqrt_rn(__fadd_rn(bn.var[c], bn.eps)));
  }
  return k;
}
template <bool BN>
PN2_DEV BnConsts bn_apply_consts(int c, const BnArgs& bn, long long rows, const float* grad_gamma,
                                 const float* grad_beta) {
  BnConsts k = bn_consts<BN>(c, bn);
  if (BN) {
    const float inv_rows = (float)(1.0 / (double)rows);
    k.mb = grad_beta[c] * inv_rows;
    k.mg = grad_gamma[c] * inv_rows;
  }
  return k;
}

// act(bn(v))
template <bool BN>
PN2_DEV float bn_act(const BnConsts& k, float v, int relu) {
  const float pre = BN ? bn_pre(v, k.m, k.s, k.b) : v;
  return relu ? fmaxf(pre, 0.f) : pre;
}
// the gradient at the pre-activation: g where the element is `hit` and the ReLU passes it
template <bool BN>
PN2_DEV float bn_dz(const BnConsts& k, float v, bool hit, float g, int relu) {
  const float pre = BN ? bn_pre(v, k.m, k.s, k.b) : v;
  return (hit && (!relu || pre > 0.f)) ? g : 0.f;
}
PN2_DEV float bn_xhat(const BnConsts& k, float v) { return (v - k.m) * k.rstd; }
// the apply pass's element: grad_y = gamma / sigma * (dz - grad_beta / R - xhat * grad_gamma / R);
// without batch norm grad_y = dz
template <bool BN>
PN2_DEV float bn_apply(const BnConsts& k, float v, bool hit, float g, int relu) {
  const float dz = bn_dz<BN>(k, v, hit, g, relu);
  if (!BN) return dz;
  return k.s * ((dz - k.mb) - bn_xhat(k, v) * k.mg);
}

// ---------------------------------------------------------------- ordered sum -----------
// stage 1's end: part[(blockIdx.x * K + k) * C + c] = acc[k] of row lanes 0, 1, ..., 7 in order.
// Every thread of the workgroup calls it.
template <int K>
PN2_DEV void lane_sum_store(float (&acc)[K], const Lane& t, int C, float* __restrict__ part) {
  __shared__ float sh[K][kRowLanes][kCols];
#pragma unroll
  for (int k = 0; k < K; ++k) sh[k][t.rl][t.cl] = acc[k];
  __syncthreads();
  if (t.rl == 0 && t.c < C) {
    for (int j = 1; j < kRowLanes; ++j)
#pragma unroll
      for (int k = 0; k < K; ++k) acc[k] += sh[k][j][t.cl];
#pragma unroll
    for (int k = 0; k < K; ++k) part[((size_t)blockIdx.x * K + k) * C + t.c] = acc[k];
  }
}

// stage 2: one workgroup per 32 channels; out0[c], out1[c] = sums 0 and 1 of the nblk blocks
// (out1 only for K = 2, and it may be null). Internal to each file that launches it: the
// library exports the C ABI only.
namespace {
template <int K>
__global__ __launch_bounds__(kBlock) void block_sum_final(const float* __restrict__ part, int C,
                                                          int nblk, float* __restrict__ out0,
                                                          float* __restrict__ out1) {
  static_assert(K == 1 || K == 2, "one or two sums per channel");
  __shared__ double sh[K][kRowLanes][kCols];
  const Lane t = lane_of(blockIdx.x);
  const int g = t.rl;
  double s[K];
#pragma unroll
  for (int k = 0; k < K; ++k) s[k] = 0.0;
  if (t.c < C) {
    for (int b = g; b < nblk; b += kRowLanes)
#pragma unroll
      for (int k = 0; k < K; ++k) s[k] += (double)part[((size_t)b * K + k) * C + t.c];
  }
#pragma unroll
  for (int k = 0; k < K; ++k) sh[k][g][t.cl] = s[k];
  __syncthreads();
  if (g == 0 && t.c < C) {
    for (int j = 1; j < kRowLanes; ++j)
#pragma unroll
      for (int k = 0; k < K; ++k) s[k] += sh[k][j][t.cl];
    out0[t.c] = (float)s[0];
    if (K == 2 && out1) out1[t.c] = (float)s[K - 1];
  }
}
}  // namespace

}  // namespace chan_rows
}  // namespace pn2
