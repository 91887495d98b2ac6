// Training-mode segmentation head (pointnet2_sem_seg.py:56, :62-69), gfx950: the dropout
// between fc1 and fc2 (tf_util.dropout, tf_util.py:594-612) and get_loss's
// tf.losses.sparse_softmax_cross_entropy(labels, logits, weights) with its default reduction
// SUM_BY_NONZERO_WEIGHTS.
//
//   pn2_dropout           out[e] = keep(e) ? x[e] / keep_prob : 0, keep(e) a pure function of
//                         (seed, e) (philox.h): no mask tensor, the backward is the same call on
//                         the gradient. One thread per Philox call = four elements, one 16-byte
//                         load and store; the tail n % 4 and unaligned pointers go scalar.
//   pn2_softmax_xent_fwd  one read of the logits: per row lse = m + log sum exp(z - m), the
//                         argmax, w * (lse - z[label]); then the two-stage ordered sum of
//                         mlp_train.hip: one fp32 partial and one count per PN2_XENT_BLOCK_ROWS
//                         rows, added in double by one workgroup in a fixed order. No atomics.
//   pn2_softmax_xent_bwd  one read of the logits, one write:
//                         g * w / num_present * (exp(z - lse) - [c == label]).
//
// Forward layouts. A row is 4 C bytes (84 at C = 21), so a lane per row reading global memory
// would stride. C <= 64: the workgroup's block_rows x C span is contiguous; it is loaded with
// coalesced 16-byte loads into LDS, then thread t owns row t. The LDS row stride in words is
// odd (C, or C + 1 for even C), so the 64 lanes of a wave fall on 64 different banks at every
// column. C > 64: one wave per row, lanes stride the columns with an online (max, sum) pair and
// the wave reductions of common.h combine them; still one read.
#include <math.h>

#include "common.h"
#include "philox.h"

namespace pn2 {
namespace {

constexpr int kDropBlock = 256;
constexpr unsigned kDropMaxGrid = 1u << 20;

constexpr int kXentRows = PN2_XENT_BLOCK_ROWS;  // rows per workgroup and per stage-1 partial
constexpr int kXentLdsThreads = kXentRows;      // LDS layout: one thread per row
constexpr int kXentLdsMaxC = 64;
constexpr int kXentWaveThreads = 256;           // wave layout: 4 waves, 32 rows each
constexpr int kXentWaves = kXentWaveThreads / kWave;
constexpr int kXentRowsPerWave = kXentRows / kXentWaves;
constexpr int kXentFinalThreads = 256;
constexpr int kXentBwdThreads = 256;
constexpr long long kXentMaxRows = 0x7fffffffLL;
constexpr int kXentMaxC = 65535;

// ---------------------------------------------------------------- dropout ---------------
template <bool VEC>
__global__ __launch_bounds__(kDropBlock) void dropout_kernel(const float* x, uint64_t n,
                                                             float keep_prob, uint64_t thr,
                                                             uint64_t seed, float* out) {
  const uint64_t nq = (n + 3) / 4, full = n / 4;
  const uint64_t step = (uint64_t)gridDim.x * kDropBlock;
  for (uint64_t q = (uint64_t)blockIdx.x * kDropBlock + threadIdx.x; q < nq; q += step) {
    const Philox4 r = dropout_words(seed, q);
    if (VEC && q < full) {
      const float4 v = reinterpret_cast<const float4*>(x)[q];
      float4 o;
      o.x = (uint64_t)r.w[0] < thr ? __fdiv_rn(v.x, keep_prob) : 0.f;
      o.y = (uint64_t)r.w[1] < thr ? __fdiv_rn(v.y, keep_prob) : 0.f;
      o.z = (uint64_t)r.w[2] < thr ? __fdiv_rn(v.z, keep_prob) : 0.f;
      o.w = (uint64_t)r.w[3] < thr ? __fdiv_rn(v.w, keep_prob) : 0.f;
      reinterpret_cast<float4*>(out)[q] = o;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint64_t e = 4 * q + j;
        if (e < n) out[e] = (uint64_t)r.w[j] < thr ? __fdiv_rn(x[e], keep_prob) : 0.f;
      }
    }
  }
}

// ---------------------------------------------------------------- loss, forward ---------
PN2_DEV int xent_block_rows(long long rows, long long r0) {
  const long long left = rows - r0;
  return left < kXentRows ? (int)left : kXentRows;
}

// w * ce of one row and whether it counts; a label outside [0, C) is never dereferenced
PN2_DEV float xent_row_loss(float lse, float z_label, bool label_ok, float w) {
  const float ce = label_ok ? lse - z_label : __builtin_nanf("");
  return w * ce;
}

// C <= 64. VEC: the span's base is 16-byte aligned.
template <bool VEC>
__global__ __launch_bounds__(kXentLdsThreads) void xent_fwd_lds(
    const float* __restrict__ z, const int32_t* __restrict__ labels,
    const float* __restrict__ weights, long long rows, int C, FastDiv divC,
    float* __restrict__ lse, int32_t* __restrict__ pred, float* __restrict__ part,
    int32_t* __restrict__ cnt) {
  extern __shared__ float sh[];  // kXentRows * stride words (at most 33,280 bytes)
  __shared__ float shs[kXentLdsThreads / kWave];
  __shared__ int shn[kXentLdsThreads / kWave];
  const int tid = threadIdx.x;
  const long long r0 = (long long)blockIdx.x * kXentRows;
  const int nr = xent_block_rows(rows, r0);
  const int len = nr * C;  // <= 128 * 64
  const int stride = C | 1;  // odd: C, or C + 1 for even C
  const int pad = stride - C;
  const float* p = z + r0 * C;
  const int len4 = VEC ? len >> 2 : 0;
  if (VEC) {
    const float4* p4 = reinterpret_cast<const float4*>(p);
    for (int i = tid; i < len4; i += kXentLdsThreads) {
      const float4 v = p4[i];
      const float e[4] = {v.x, v.y, v.z, v.w};
      const int k = 4 * i;
      int r = (int)fdiv((uint32_t)k, divC);
      int c = k - r * C;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        sh[k + j + pad * r] = e[j];  // r * stride + c
        if (++c == C) {
          c = 0;
          ++r;
        }
      }
    }
  }
  for (int k = 4 * len4 + tid; k < len; k += kXentLdsThreads) {
    const int r = (int)fdiv((uint32_t)k, divC);
    sh[k + pad * r] = p[k];
  }
  __syncthreads();

  float contrib = 0.f;
  int present = 0;
  if (tid < nr) {
    const float* row = sh + tid * stride;
    float m = row[0];
    int am = 0;
    for (int c = 1; c < C; ++c) {
      const float v = row[c];
      if (v > m) {  // strict: ties keep the lowest index
        m = v;
        am = c;
      }
    }
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += expf(row[c] - m);
    const float l = m + logf(s);
    const long long gr = r0 + tid;
    lse[gr] = l;
    if (pred) pred[gr] = am;
    const int lab = labels[gr];
    const bool ok = lab >= 0 && lab < C;
    const float w = weights ? weights[gr] : 1.f;
    contrib = xent_row_loss(l, ok ? row[lab] : 0.f, ok, w);
    present = w != 0.f ? 1 : 0;
  }
  // rows of a wave in xor-shuffle order, then the waves in order
  const float ws = seg_sum<kWave>(contrib);
  const int wn = __popcll(__ballot(present));
  if ((tid & (kWave - 1)) == 0) {
    shs[tid / kWave] = ws;
    shn[tid / kWave] = wn;
  }
  __syncthreads();
  if (tid == 0) {
    float s = shs[0];
    int n = shn[0];
    for (int k = 1; k < kXentLdsThreads / kWave; ++k) {
      s += shs[k];
      n += shn[k];
    }
    part[blockIdx.x] = s;
    cnt[blockIdx.x] = n;
  }
}

// order-preserving map of a float onto uint32 (-0 counts as +0, as it compares)
PN2_DEV uint32_t float_key(float v) {
  const uint32_t b = __float_as_uint(v + 0.f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
PN2_DEV float key_float(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// C > 64: wave w of the workgroup walks rows 32 w .. 32 w + 31 of the block, in order
__global__ __launch_bounds__(kXentWaveThreads) void xent_fwd_wave(
    const float* __restrict__ z, const int32_t* __restrict__ labels,
    const float* __restrict__ weights, long long rows, int C, float* __restrict__ lse,
    int32_t* __restrict__ pred, float* __restrict__ part, int32_t* __restrict__ cnt) {
  __shared__ float shs[kXentWaves];
  __shared__ int shn[kXentWaves];
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
  const long long r0 = (long long)blockIdx.x * kXentRows;
  const int nr = xent_block_rows(rows, r0);
  float acc = 0.f;
  int np = 0;
  for (int i = 0; i < kXentRowsPerWave; ++i) {
    const int r = w * kXentRowsPerWave + i;
    if (r >= nr) break;  // uniform over the wave
    const long long gr = r0 + r;
    const float* row = z + gr * C;
    // online (max, sum of exp) per lane; every lane sees at least one column (C > 64)
    float m = -INFINITY, s = 0.f;
    int am = 0;
    for (int c = lane; c < C; c += kWave) {
      const float v = row[c];
      if (v > m) {  // strict and ascending c: the lane's lowest index among ties
        s = s * expf(m - v) + 1.f;
        m = v;
        am = c;
      } else {
        s += expf(v - m);
      }
    }
    // the largest value, then the lowest index
    const uint64_t best = wave_max_u64(pack64(0xffffffffu - (uint32_t)am, float_key(m)));
    const float M = key_float((uint32_t)(best >> 32));
    const int AM = (int)(0xffffffffu - (uint32_t)best);
    const float S = seg_sum<kWave>(s * expf(m - M));
    const float l = M + logf(S);
    const int lab = labels[gr];
    const bool ok = lab >= 0 && lab < C;
    const float wt = weights ? weights[gr] : 1.f;
    if (lane == 0) {
      lse[gr] = l;
      if (pred) pred[gr] = AM;
    }
    acc += xent_row_loss(l, ok ? row[lab] : 0.f, ok, wt);
    np += wt != 0.f ? 1 : 0;
  }
  if (lane == 0) {
    shs[w] = acc;
    shn[w] = np;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = shs[0];
    int n = shn[0];
    for (int k = 1; k < kXentWaves; ++k) {
      s += shs[k];
      n += shn[k];
    }
    part[blockIdx.x] = s;
    cnt[blockIdx.x] = n;
  }
}

// stage 2: thread t adds blocks t, t + 256, ... in double, then a fixed tree over the threads
__global__ __launch_bounds__(kXentFinalThreads) void xent_final(const float* __restrict__ part,
                                                                const int32_t* __restrict__ cnt,
                                                                int nblk, float* __restrict__ loss,
                                                                int32_t* __restrict__ num_present) {
  __shared__ double shs[kXentFinalThreads];
  __shared__ long long shn[kXentFinalThreads];
  const int tid = threadIdx.x;
  double s = 0.0;
  long long n = 0;
  for (int b = tid; b < nblk; b += kXentFinalThreads) {
    s += (double)part[b];
    n += cnt[b];
  }
  shs[tid] = s;
  shn[tid] = n;
  for (int o = kXentFinalThreads / 2; o > 0; o >>= 1) {
    __syncthreads();
    if (tid < o) {
      shs[tid] += shs[tid + o];
      shn[tid] += shn[tid + o];
    }
  }
  if (tid == 0) {
    *num_present = (int32_t)shn[0];
    *loss = shn[0] ? (float)(shs[0] / (double)shn[0]) : 0.f;  // TF's safe division
  }
}

// ---------------------------------------------------------------- loss, backward --------
// A workgroup owns the contiguous span of kXentRows rows; thread t takes W consecutive elements
// (W = 4: one 16-byte load and store) and strides the span, carrying (row, column) along
// without a division per step. The row's constants are reloaded when the row changes.
template <int W>
__global__ __launch_bounds__(kXentBwdThreads) void xent_bwd_kernel(
    const float* __restrict__ grad_loss, const float* __restrict__ z,
    const int32_t* __restrict__ labels, const float* __restrict__ weights,
    const float* __restrict__ lse, const int32_t* __restrict__ num_present, long long rows, int C,
    float* __restrict__ grad) {
  const long long r0 = (long long)blockIdx.x * kXentRows;
  const int nr = xent_block_rows(rows, r0);
  const int len = nr * C;  // <= 128 * 65535
  const long long base = r0 * C;
  const float* p = z + base;
  float* o = grad + base;
  const int n = *num_present;
  if (n == 0) {  // uniform: every element is 0
    for (int k = threadIdx.x; k < len; k += kXentBwdThreads) o[k] = 0.f;
    return;
  }
  const float g = *grad_loss, fn = (float)n;
  constexpr int kStep = kXentBwdThreads * W;
  const int dr = kStep / C, dc = kStep % C;
  const int lenw = len / W * W;
  int k = threadIdx.x * W;
  int r = k / C, c = k - r * C;
  int cur = -1, lab = -1;
  float l = 0.f, sc = 0.f;
  auto elem = [&](float v, int rr, int cc) {
    if (rr != cur) {
      cur = rr;
      l = lse[r0 + rr];
      lab = labels[r0 + rr];
      sc = __fdiv_rn(g * (weights ? weights[r0 + rr] : 1.f), fn);
    }
    return sc * (expf(v - l) - (cc == lab ? 1.f : 0.f));
  };
  for (; k < lenw; k += kStep) {
    int rr = r, cc = c;
    if (W == 4) {
      const float4 v = *reinterpret_cast<const float4*>(p + k);
      const float e[4] = {v.x, v.y, v.z, v.w};
      float out[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        out[j] = elem(e[j], rr, cc);
        if (++cc == C) {
          cc = 0;
          ++rr;
        }
      }
      *reinterpret_cast<float4*>(o + k) = make_float4(out[0], out[1], out[2], out[3]);
    } else {
      o[k] = elem(p[k], rr, cc);
    }
    r += dr;
    c += dc;
    if (c >= C) {
      c -= C;
      ++r;
    }
  }
  // the span's last len % W elements
  const int kt = lenw + threadIdx.x;
  if (kt < len) {
    const int rr = kt / C;
    o[kt] = elem(p[kt], rr, kt - rr * C);
  }
}

bool xent_shape_ok(long long rows, int C) {
  return rows > 0 && C > 0 && rows <= kXentMaxRows && C <= kXentMaxC;
}

}  // namespace
}  // namespace pn2

extern "C" {

int pn2_dropout(const float* x, long long n, float keep_prob, uint64_t seed, float* out,
                pn2_stream_t stream) {
  using namespace pn2;
  if (n < 0 || !(keep_prob > 0.f && keep_prob <= 1.f)) return PN2_EINVAL;
  if (n == 0) return PN2_OK;
  if (!x || !out) return PN2_EINVAL;
  const uint64_t thr = dropout_threshold(keep_prob);
  const uint64_t nq = ((uint64_t)n + 3) / 4;
  uint64_t blocks = (nq + kDropBlock - 1) / kDropBlock;
  if (blocks > kDropMaxGrid) blocks = kDropMaxGrid;  // grid-stride beyond
  const dim3 grid((unsigned)blocks);
  if (aligned16(x) && aligned16(out))
    hipLaunchKernelGGL(dropout_kernel<true>, grid, dim3(kDropBlock), 0, (hipStream_t)stream, x,
                       (uint64_t)n, keep_prob, thr, seed, out);
  else
    hipLaunchKernelGGL(dropout_kernel<false>, grid, dim3(kDropBlock), 0, (hipStream_t)stream, x,
                       (uint64_t)n, keep_prob, thr, seed, out);
  PN2_RETURN_LAUNCH();
}

size_t pn2_softmax_xent_workspace_size(long long rows) {
  if (rows <= 0) return 0;
  const size_t nblk = (size_t)((rows + pn2::kXentRows - 1) / pn2::kXentRows);
  return nblk * (sizeof(float) + sizeof(int32_t));  // the partial sums, then the counts
}

int pn2_softmax_xent_fwd(const float* logits, const int32_t* labels, const float* weights,
                         long long rows, int C, float* lse, int32_t* pred, float* loss,
                         int32_t* num_present, void* workspace, size_t workspace_bytes,
                         pn2_stream_t stream) {
  using namespace pn2;
  if (!xent_shape_ok(rows, C)) return PN2_EINVAL;
  if (!logits || !labels || !lse || !loss || !num_present || !workspace) return PN2_EINVAL;
  if (workspace_bytes < pn2_softmax_xent_workspace_size(rows)) return PN2_EINVAL;
  const int nblk = (int)((rows + kXentRows - 1) / kXentRows);
  float* part = static_cast<float*>(workspace);
  int32_t* cnt = reinterpret_cast<int32_t*>(part + nblk);
  hipStream_t s = (hipStream_t)stream;
  if (C <= kXentLdsMaxC) {
    const FastDiv divC = make_fastdiv((uint32_t)C);
    const size_t lds = (size_t)kXentRows * (C | 1) * sizeof(float);  // the kernel's odd stride
    if (aligned16(logits))
      hipLaunchKernelGGL(xent_fwd_lds<true>, dim3(nblk), dim3(kXentLdsThreads), lds, s, logits,
                         labels, weights, rows, C, divC, lse, pred, part, cnt);
    else
      hipLaunchKernelGGL(xent_fwd_lds<false>, dim3(nblk), dim3(kXentLdsThreads), lds, s, logits,
                         labels, weights, rows, C, divC, lse, pred, part, cnt);
  } else {
    hipLaunchKernelGGL(xent_fwd_wave, dim3(nblk), dim3(kXentWaveThreads), 0, s, logits, labels,
                       weights, rows, C, lse, pred, part, cnt);
  }
  hipLaunchKernelGGL(xent_final, dim3(1), dim3(kXentFinalThreads), 0, s, part, cnt, nblk, loss,
                     num_present);
  PN2_RETURN_LAUNCH();
}

int pn2_softmax_xent_bwd(const float* grad_loss, const float* logits, const int32_t* labels,
                         const float* weights, const float* lse, const int32_t* num_present,
                         long long rows, int C, float* grad_logits, pn2_stream_t stream) {
  using namespace pn2;
  if (!xent_shape_ok(rows, C)) return PN2_EINVAL;
  if (!grad_loss || !logits || !labels || !lse || !num_present || !grad_logits) return PN2_EINVAL;
  const int nblk = (int)((rows + kXentRows - 1) / kXentRows);
  hipStream_t s = (hipStream_t)stream;
  // a block's span starts at a multiple of 128 * C floats: aligned when the bases are
  if (aligned16(logits) && aligned16(grad_logits))
    hipLaunchKernelGGL(xent_bwd_kernel<4>, dim3(nblk), dim3(kXentBwdThreads), 0, s, grad_loss,
                       logits, labels, weights, lse, num_present, rows, C, grad_logits);
  else
    hipLaunchKernelGGL(xent_bwd_kernel<1>, dim3(nblk), dim3(kXentBwdThreads), 0, s, grad_loss,
                       logits, labels, weights, lse, num_present, rows, C, grad_logits);
  PN2_RETURN_LAUNCH();
}

}  // extern "C"
