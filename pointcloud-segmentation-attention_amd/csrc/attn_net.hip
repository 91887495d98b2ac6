// The attention networks' two reductions for gfx950 (attention_points/attention_scannet:
// AttentionNetLayer, AttentionNetMLPLayer, PoolingAttentionNetLayer, InnerAttentionLayer).
//
// 1. pn2_attn_reduce_kd: AttentionLayer.call (attention_layer.py:29-45) for any key_dim = kd
//    (the net layers build AttentionLayer(out_dim, key_dim=out_dim) at :142, :185 and
//    pooling_attention_layer.py:17, kd = 8 .. 512, 16 heads). The reshape quirk of attn.hip holds
//    for every kd: head h of a group is the CONTIGUOUS run [h*ns*kd, (h+1)*ns*kd) of the group's
//    ns*C values, read as ns rows of kd. One wave owns one (group, head): LPR = kd/4 lanes lie
//    along a row with one float4 each (kd = 512: two), so 64/LPR rows make one 1 KiB wave load;
//    the score is a sum over the LPR lanes of a row segment (xor_reduce below: DPP and the
//    permlane swaps), and every lane keeps a running (max, sum, weighted sum) for its row slot
//    over the ns/(64/LPR) iterations, merged across the row slots once per head. K and V are
//    read once (streamed); nothing but 2 + 4*VPL floats per lane lives across iterations.
//    A kd/4 that is no power of two runs on the next power of two of lanes, the rest masked
//    (correct, less well coalesced); any ns runs on the same loop with the last rows masked.
//    The backward recomputes the forward, then reads the slab again (it is in the caches) and
//    writes every element of grad_K, grad_V and grad_Q once: no atomics.
// 2. pn2_head_mix: InnerAttentionLayer.call (:61-78), the H x H attention among the heads of ONE
//    point (it does not look across the group). LPR lanes hold one row's kd columns as float4,
//    the row's H keys and values stay in registers, and 64/LPR rows share a wave.
#include <math.h>

#include "attn_dev.h"
#include "common.h"

namespace pn2 {
namespace {

constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / kWave;
// blocks before the grid strides: 16 per CU (the tests step one task past it)
constexpr long long kMaxBlocks = PN2_ATTN_NET_MAX_BLOCKS;
constexpr int kMaxHeads = PN2_HEAD_MIX_MAX_HEADS;
constexpr int kDppRor8 = 0x128;  // row_ror:8 (lane i <- lane i ^ 8 within 16)

unsigned grid_for(long long waves) {
  long long blocks = (waves + kWavesPerBlock - 1) / kWavesPerBlock;
  if (blocks > kMaxBlocks) blocks = kMaxBlocks;  // grid-stride beyond
  return (unsigned)(blocks > 0 ? blocks : 1);
}

// v op (v of lane ^ OFF): every lane has a source, both lanes of a pair get the same bits
template <int OFF, bool MAX>
PN2_DEV float xor_step(float v) {
  auto op = [](float a, float b) { return MAX ? fmaxf(a, b) : a + b; };
  if constexpr (OFF == 1) return op(v, dpp_get<kDppXor1, false>(v));
  else if constexpr (OFF == 2) return op(v, dpp_get<kDppXor2, false>(v));
  else if constexpr (OFF == 4) return op(v, __shfl_xor(v, 4, kWave));
  else if constexpr (OFF == 8) return op(v, dpp_get<kDppRor8, false>(v));
  else if constexpr (OFF == 16) return row_swap_op<16>(v, op);
  else return row_swap_op<32>(v, op);
}
// sum / max over the lanes that differ in the lane-index bits [LO, HI) (powers of two):
// <1, LPR> is a row segment, <LPR, 64> the lanes of one column across the row slots
template <int LO, int HI, bool MAX>
PN2_DEV float xor_reduce(float v) {
  if constexpr (LO <= 1 && 1 < HI) v = xor_step<1, MAX>(v);
  if constexpr (LO <= 2 && 2 < HI) v = xor_step<2, MAX>(v);
  if constexpr (LO <= 4 && 4 < HI) v = xor_step<4, MAX>(v);
  if constexpr (LO <= 8 && 8 < HI) v = xor_step<8, MAX>(v);
  if constexpr (LO <= 16 && 16 < HI) v = xor_step<16, MAX>(v);
  if constexpr (LO <= 32 && 32 < HI) v = xor_step<32, MAX>(v);
  return v;
}

PN2_DEV float4 f4zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
PN2_DEV float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
PN2_DEV void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
PN2_DEV float4 scale4(float a, float4 v) { return make_float4(a * v.x, a * v.y, a * v.z, a * v.w); }
PN2_DEV void axpy4(float4& o, float a, float4 v) {  // o += a v, product rounded, then added
  o.x = o.x + a * v.x;
  o.y = o.y + a * v.y;
  o.z = o.z + a * v.z;
  o.w = o.w + a * v.w;
}

// One (group, head) of the reduction. LPR lanes per row, VPL float4 per lane and row (column
// c + j*LPR), RPI = 64 / LPR rows per iteration; nq = kd/4 valid columns.
template <int LPR, int VPL>
struct HeadTask {
  static constexpr int RPI = kWave / LPR;
  int r, c, nq;
  bool cok[VPL];
  float4 q[VPL];
  const float* Kh;
  const float* Vh;

  PN2_DEV void init(int lane, const float* Q, const float* K, const float* V, long long g, int h,
                    int H, int ns, int kd) {
    r = lane / LPR;
    c = lane % LPR;
    nq = kd / 4;
    const long long C = (long long)H * kd;
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
      cok[j] = c + j * LPR < nq;
      q[j] = cok[j] ? ld4(Q + g * C + (long long)h * kd + 4 * (c + j * LPR)) : f4zero();
    }
    const long long off = g * ns * C + (long long)h * ns * kd;  // reshape quirk (:35-36)
    Kh = K + off;
    Vh = V + off;
  }
  // row s of the head's slab at this lane's columns (zeros outside the slab)
  PN2_DEV void load(const float* base, int s, bool rok, int kd, float4 (&x)[VPL]) const {
#pragma unroll
    for (int j = 0; j < VPL; ++j)
      x[j] = rok && cok[j] ? ld_stream(base + (long long)s * kd + 4 * (c + j * LPR)) : f4zero();
  }
  // sum over the row's lanes of this lane's part of a . b
  PN2_DEV float row_dot(const float4 (&a)[VPL], const float4 (&b)[VPL]) const {
    float d = dot4(a[0], b[0]);
#pragma unroll
    for (int j = 1; j < VPL; ++j) d = d + dot4(a[j], b[j]);
    return xor_reduce<1, LPR, false>(d);
  }
  // softmax statistics and output of the head: mx and sum in every lane, o = this lane's columns
  // of a^T V_h (:37-40), the same bits in every row slot
  PN2_DEV void forward(int ns, int kd, float rs, float& mx, float& sum, float4 (&o)[VPL]) const {
    float m = -__builtin_inff(), l = 0.f;
#pragma unroll
    for (int j = 0; j < VPL; ++j) o[j] = f4zero();
    for (int s0 = 0; s0 < ns; s0 += RPI) {
      const int s = s0 + r;
      const bool rok = s < ns;
      float4 k[VPL], v[VPL];
      load(Kh, s, rok, kd, k);
      load(Vh, s, rok, kd, v);
      const float sc = row_dot(q, k) / rs;  // / tf.sqrt(key_dim) (:38)
      if (rok) {  // running max: exp(-inf) = 0 drops the empty state
        const float mn = fmaxf(m, sc);
        const float f = expf(m - mn), p = expf(sc - mn);
        l = l * f + p;
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
          o[j] = scale4(f, o[j]);
          axpy4(o[j], p, v[j]);
        }
        m = mn;
      }
    }
    // the row slots of one column (slot 0 always holds a row: ns >= 1)
    mx = xor_reduce<LPR, kWave, true>(m);
    const float f = m == -__builtin_inff() ? 0.f : expf(m - mx);
    sum = xor_reduce<LPR, kWave, false>(l * f);
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
      o[j].x = xor_reduce<LPR, kWave, false>(o[j].x * f) / sum;
      o[j].y = xor_reduce<LPR, kWave, false>(o[j].y * f) / sum;
      o[j].z = xor_reduce<LPR, kWave, false>(o[j].z * f) / sum;
      o[j].w = xor_reduce<LPR, kWave, false>(o[j].w * f) / sum;
    }
  }
};

template <int LPR, int VPL>
__global__ __launch_bounds__(kBlock) void attn_kd_kernel(
    const float* __restrict__ Q, const float* __restrict__ K, const float* __restrict__ V,
    long long tasks, int H, int ns, int kd, float rs, float* __restrict__ out) {
  const int lane = lane_id();
  const long long nwaves = (long long)gridDim.x * kWavesPerBlock;
  for (long long task = (long long)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave; task < tasks;
       task += nwaves) {
    const long long g = task / H;
    const int h = (int)(task - g * H);
    HeadTask<LPR, VPL> t;
    t.init(lane, Q, K, V, g, h, H, ns, kd);
    float mx, sum;
    float4 o[VPL];
    t.forward(ns, kd, rs, mx, sum, o);
    if (t.r == 0) {
#pragma unroll
      for (int j = 0; j < VPL; ++j)
        if (t.cok[j]) st4(out + (g * H + h) * kd + 4 * (t.c + j * LPR), o[j]);  // (:42)
    }
  }
}

// Backward, the formulas of attn_reduce_grad_kernel (attn.hip) with kd columns: s_i = q.K_i / rs,
// a = softmax(s), o = sum_i a_i V_i;  dV_i = a_i dO,  ds_i = a_i (dO.V_i - dO.o),
// dK_i = ds_i q / rs,  dq = sum_i ds_i K_i / rs.
template <int LPR, int VPL>
__global__ __launch_bounds__(kBlock) void attn_kd_grad_kernel(
    const float* __restrict__ Q, const float* __restrict__ K, const float* __restrict__ V,
    const float* __restrict__ dO, long long tasks, int H, int ns, int kd, float rs,
    float* __restrict__ dQ, float* __restrict__ dK, float* __restrict__ dV) {
  constexpr int RPI = kWave / LPR;
  const int lane = lane_id();
  const long long nwaves = (long long)gridDim.x * kWavesPerBlock;
  for (long long task = (long long)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave; task < tasks;
       task += nwaves) {
    const long long g = task / H;
    const int h = (int)(task - g * H);
    HeadTask<LPR, VPL> t;
    t.init(lane, Q, K, V, g, h, H, ns, kd);
    float mx, sum;
    float4 o[VPL], go[VPL], gq[VPL];
    t.forward(ns, kd, rs, mx, sum, o);
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
      go[j] = t.cok[j] ? ld4(dO + (g * H + h) * kd + 4 * (t.c + j * LPR)) : f4zero();
      gq[j] = f4zero();
    }
    const float go_o = t.row_dot(go, o);
    float* dKh = dK + (t.Kh - K);
    float* dVh = dV + (t.Vh - V);
    for (int s0 = 0; s0 < ns; s0 += RPI) {
      const int s = s0 + t.r;
      const bool rok = s < ns;
      float4 k[VPL], v[VPL];
      t.load(t.Kh, s, rok, kd, k);
      t.load(t.Vh, s, rok, kd, v);
      const float sc = t.row_dot(t.q, k) / rs;
      const float gv = t.row_dot(go, v);
      if (rok) {
        const float a = expf(sc - mx) / sum;
        const float hds = a * (gv - go_o) / rs;
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
          if (t.cok[j]) {
            const long long at = (long long)s * kd + 4 * (t.c + j * LPR);
            st4(dVh + at, scale4(a, go[j]));
            st4(dKh + at, scale4(hds, t.q[j]));
          }
          axpy4(gq[j], hds, k[j]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
      gq[j].x = xor_reduce<LPR, kWave, false>(gq[j].x);
      gq[j].y = xor_reduce<LPR, kWave, false>(gq[j].y);
      gq[j].z = xor_reduce<LPR, kWave, false>(gq[j].z);
      gq[j].w = xor_reduce<LPR, kWave, false>(gq[j].w);
      if (t.r == 0 && t.cok[j]) st4(dQ + (g * H + h) * kd + 4 * (t.c + j * LPR), gq[j]);
    }
  }
}

// ---- head mixing --------------------------------------------------------------------------
// qkv (rows, 3 W), W = H kd, one row = [Q_0..Q_{H-1} | K_0.. | V_0..]. LPR lanes hold one row's
// columns (float4 each), 64 / LPR rows per wave task; the loops over heads are unrolled to
// kMaxHeads behind wave-uniform tests so K and V index registers.
template <int LPR>
struct MixRow {
  static constexpr int RPW = kWave / LPR;
  bool ok;
  const float* p;  // the row's Q_0 at this lane's columns
  long long row;
  int c;
  PN2_DEV void init(int lane, const float* qkv, long long task, long long rows, int W, int kd) {
    c = lane % LPR;
    row = task * RPW + lane / LPR;
    ok = row < rows && c < kd / 4;
    p = qkv + (ok ? row : 0) * 3 * W + 4 * (ok ? c : 0);
  }
  PN2_DEV float4 ld(const float* at) const { return ok ? ld_stream(at) : f4zero(); }
};

template <int LPR>
__global__ __launch_bounds__(kBlock) void head_mix_kernel(const float* __restrict__ qkv,
                                                          long long rows, int H, int kd, float rs,
                                                          float* __restrict__ out) {
  const int lane = lane_id();
  const int W = H * kd;
  const long long tasks = (rows + MixRow<LPR>::RPW - 1) / MixRow<LPR>::RPW;
  const long long nwaves = (long long)gridDim.x * kWavesPerBlock;
  for (long long task = (long long)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave; task < tasks;
       task += nwaves) {
    MixRow<LPR> t;
    t.init(lane, qkv, task, rows, W, kd);
    float4 k[kMaxHeads], v[kMaxHeads];
#pragma unroll
    for (int j = 0; j < kMaxHeads; ++j) {
      k[j] = v[j] = f4zero();
      if (j < H) {
        k[j] = t.ld(t.p + W + j * kd);
        v[j] = t.ld(t.p + 2 * W + j * kd);
      }
    }
#pragma unroll
    for (int i = 0; i < kMaxHeads; ++i) {
      if (i < H) {
        const float4 q = t.ld(t.p + i * kd);
        float s[kMaxHeads];
        float mx = -__builtin_inff();
#pragma unroll
        for (int j = 0; j < kMaxHeads; ++j) {
          s[j] = 0.f;
          if (j < H) {
            s[j] = xor_reduce<1, LPR, false>(dot4(q, k[j])) / rs;  // (Q_i . K_j) / sqrt(kd)
            mx = fmaxf(mx, s[j]);
          }
        }
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < kMaxHeads; ++j)
          if (j < H) {
            s[j] = expf(s[j] - mx);
            sum = sum + s[j];
          }
        float4 o = f4zero();
#pragma unroll
        for (int j = 0; j < kMaxHeads; ++j)
          if (j < H) axpy4(o, s[j] / sum, v[j]);
        if (t.ok) st4(out + t.row * W + i * kd + 4 * t.c, o);
      }
    }
  }
}

// Backward per row, A recomputed: dV_j = sum_i A_ij dO_i, dA_ij = dO_i . V_j,
// dS_ij = A_ij (dA_ij - sum_j' A_ij' dA_ij'), dQ_i = sum_j dS_ij K_j / rs,
// dK_j = sum_i dS_ij Q_i / rs. grad_qkv has qkv's layout; every element written once.
template <int LPR>
__global__ __launch_bounds__(kBlock) void head_mix_grad_kernel(
    const float* __restrict__ qkv, const float* __restrict__ dO, long long rows, int H, int kd,
    float rs, float* __restrict__ dqkv) {
  const int lane = lane_id();
  const int W = H * kd;
  const long long tasks = (rows + MixRow<LPR>::RPW - 1) / MixRow<LPR>::RPW;
  const long long nwaves = (long long)gridDim.x * kWavesPerBlock;
  for (long long task = (long long)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave; task < tasks;
       task += nwaves) {
    MixRow<LPR> t;
    t.init(lane, qkv, task, rows, W, kd);
    float* gp = dqkv + (t.p - qkv);
    const float* gop = dO + (t.ok ? t.row : 0) * W + 4 * (t.ok ? t.c : 0);
    float4 k[kMaxHeads], v[kMaxHeads], gk[kMaxHeads], gv[kMaxHeads];
#pragma unroll
    for (int j = 0; j < kMaxHeads; ++j) {
      k[j] = v[j] = gk[j] = gv[j] = f4zero();
      if (j < H) {
        k[j] = t.ld(t.p + W + j * kd);
        v[j] = t.ld(t.p + 2 * W + j * kd);
      }
    }
#pragma unroll
    for (int i = 0; i < kMaxHeads; ++i) {
      if (i < H) {
        const float4 q = t.ld(t.p + i * kd);
        const float4 go = t.ld(gop + i * kd);
        float a[kMaxHeads], da[kMaxHeads];
        float mx = -__builtin_inff();
#pragma unroll
        for (int j = 0; j < kMaxHeads; ++j) {
          a[j] = da[j] = 0.f;
          if (j < H) {
            a[j] = xor_reduce<1, LPR, false>(dot4(q, k[j])) / rs;
            da[j] = xor_reduce<1, LPR, false>(dot4(go, v[j]));
            mx = fmaxf(mx, a[j]);
          }
        }
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < kMaxHeads; ++j)
          if (j < H) {
            a[j] = expf(a[j] - mx);
            sum = sum + a[j];
          }
        float ada = 0.f;
#pragma unroll
        for (int j = 0; j < kMaxHeads; ++j)
          if (j < H) {
            a[j] = a[j] / sum;
            ada = ada + a[j] * da[j];
          }
        float4 gq = f4zero();
#pragma unroll
        for (int j = 0; j < kMaxHeads; ++j)
          if (j < H) {
            const float ds = a[j] * (da[j] - ada) / rs;
            axpy4(gv[j], a[j], go);
            axpy4(gk[j], ds, q);
            axpy4(gq, ds, k[j]);
          }
        if (t.ok) st4(gp + i * kd, gq);
      }
    }
#pragma unroll
    for (int j = 0; j < kMaxHeads; ++j)
      if (j < H && t.ok) {
        st4(gp + W + j * kd, gk[j]);
        st4(gp + 2 * W + j * kd, gv[j]);
      }
  }
}

int pow2_lanes(int nq) {  // lanes along a row: the next power of two >= nq, at most a wave
  int l = 1;
  while (l < nq && l < kWave) l *= 2;
  return l;
}

bool attn_kd_args_ok(int B, int M, int ns, int C, int kd) {
  return B >= 0 && M >= 0 && ns >= 1 && C >= 0 && kd >= 4 && kd <= 512 && kd % 4 == 0 &&
         C % kd == 0;
}

bool head_mix_args_ok(long long rows, int heads, int kd) {
  return rows >= 0 && heads >= 1 && heads <= kMaxHeads && kd >= 4 && kd <= 256 && kd % 4 == 0;
}

}  // namespace
}  // namespace pn2

// one launch per lanes-per-row instance (kd / 4 rounded up to a power of two; above a wave two
// float4 per lane)
#define PN2_ATTN_KD_DISPATCH(KERNEL, lanes, nq, ...)                                        \
  do {                                                                                      \
    if ((nq) > pn2::kWave) hipLaunchKernelGGL((pn2::KERNEL<64, 2>), __VA_ARGS__);           \
    else if ((lanes) == 64) hipLaunchKernelGGL((pn2::KERNEL<64, 1>), __VA_ARGS__);          \
    else if ((lanes) == 32) hipLaunchKernelGGL((pn2::KERNEL<32, 1>), __VA_ARGS__);          \
    else if ((lanes) == 16) hipLaunchKernelGGL((pn2::KERNEL<16, 1>), __VA_ARGS__);          \
    else if ((lanes) == 8) hipLaunchKernelGGL((pn2::KERNEL<8, 1>), __VA_ARGS__);            \
    else if ((lanes) == 4) hipLaunchKernelGGL((pn2::KERNEL<4, 1>), __VA_ARGS__);            \
    else hipLaunchKernelGGL((pn2::KERNEL<2, 1>), __VA_ARGS__);                              \
  } while (0)

#define PN2_HEAD_MIX_DISPATCH(KERNEL, lanes, ...)                                           \
  do {                                                                                      \
    if ((lanes) == 64) hipLaunchKernelGGL((pn2::KERNEL<64>), __VA_ARGS__);                  \
    else if ((lanes) == 32) hipLaunchKernelGGL((pn2::KERNEL<32>), __VA_ARGS__);             \
    else if ((lanes) == 16) hipLaunchKernelGGL((pn2::KERNEL<16>), __VA_ARGS__);             \
    else if ((lanes) == 8) hipLaunchKernelGGL((pn2::KERNEL<8>), __VA_ARGS__);               \
    else if ((lanes) == 4) hipLaunchKernelGGL((pn2::KERNEL<4>), __VA_ARGS__);               \
    else if ((lanes) == 2) hipLaunchKernelGGL((pn2::KERNEL<2>), __VA_ARGS__);               \
    else hipLaunchKernelGGL((pn2::KERNEL<1>), __VA_ARGS__);                                 \
  } while (0)

extern "C" {

int pn2_attn_reduce_kd(const float* Q, const float* K, const float* V, int B, int M, int ns,
                       int C, int key_dim, float* out, pn2_stream_t stream) {
  if (!pn2::attn_kd_args_ok(B, M, ns, C, key_dim)) return PN2_EINVAL;
  if (!pn2::aligned16(Q, K, V, out)) return PN2_EINVAL;
  if (key_dim == 4) return pn2_attn_reduce(Q, K, V, B, M, ns, C, out, stream);
  const long long G = (long long)B * M;
  if (G == 0 || C == 0) return PN2_OK;
  if (!Q || !K || !V || !out || G > INT32_MAX) return PN2_EINVAL;
  const int H = C / key_dim, nq = key_dim / 4, lanes = pn2::pow2_lanes(nq);
  const long long tasks = G * H;
  const float rs = sqrtf((float)key_dim);
  PN2_ATTN_KD_DISPATCH(attn_kd_kernel, lanes, nq, dim3(pn2::grid_for(tasks)), dim3(pn2::kBlock),
                       0, (hipStream_t)stream, Q, K, V, tasks, H, ns, key_dim, rs, out);
  PN2_RETURN_LAUNCH();
}

int pn2_attn_reduce_kd_grad(const float* Q, const float* K, const float* V, const float* grad_out,
                            int B, int M, int ns, int C, int key_dim, float* grad_Q,
                            float* grad_K, float* grad_V, pn2_stream_t stream) {
  if (!pn2::attn_kd_args_ok(B, M, ns, C, key_dim)) return PN2_EINVAL;
  if (!pn2::aligned16(Q, K, V, grad_out, grad_Q, grad_K, grad_V)) return PN2_EINVAL;
  if (key_dim == 4)
    return pn2_attn_reduce_grad(Q, K, V, grad_out, B, M, ns, C, grad_Q, grad_K, grad_V, stream);
  const long long G = (long long)B * M;
  if (G == 0 || C == 0) return PN2_OK;
  if (!Q || !K || !V || !grad_out || !grad_Q || !grad_K || !grad_V || G > INT32_MAX)
    return PN2_EINVAL;
  const int H = C / key_dim, nq = key_dim / 4, lanes = pn2::pow2_lanes(nq);
  const long long tasks = G * H;
  const float rs = sqrtf((float)key_dim);
  PN2_ATTN_KD_DISPATCH(attn_kd_grad_kernel, lanes, nq, dim3(pn2::grid_for(tasks)),
                       dim3(pn2::kBlock), 0, (hipStream_t)stream, Q, K, V, grad_out, tasks, H, ns,
                       key_dim, rs, grad_Q, grad_K, grad_V);
  PN2_RETURN_LAUNCH();
}

int pn2_head_mix(const float* qkv, long long rows, int heads, int key_dim, float* out,
                 pn2_stream_t stream) {
  if (!pn2::head_mix_args_ok(rows, heads, key_dim)) return PN2_EINVAL;
  if (!pn2::aligned16(qkv, out)) return PN2_EINVAL;
  if (rows == 0) return PN2_OK;
  if (!qkv || !out) return PN2_EINVAL;
  const int lanes = pn2::pow2_lanes(key_dim / 4);
  const long long tasks = (rows + pn2::kWave / lanes - 1) / (pn2::kWave / lanes);
  const float rs = sqrtf((float)key_dim);
  PN2_HEAD_MIX_DISPATCH(head_mix_kernel, lanes, dim3(pn2::grid_for(tasks)), dim3(pn2::kBlock), 0,
                        (hipStream_t)stream, qkv, rows, heads, key_dim, rs, out);
  PN2_RETURN_LAUNCH();
}

int pn2_head_mix_grad(const float* qkv, const float* grad_out, long long rows, int heads,
                      int key_dim, float* grad_qkv, pn2_stream_t stream) {
  if (!pn2::head_mix_args_ok(rows, heads, key_dim)) return PN2_EINVAL;
  if (!pn2::aligned16(qkv, grad_out, grad_qkv)) return PN2_EINVAL;
  if (rows == 0) return PN2_OK;
  if (!qkv || !grad_out || !grad_qkv) return PN2_EINVAL;
  const int lanes = pn2::pow2_lanes(key_dim / 4);
  const long long tasks = (rows + pn2::kWave / lanes - 1) / (pn2::kWave / lanes);
  const float rs = sqrtf((float)key_dim);
  PN2_HEAD_MIX_DISPATCH(head_mix_grad_kernel, lanes, dim3(pn2::grid_for(tasks)),
                        dim3(pn2::kBlock), 0, (hipStream_t)stream, qkv, grad_out, rows, heads,
                        key_dim, rs, grad_qkv);
  PN2_RETURN_LAUNCH();
}

}  // extern "C"
