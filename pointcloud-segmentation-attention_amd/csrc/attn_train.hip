// Training-mode attention reduction for gfx950: AttentionLayer.call's reduction core
// (attention_points/attention_scannet/attention_layer.py:35-42) and its gradient on K and V
// projected TOGETHER.
//
// KV = X [Wk | Wv] + [bk | bv] is one GEMM that reads X once; its output (G, ns, 2C) holds in row
// j of group g the K row (C floats) followed by the V row. The semantics are those of
// pn2_attn_reduce / pn2_attn_reduce_grad (attn.hip), the reshape quirk included: head h of
// group g reads the contiguous block [4 ns h, 4 ns (h + 1)) of the group's row-major (ns, C) K
// matrix as ns pseudo-keys of 4 floats. Only the addressing differs: pseudo-key i of head h is
// flat element f = 4 ns h + 4 i of K, i.e. KV[g][f / C][f % C .. + 3], and its value vector is
// KV[g][f / C][C + f % C .. + 3]. C % 4 == 0 and f % 4 == 0, so a pseudo-key never straddles a
// row, whether a head spans several rows (C < 4 ns), a row holds several heads, or neither
// divides the other.
//
// Forward: attn.hip's layouts and device functions (attn_dev.h) under attn.hip's dispatch rule,
// so the result has the bits of pn2_attn_reduce on de-interleaved copies of K and V.
//
// Backward, ns in {8, 16, 32, 64, 128}: the forward's lane layout. A lane holds its pseudo-keys'
// K and V float4s in registers, read once; the max, the normaliser and o are segment
// reductions; with s_i = q.K_i / 2, a = softmax(s), o = sum_i a_i V_i:
//   dV_i = a_i dO,   ds_i = a_i (dO.V_i - dO.o),   dK_i = ds_i q / 2,   dq = sum_i ds_i K_i / 2
// dK_i and dV_i are written once as float4, dq is one more segment sum. Every other ns: one
// wave per (group, head), lanes striding over the pseudo-keys. All reductions have a fixed
// order: two runs give equal bits.
//
// Also here: pn2_attn_dx_scatter (the query row's and the max pool's gradients added into
// grad_x at G x C elements). The bias gradients are pn2_col_sum (mlp_train.hip).
#include <math.h>

#include <initializer_list>

#include "attn_dev.h"
#include "chan_rows.h"
#include "common.h"

namespace pn2 {
namespace {

constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / kWave;
// the forward's launch shape is attn.hip's: 2 tasks in flight per wave, 8 workgroups per CU
// before the grid strides; the backward keeps one task per wave (twice the registers per task)
constexpr int kFwdTif = 2;
constexpr int kBlocksPerCu = 8;
constexpr int kGenericBlocksPerCu = 16;
constexpr long long kScatterMaxBlocks = 256LL * 16;

// Where pseudo-key f4 (in float4 units of the group's flat K matrix) lives in the group's
// interleaved rows: row f4 / C4, K at column 4 (f4 % C4), V at C floats after it.
struct KvAddr {
  uint32_t C4;
  FastDiv div;
  int fast;  // fdiv is exact for every f4 < ns * C4
};
PN2_DEV uint32_t kv_offset(uint32_t f4, const KvAddr& A) {
  const uint32_t row = A.fast ? fdiv(f4, A.div) : f4 / A.C4;
  return row * (8u * A.C4) + 4u * (f4 - row * A.C4);
}

// ---------------------------------------------------------------- forward ----------------
// attn.hip attn_reduce_kernel for one layer, K and V from the interleaved rows.
template <int NS, int TIF>
__global__ __launch_bounds__(kBlock) void attn_kv_reduce_kernel(
    const float* __restrict__ Q, const float* __restrict__ KV, int C, int steps, FastDiv div_steps,
    KvAddr A, long long tasks, float* __restrict__ out) {
  constexpr int LPH = NS < kWave ? NS : kWave;
  constexpr int KPL = NS / LPH;
  constexpr int HPW = kWave / LPH;  // heads per wave step
  const int lane = lane_id();
  const int hl = lane / LPH, sl = lane % LPH;
  const int H = C / 4;
  const long long nwaves = (long long)gridDim.x * kWavesPerBlock;
  for (long long t0 = (long long)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave; t0 < tasks;
       t0 += nwaves * TIF) {
    float4 q[TIF], k[TIF][KPL], v[TIF][KPL];
    float* op[TIF];
    bool ok[TIF];
#pragma unroll
    for (int i = 0; i < TIF; ++i) {
      long long task = t0 + i * nwaves;
      ok[i] = task < tasks;
      task = ok[i] ? task : t0;
      const uint32_t lt = (uint32_t)task;
      const uint32_t g = fdiv(lt, div_steps);
      const int step = (int)(lt - g * (uint32_t)steps);
      const int h = step * HPW + hl;
      ok[i] = ok[i] && h < H;
      const int hh = h < H ? h : 0;
      q[i] = *reinterpret_cast<const float4*>(Q + (size_t)g * C + 4 * hh);
      const float* KVg = KV + (size_t)g * NS * 2 * C;
#pragma unroll
      for (int kk = 0; kk < KPL; ++kk) {
        const uint32_t off = kv_offset((uint32_t)hh * NS + sl + kk * LPH, A);  // reshape quirk
        k[i][kk] = ld_stream(KVg + off);
        v[i][kk] = ld_stream(KVg + off + C);
      }
      op[i] = out + (size_t)g * C + 4 * h;
    }
#pragma unroll
    for (int i = 0; i < TIF; ++i) {
      float sc[KPL];
      float mx = -__builtin_inff();
#pragma unroll
      for (int kk = 0; kk < KPL; ++kk) {
        sc[kk] = dot4(q[i], k[i][kk]) / 2.0f;  // / tf.sqrt(key_dim = 4)  (:38)
        mx = fmaxf(mx, sc[kk]);
      }
      mx = seg_reduce<LPH, true>(mx);  // softmax over the ns pseudo-keys (:39)
      float sum = 0.0f;
#pragma unroll
      for (int kk = 0; kk < KPL; ++kk) {
        sc[kk] = expf(sc[kk] - mx);
        sum = sum + sc[kk];
      }
      sum = seg_reduce<LPH, false>(sum);
      float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int kk = 0; kk < KPL; ++kk) {
        const float w = sc[kk] / sum;
        o.x = o.x + w * v[i][kk].x;  // aᵀ·V_h (:40)
        o.y = o.y + w * v[i][kk].y;
        o.z = o.z + w * v[i][kk].z;
        o.w = o.w + w * v[i][kk].w;
      }
      o.x = seg_reduce<LPH, false>(o.x);
      o.y = seg_reduce<LPH, false>(o.y);
      o.z = seg_reduce<LPH, false>(o.z);
      o.w = seg_reduce<LPH, false>(o.w);
      if (sl == 0 && ok[i]) *reinterpret_cast<float4*>(op[i]) = o;  // (:42)
    }
  }
}

// attn.hip attn_reduce_generic_kernel on the interleaved rows: any nsample, one wave per
// (group, head).
__global__ __launch_bounds__(kBlock) void attn_kv_reduce_generic_kernel(
    const float* __restrict__ Q, const float* __restrict__ KV, long long G, int ns, int C,
    KvAddr A, float* __restrict__ out) {
  const int lane = lane_id();
  const int H = C / 4;
  const long long tasks = G * H;
  const long long nwaves = (long long)gridDim.x * kWavesPerBlock;
  for (long long task = (long long)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave; task < tasks;
       task += nwaves) {
    const long long g = task / H;
    const int h = (int)(task - g * H);
    const float4 q = *reinterpret_cast<const float4*>(Q + g * C + 4 * h);
    const float* KVg = KV + g * (long long)ns * 2 * C;
    const uint32_t f0 = (uint32_t)h * (uint32_t)ns;
    float mx = -__builtin_inff();
    for (int s = lane; s < ns; s += kWave)
      mx = fmaxf(mx, dot4(q, *reinterpret_cast<const float4*>(KVg + kv_offset(f0 + s, A))) / 2.0f);
    mx = seg_max<kWave>(mx);
    float sum = 0.f;
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int s = lane; s < ns; s += kWave) {
      const uint32_t off = kv_offset(f0 + s, A);
      const float e = expf(dot4(q, *reinterpret_cast<const float4*>(KVg + off)) / 2.0f - mx);
      const float4 v = *reinterpret_cast<const float4*>(KVg + off + C);
      sum = sum + e;
      o.x = o.x + e * v.x;
      o.y = o.y + e * v.y;
      o.z = o.z + e * v.z;
      o.w = o.w + e * v.w;
    }
    sum = seg_sum<kWave>(sum);
    o.x = seg_sum<kWave>(o.x) / sum;
    o.y = seg_sum<kWave>(o.y) / sum;
    o.z = seg_sum<kWave>(o.z) / sum;
    o.w = seg_sum<kWave>(o.w) / sum;
    if (lane == 0) *reinterpret_cast<float4*>(out + g * C + 4 * h) = o;
  }
}

// ---------------------------------------------------------------- backward ---------------
// The forward's lane layout: LPH lanes per head, KPL pseudo-keys per lane, HPW heads per wave
// task. K and V are read once and stay in registers; dK, dV are written once.
template <int NS>
__global__ __launch_bounds__(kBlock) void attn_kv_grad_kernel(
    const float* __restrict__ Q, const float* __restrict__ KV, const float* __restrict__ dO, int C,
    int steps, FastDiv div_steps, KvAddr A, long long tasks, float* __restrict__ dQ,
    float* __restrict__ dKV) {
  constexpr int LPH = NS < kWave ? NS : kWave;
  constexpr int KPL = NS / LPH;
  constexpr int HPW = kWave / LPH;
  const int lane = lane_id();
  const int hl = lane / LPH, sl = lane % LPH;
  const int H = C / 4;
  const long long nwaves = (long long)gridDim.x * kWavesPerBlock;
  for (long long task = (long long)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave; task < tasks;
       task += nwaves) {
    const uint32_t lt = (uint32_t)task;
    const uint32_t g = fdiv(lt, div_steps);
    const int step = (int)(lt - g * (uint32_t)steps);
    const int h = step * HPW + hl;
    const bool live = h < H;  // the last step of a group may hold fewer than HPW heads
    const int hh = live ? h : 0;
    const float4 q = *reinterpret_cast<const float4*>(Q + (size_t)g * C + 4 * hh);
    const float4 go = *reinterpret_cast<const float4*>(dO + (size_t)g * C + 4 * hh);
    const size_t base = (size_t)g * NS * 2 * C;
    uint32_t off[KPL];
    float4 k[KPL], v[KPL];
#pragma unroll
    for (int kk = 0; kk < KPL; ++kk) {
      off[kk] = kv_offset((uint32_t)hh * NS + sl + kk * LPH, A);  // reshape quirk (:35-36)
      k[kk] = ld_stream(KV + base + off[kk]);
      v[kk] = ld_stream(KV + base + off[kk] + C);
    }
    float a[KPL];
    float mx = -__builtin_inff();
#pragma unroll
    for (int kk = 0; kk < KPL; ++kk) {
      a[kk] = dot4(q, k[kk]) / 2.0f;
      mx = fmaxf(mx, a[kk]);
    }
    mx = seg_reduce<LPH, true>(mx);
    float sum = 0.0f;
#pragma unroll
    for (int kk = 0; kk < KPL; ++kk) {
      a[kk] = expf(a[kk] - mx);
      sum = sum + a[kk];
    }
    sum = seg_reduce<LPH, false>(sum);
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int kk = 0; kk < KPL; ++kk) {
      a[kk] = a[kk] / sum;
      o.x = o.x + a[kk] * v[kk].x;
      o.y = o.y + a[kk] * v[kk].y;
      o.z = o.z + a[kk] * v[kk].z;
      o.w = o.w + a[kk] * v[kk].w;
    }
    o.x = seg_reduce<LPH, false>(o.x);
    o.y = seg_reduce<LPH, false>(o.y);
    o.z = seg_reduce<LPH, false>(o.z);
    o.w = seg_reduce<LPH, false>(o.w);
    const float go_o = dot4(go, o);
    float4 gq = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int kk = 0; kk < KPL; ++kk) {
      const float ds = a[kk] * (dot4(go, v[kk]) - go_o);
      const float hds = ds / 2.0f;
      if (live) {
        *reinterpret_cast<float4*>(dKV + base + off[kk]) =
            make_float4(hds * q.x, hds * q.y, hds * q.z, hds * q.w);
        *reinterpret_cast<float4*>(dKV + base + off[kk] + C) =
            make_float4(a[kk] * go.x, a[kk] * go.y, a[kk] * go.z, a[kk] * go.w);
      }
      gq.x = gq.x + hds * k[kk].x;
      gq.y = gq.y + hds * k[kk].y;
      gq.z = gq.z + hds * k[kk].z;
      gq.w = gq.w + hds * k[kk].w;
    }
    gq.x = seg_reduce<LPH, false>(gq.x);
    gq.y = seg_reduce<LPH, false>(gq.y);
    gq.z = seg_reduce<LPH, false>(gq.z);
    gq.w = seg_reduce<LPH, false>(gq.w);
    if (sl == 0 && live) *reinterpret_cast<float4*>(dQ + (size_t)g * C + 4 * h) = gq;
  }
}

// Any nsample: one wave per (group, head), lanes striding over the pseudo-keys; the forward is
// recomputed (max, normaliser, o), then one pass writes dK and dV.
__global__ __launch_bounds__(kBlock) void attn_kv_grad_generic_kernel(
    const float* __restrict__ Q, const float* __restrict__ KV, const float* __restrict__ dO,
    long long G, int ns, int C, KvAddr A, float* __restrict__ dQ, float* __restrict__ dKV) {
  const int lane = lane_id();
  const int H = C / 4;
  const long long tasks = G * H;
  const long long nwaves = (long long)gridDim.x * kWavesPerBlock;
  for (long long task = (long long)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave; task < tasks;
       task += nwaves) {
    const long long g = task / H;
    const int h = (int)(task - g * H);
    const float4 q = *reinterpret_cast<const float4*>(Q + g * C + 4 * h);
    const float4 go = *reinterpret_cast<const float4*>(dO + g * C + 4 * h);
    const float* KVg = KV + g * (long long)ns * 2 * C;
    float* dKVg = dKV + g * (long long)ns * 2 * C;
    const uint32_t f0 = (uint32_t)h * (uint32_t)ns;
    float mx = -__builtin_inff();
    for (int s = lane; s < ns; s += kWave)
      mx = fmaxf(mx, dot4(q, *reinterpret_cast<const float4*>(KVg + kv_offset(f0 + s, A))) / 2.0f);
    mx = seg_max<kWave>(mx);
    float sum = 0.f;
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int s = lane; s < ns; s += kWave) {
      const uint32_t off = kv_offset(f0 + s, A);
      const float e = expf(dot4(q, *reinterpret_cast<const float4*>(KVg + off)) / 2.0f - mx);
      const float4 v = *reinterpret_cast<const float4*>(KVg + off + C);
      sum = sum + e;
      o.x = o.x + e * v.x;
      o.y = o.y + e * v.y;
      o.z = o.z + e * v.z;
      o.w = o.w + e * v.w;
    }
    sum = seg_sum<kWave>(sum);
    const float inv = 1.0f / sum;
    const float go_o = dot4(go, make_float4(seg_sum<kWave>(o.x) * inv, seg_sum<kWave>(o.y) * inv,
                                            seg_sum<kWave>(o.z) * inv, seg_sum<kWave>(o.w) * inv));
    float4 gq = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int s = lane; s < ns; s += kWave) {
      const uint32_t off = kv_offset(f0 + s, A);
      const float4 k = *reinterpret_cast<const float4*>(KVg + off);
      const float4 v = *reinterpret_cast<const float4*>(KVg + off + C);
      const float a = expf(dot4(q, k) / 2.0f - mx) * inv;
      const float ds = a * (dot4(go, v) - go_o);
      const float hds = ds / 2.0f;
      *reinterpret_cast<float4*>(dKVg + off) =
          make_float4(hds * q.x, hds * q.y, hds * q.z, hds * q.w);
      *reinterpret_cast<float4*>(dKVg + off + C) =
          make_float4(a * go.x, a * go.y, a * go.z, a * go.w);
      gq.x = gq.x + hds * k.x;
      gq.y = gq.y + hds * k.y;
      gq.z = gq.z + hds * k.z;
      gq.w = gq.w + hds * k.w;
    }
    gq.x = seg_sum<kWave>(gq.x);
    gq.y = seg_sum<kWave>(gq.y);
    gq.z = seg_sum<kWave>(gq.z);
    gq.w = seg_sum<kWave>(gq.w);
    if (lane == 0) *reinterpret_cast<float4*>(dQ + g * C + 4 * h) = gq;
  }
}

// ---------------------------------------------------------------- grad_x patches ---------
// One thread per (g, c): the query row's gradient into row 0, then the max pool's gradient into
// row arg[g][c]. Both adds by the same thread, in that order: no atomics.
__global__ __launch_bounds__(kBlock) void attn_dx_scatter_kernel(
    float* __restrict__ gx, const float* __restrict__ gxq, const float* __restrict__ gp,
    const int* __restrict__ arg, long long n, int ns, int C) {
  const long long stride = (long long)gridDim.x * kBlock;
  for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    const long long g = i / C;
    const int c = (int)(i - g * C);
    float* col = gx + g * ns * C + c;
    col[0] = col[0] + gxq[i];
    if (gp) {
      const int a = arg[i];
      if (a >= 0 && a < ns) col[(long long)a * C] = col[(long long)a * C] + gp[i];
    }
  }
}

// ---------------------------------------------------------------- launchers --------------
unsigned grid_for(long long waves, int per_cu) {
  long long blocks = (waves + kWavesPerBlock - 1) / kWavesPerBlock;
  if (blocks > 256LL * per_cu) blocks = 256LL * per_cu;  // grid-stride beyond
  return (unsigned)(blocks > 0 ? blocks : 1);
}

// attn.hip's rule: the specialised kernels' FastDiv task arithmetic stays exact
bool small_tasks(long long G, int C) {
  const long long steps_max = (long long)C / 4;
  return G * steps_max * steps_max < (1LL << 32);
}

KvAddr kv_addr(int ns, int C) {
  KvAddr A;
  A.C4 = (uint32_t)(C / 4);
  A.div = make_fastdiv(A.C4);
  // fdiv(f4, C4) is exact while f4 * C4 < 2^32, f4 < ns * C4
  A.fast = (unsigned long long)ns * A.C4 * A.C4 < (1ULL << 32) ? 1 : 0;
  return A;
}

template <int NS>
void launch_fwd(const float* Q, const float* KV, long long G, int C, float* out, hipStream_t s) {
  constexpr int LPH = NS < kWave ? NS : kWave;
  constexpr int HPW = kWave / LPH;
  const int steps = (C / 4 + HPW - 1) / HPW;
  const long long tasks = G * steps;
  hipLaunchKernelGGL((attn_kv_reduce_kernel<NS, kFwdTif>),
                     dim3(grid_for((tasks + kFwdTif - 1) / kFwdTif, kBlocksPerCu)), dim3(kBlock),
                     0, s, Q, KV, C, steps, make_fastdiv((uint32_t)steps), kv_addr(NS, C), tasks,
                     out);
}

template <int NS>
void launch_bwd(const float* Q, const float* KV, const float* dO, long long G, int C, float* dQ,
                float* dKV, hipStream_t s) {
  constexpr int LPH = NS < kWave ? NS : kWave;
  constexpr int HPW = kWave / LPH;
  const int steps = (C / 4 + HPW - 1) / HPW;
  const long long tasks = G * steps;
  hipLaunchKernelGGL((attn_kv_grad_kernel<NS>), dim3(grid_for(tasks, kBlocksPerCu)), dim3(kBlock),
                     0, s, Q, KV, dO, C, steps, make_fastdiv((uint32_t)steps), kv_addr(NS, C),
                     tasks, dQ, dKV);
}

bool specialised(int ns) { return ns == 8 || ns == 16 || ns == 32 || ns == 64 || ns == 128; }

// shapes both reductions take; 1: nothing to do, 0: launch, PN2_EINVAL
int kv_shape(long long G, int ns, int C) {
  if (G < 0 || ns <= 0 || C < 0 || (C % 4) != 0) return PN2_EINVAL;
  if (G == 0 || C == 0) return 1;
  // a group's interleaved rows are addressed in 32 bits, the groups in 64
  if (G > INT32_MAX || (long long)ns * C > INT32_MAX / 2) return PN2_EINVAL;
  return 0;
}

}  // namespace
}  // namespace pn2

extern "C" {

int pn2_attn_kv_reduce(const float* Q, const float* KV, long long G, int ns, int C, float* out,
                       pn2_stream_t stream) {
  using namespace pn2;
  const int sh = kv_shape(G, ns, C);
  if (sh) return sh < 0 ? sh : PN2_OK;
  if (!Q || !KV || !out || !aligned16(Q, KV, out)) return PN2_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (small_tasks(G, C) && specialised(ns)) {
    if (ns == 8) launch_fwd<8>(Q, KV, G, C, out, s);
    else if (ns == 16) launch_fwd<16>(Q, KV, G, C, out, s);
    else if (ns == 32) launch_fwd<32>(Q, KV, G, C, out, s);
    else if (ns == 64) launch_fwd<64>(Q, KV, G, C, out, s);
    else launch_fwd<128>(Q, KV, G, C, out, s);
  } else {
    hipLaunchKernelGGL(attn_kv_reduce_generic_kernel,
                       dim3(grid_for(G * (C / 4), kGenericBlocksPerCu)), dim3(kBlock), 0, s, Q, KV,
                       G, ns, C, kv_addr(ns, C), out);
  }
  PN2_RETURN_LAUNCH();
}

int pn2_attn_kv_reduce_grad(const float* Q, const float* KV, const float* grad_out, long long G,
                            int ns, int C, float* grad_Q, float* grad_KV, pn2_stream_t stream) {
  using namespace pn2;
  const int sh = kv_shape(G, ns, C);
  if (sh) return sh < 0 ? sh : PN2_OK;
  if (!Q || !KV || !grad_out || !grad_Q || !grad_KV) return PN2_EINVAL;
  if (!aligned16(Q, KV, grad_out, grad_Q, grad_KV)) return PN2_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (small_tasks(G, C) && specialised(ns)) {
    if (ns == 8) launch_bwd<8>(Q, KV, grad_out, G, C, grad_Q, grad_KV, s);
    else if (ns == 16) launch_bwd<16>(Q, KV, grad_out, G, C, grad_Q, grad_KV, s);
    else if (ns == 32) launch_bwd<32>(Q, KV, grad_out, G, C, grad_Q, grad_KV, s);
    else if (ns == 64) launch_bwd<64>(Q, KV, grad_out, G, C, grad_Q, grad_KV, s);
    else launch_bwd<128>(Q, KV, grad_out, G, C, grad_Q, grad_KV, s);
  } else {
    hipLaunchKernelGGL(attn_kv_grad_generic_kernel,
                       dim3(grid_for(G * (C / 4), kGenericBlocksPerCu)), dim3(kBlock), 0, s, Q, KV,
                       grad_out, G, ns, C, kv_addr(ns, C), grad_Q, grad_KV);
  }
  PN2_RETURN_LAUNCH();
}

int pn2_attn_dx_scatter(float* grad_x, const float* grad_xq, const float* grad_pmax,
                        const int* arg, long long G, int ns, int C, pn2_stream_t stream) {
  using namespace pn2;
  if (G < 0 || ns <= 0 || C < 0) return PN2_EINVAL;
  if ((grad_pmax != nullptr) != (arg != nullptr)) return PN2_EINVAL;
  if (G == 0 || C == 0) return PN2_OK;
  using chan_rows::kMaxRows;
  if (!grad_x || !grad_xq || G > kMaxRows || G * ns > kMaxRows) return PN2_EINVAL;
  const long long n = G * C;
  long long blocks = (n + kBlock - 1) / kBlock;
  if (blocks > kScatterMaxBlocks) blocks = kScatterMaxBlocks;  // grid-stride beyond
  hipLaunchKernelGGL(attn_dx_scatter_kernel, dim3((unsigned)blocks), dim3(kBlock), 0,
                     (hipStream_t)stream, grad_x, grad_xq, grad_pmax, arg, n, ns, C);
  PN2_RETURN_LAUNCH();
}

}  // extern "C"
