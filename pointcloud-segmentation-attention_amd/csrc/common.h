// Shared device helpers for the gfx950 kernels of libpn2hip.so.
//
// Every translation unit is compiled with -ffp-contract=off AND starts with
// `#pragma clang fp contract(off)`: the reference's index results (FPS argmax, ball-query
// membership, three_nn order) depend on un-fused fp32 `(dx*dx+dy*dy)+dz*dz`, which is what
// the reference CPU code computes under plain `g++ -O2` (tf_interpolate_compile.sh:2,
// grouping/test/compile.sh:1). An FMA would change the rounding of d2 and therefore indices.
#pragma once
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pn2hip.h"

#define PN2_DEV __device__ __forceinline__

namespace pn2 {

constexpr int kWave = 64;  // CDNA wavefront

// Squared distance exactly as the reference writes it: (x2-x1)*(x2-x1)+(y2-y1)*(y2-y1)+
// (z2-z1)*(z2-z1), evaluated left to right in fp32 with no contraction
// (tf_sampling_g.cu:142, tf_grouping_g.cu:24, tf_interpolate.cpp:73).
PN2_DEV float sqdist(float ax, float ay, float az, float bx, float by, float bz) {
  const float dx = ax - bx;
  const float dy = ay - by;
  const float dz = az - bz;
  float d = __fmul_rn(dx, dx);
  d = __fadd_rn(d, __fmul_rn(dy, dy));
  d = __fadd_rn(d, __fmul_rn(dz, dz));
  return d;
}

// ---- wave-level reductions (64 lanes, result in every lane) ----------------------------
// Rows of 16 lanes are reduced with DPP (quad_perm xor1/xor2, row_half_mirror, row_mirror),
// then rows are combined with the gfx950 v_permlane16_swap / v_permlane32_swap exchanges:
// no LDS round trip, no ds_bpermute.
constexpr int kDppXor1 = 0xB1;        // quad_perm [1,0,3,2]
constexpr int kDppXor2 = 0x4E;        // quad_perm [2,3,0,1]
constexpr int kDppHalfMirror = 0x141; // row_half_mirror (lane i <-> 7-i within 8)
constexpr int kDppMirror = 0x140;     // row_mirror (lane i <-> 15-i within 16)

// The pattern, once, for a 32-bit T: op over aligned segments of SEG = 4..64 lanes, every lane
// of a segment ends with the same value. Every lane has a valid source in these DPP patterns,
// so the move's old value is never used; which one is named still decides the code. 0 lets the
// move fold into the operation (v_max_u32_dpp and its kin: one instruction per step);
// OLD_SELF names the value itself and keeps a v_mov_b32_dpp per step: the float min / max use
// it, because with 0 the kernels around them (grid builds, FP search, sampler boxes) come out
// with other schedules and registers.
template <int CTRL, bool OLD_SELF, typename T>
PN2_DEV T dpp_get(T v) {
  const int u = __builtin_bit_cast(int, v);
  return __builtin_bit_cast(
      T, __builtin_amdgcn_update_dpp(OLD_SELF ? u : 0, u, CTRL, 0xF, 0xF, false));
}
template <int ROWS, typename T, typename Op>
PN2_DEV T row_swap_op(T v, Op op) {  // op of the values of rows r and r ^ (ROWS / 16)
  const uint32_t u = __builtin_bit_cast(uint32_t, v);
  const auto x = ROWS == 16 ? __builtin_amdgcn_permlane16_swap(u, u, false, false)
                            : __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return op(__builtin_bit_cast(T, (uint32_t)x[0]), __builtin_bit_cast(T, (uint32_t)x[1]));
}
template <int SEG, bool OLD_SELF = false, typename T, typename Op>
PN2_DEV T dpp_reduce(T v, Op op) {
  static_assert(sizeof(T) == 4 && SEG >= 4 && SEG <= kWave && (SEG & (SEG - 1)) == 0, "");
  v = op(v, dpp_get<kDppXor1, OLD_SELF>(v));
  v = op(v, dpp_get<kDppXor2, OLD_SELF>(v));
  if constexpr (SEG >= 8) v = op(v, dpp_get<kDppHalfMirror, OLD_SELF>(v));
  if constexpr (SEG >= 16) v = op(v, dpp_get<kDppMirror, OLD_SELF>(v));
  if constexpr (SEG >= 32) v = row_swap_op<16>(v, op);
  if constexpr (SEG >= 64) v = row_swap_op<32>(v, op);
  return v;
}

template <int SEG>
PN2_DEV uint32_t seg_max_u32(uint32_t v) {
  return dpp_reduce<SEG>(v, [](uint32_t a, uint32_t b) { return a > b ? a : b; });
}
PN2_DEV uint32_t row16_max_u32(uint32_t v) { return seg_max_u32<16>(v); }
PN2_DEV uint32_t wave_max_u32(uint32_t v) { return seg_max_u32<kWave>(v); }
PN2_DEV int wave_max_i32(int v) {
  return dpp_reduce<kWave>(v, [](int a, int b) { return max(a, b); });
}
PN2_DEV float wave_min_f(float v) {
  return dpp_reduce<kWave, true>(v, [](float a, float b) { return fminf(a, b); });
}
PN2_DEV float wave_max_f(float v) {
  return dpp_reduce<kWave, true>(v, [](float a, float b) { return fmaxf(a, b); });
}
// float sum / max over aligned segments of SEG lanes (the attention reductions)
template <int SEG, bool MAX>
PN2_DEV float seg_reduce(float v) {
  return dpp_reduce<SEG>(v, [](float a, float b) { return MAX ? fmaxf(a, b) : a + b; });
}

PN2_DEV uint64_t pack64(uint32_t lo, uint32_t hi) { return ((uint64_t)hi << 32) | lo; }

// The 64-bit max: the same pattern on two dwords per exchange, the DPP moves without an old
// value (dpp_u32; also the quad exchanges of interp.hip's three_nn merge). Written out, not
// through dpp_reduce: with either old value the samplers, knn_select_kernel and xent_fwd_wave
// come out with other instructions.
template <int CTRL>
PN2_DEV uint32_t dpp_u32(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xF, 0xF, false);
}
template <int CTRL>
PN2_DEV uint64_t max_dpp_u64(uint64_t v) {
  const uint32_t lo = dpp_u32<CTRL>((uint32_t)v);
  const uint32_t hi = dpp_u32<CTRL>((uint32_t)(v >> 32));
  const uint64_t o = pack64(lo, hi);
  return o > v ? o : v;
}

// max over the 16 lanes of each DPP row (all 16 lanes get the row max)
PN2_DEV uint64_t row16_max_u64(uint64_t v) {
  v = max_dpp_u64<kDppXor1>(v);
  v = max_dpp_u64<kDppXor2>(v);
  v = max_dpp_u64<kDppHalfMirror>(v);
  v = max_dpp_u64<kDppMirror>(v);
  return v;
}

PN2_DEV uint64_t wave_max_u64(uint64_t v) {
  v = row16_max_u64(v);
  {
    uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
    auto l = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    auto h = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    const uint64_t a = pack64(l[0], h[0]), b = pack64(l[1], h[1]);
    v = a > b ? a : b;
  }
  {
    uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
    auto l = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
    auto h = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
    const uint64_t a = pack64(l[0], h[0]), b = pack64(l[1], h[1]);
    v = a > b ? a : b;
  }
  return v;
}

// inclusive prefix sum over the wave: DPP row shifts (1, 2, 4, 8 within each 16-lane row; a
// lane without a source adds 0), then row_bcast:15 / :31 carry each row's total into the rows
// above -- six VALU steps, where the __shfl_up form was six dependent LDS-crossbar round trips
// (every lane of the wave active; SA1's grid query 22.0 -> 21.0 us, tools/bench_side.py)
PN2_DEV int wave_incl_scan(int v, int lane) {
  (void)lane;
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, false);  // row_shr:1
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, false);  // row_shr:2
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, false);  // row_shr:4
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, false);  // row_shr:8
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false);  // row_bcast:15, rows 1, 3
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false);  // row_bcast:31, rows 2, 3
  return v;
}

PN2_DEV uint32_t uniform_u32(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
PN2_DEV uint64_t uniform_u64(uint64_t v) {
  return pack64(uniform_u32((uint32_t)v), uniform_u32((uint32_t)(v >> 32)));
}

PN2_DEV int lane_id() { return (int)__lane_id(); }

// ---- bf16 matrix-core operands -----------------------------------------------------------
typedef float f32x16 __attribute__((ext_vector_type(16)));   // a 32x32 MFMA accumulator
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));   // a v_mfma_f32_32x32x16_bf16 operand
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));  // the same 16 bytes as dwords

// Two fp32 to one packed bf16 pair (lo in bits 0..15), round to nearest even; no builtin.
PN2_DEV uint32_t cvt_pk_bf16(float lo, float hi) {
  uint32_t r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}
// eight fp32 to one bf16 MFMA operand (element j in bits 16 j ..), round to nearest even
PN2_DEV bf16x8 pack_bf16x8(const float (&v)[8]) {
  u32x4 p;
  p.x = cvt_pk_bf16(v[0], v[1]);
  p.y = cvt_pk_bf16(v[2], v[3]);
  p.z = cvt_pk_bf16(v[4], v[5]);
  p.w = cvt_pk_bf16(v[6], v[7]);
  return __builtin_bit_cast(bf16x8, p);
}
// one fp32 to bf16 in plain integer code, round to nearest even (cvt_pk_bf16's rounding)
PN2_DEV uint16_t bf16_rne(float v) {
  uint32_t u = __float_as_uint(v);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);  // NaN stays NaN
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

// ---- arithmetic that several kernels must round alike ---------------------------------------
// One definition each: the paths that the project promises agree bit for bit (pn2_fp_apply and
// the fused FP MLP; attn.hip, attn_train.hip and the fused attention tail) call the same code.

// three_interpolate's weights: (1/d)/sum(1/d), d = max(dist, 1e-10)  (pointnet_util.py:219-222)
PN2_DEV void idw(float d1, float d2, float d3, float& w1, float& w2, float& w3) {
  const float r1 = 1.0f / fmaxf(d1, 1e-10f);
  const float r2 = 1.0f / fmaxf(d2, 1e-10f);
  const float r3 = 1.0f / fmaxf(d3, 1e-10f);
  const float norm = (r1 + r2) + r3;
  w1 = r1 / norm;
  w2 = r2 / norm;
  w3 = r3 / norm;
}

PN2_DEV float dot4(float4 q, float4 k) {  // (1x4)·(4x1) of tf.matmul, summed left to right
  float s = q.x * k.x;
  s = s + q.y * k.y;
  s = s + q.z * k.z;
  s = s + q.w * k.w;
  return s;
}

// Sum / max over aligned segments of SEG lanes (SEG a power of two <= 64) using xor shuffles.
template <int SEG>
PN2_DEV float seg_sum(float v) {
#pragma unroll
  for (int o = SEG / 2; o > 0; o >>= 1) v = __fadd_rn(v, __shfl_xor(v, o, kWave));
  return v;
}
template <int SEG>
PN2_DEV float seg_max(float v) {
#pragma unroll
  for (int o = SEG / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, kWave));
  return v;
}

// Every pointer on a 16-byte boundary (null counts as aligned): what the float4 / 16-byte
// paths need of their bases.
template <typename... P>
__host__ __device__ inline bool aligned16(const P*... p) {
  return (((uintptr_t)p | ...) & 15) == 0;
}

// XCD-aware block order (MI355X_MICROARCH.md, workgroup dispatch): linear blocks are dealt
// round-robin over the 8 XCDs (blocks L and L + 8 share one XCD and its L2). Launching
// xcd_grid(n) blocks and working on logical block xcd_block(L, n) gives every XCD one
// contiguous range of logical blocks, so the blocks of one cloud share an L2 instead of each
// XCD fetching the cloud's rows. Speed only: any placement gives the same results. Logical
// blocks >= n (the padding) must return before any barrier.
constexpr int kXcds = 8;
inline unsigned xcd_grid(long long n) { return (unsigned)((n + kXcds - 1) / kXcds * kXcds); }
PN2_DEV int xcd_block(int L, int n) {
  const int per = (n + kXcds - 1) / kXcds;
  return (L % kXcds) * per + L / kXcds;
}

// Integer division by a runtime divisor via a precomputed 32-bit magic (exact when
// numerator * divisor < 2^32; the launcher checks that bound).
struct FastDiv {
  uint32_t d, magic;
};
inline FastDiv make_fastdiv(uint32_t d) {
  FastDiv f;
  f.d = d;
  f.magic = d <= 1 ? 0u : (uint32_t)((((uint64_t)1 << 32) + d - 1) / d);
  return f;
}
PN2_DEV uint32_t fdiv(uint32_t n, FastDiv f) { return f.d == 1 ? n : __umulhi(n, f.magic); }

// pn2_fps_chain's argument check (fps.hip), shared with the plan executor (plan.hip)
int fps_chain_check(const float* xyz, int B, int N, int nstages, const int* npoint,
                    int32_t* const* idx, float* const* new_xyz);
// pn2_fps_chain without the stored-fault report (the plan executor takes the fault word once,
// before it enqueues anything, so a plan never stops part-way through a step)
int fps_chain_launch(const float* xyz, int B, int N, int nstages, const int* npoint,
                     int32_t* const* idx, float* const* new_xyz, hipStream_t s, bool take,
                     void* grid0 = nullptr, size_t grid0_bytes = 0);
// a fault stored by an earlier sampler launch, cleared (0: none)
int fps_take_fault();

}  // namespace pn2

// launch-status helper for the C ABI
#define PN2_RETURN_LAUNCH()                         \
  do {                                              \
    hipError_t e__ = hipGetLastError();             \
    return e__ == hipSuccess ? PN2_OK : (int)e__;   \
  } while (0)
