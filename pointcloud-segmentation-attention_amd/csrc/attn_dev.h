// Device functions shared by the attention reductions: attn.hip (K and V in tensors of their
// own) and attn_train.hip (training: K and V interleaved in one row). One definition of the
// streamed load, the score product and the segment reductions, so both files round identically.
#pragma once

#include "common.h"

namespace pn2 {
namespace {

// K / V are streamed once: non-temporal loads (no reuse in the caches)
PN2_DEV float4 ld_stream(const float* p) {
  using v4 = float __attribute__((ext_vector_type(4)));
  const v4 r = __builtin_nontemporal_load(reinterpret_cast<const v4*>(p));
  return make_float4(r.x, r.y, r.z, r.w);
}

PN2_DEV float dot4(float4 q, float4 k) {  // (1x4)·(4x1) of tf.matmul, summed left to right
  float s = q.x * k.x;
  s = s + q.y * k.y;
  s = s + q.z * k.z;
  s = s + q.w * k.w;
  return s;
}

// Segment reductions over LPH = 8..64 lanes with DPP / permlane exchanges (no LDS crossbar
// round trip per step, unlike ds_bpermute shuffles): quad xor1 / xor2, row_half_mirror,
// row_mirror, then the gfx950 row swaps. Every lane of a segment ends with the same value.
template <int CTRL>
PN2_DEV float dppf(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
template <int SEG, bool MAX>
PN2_DEV float seg_reduce(float v) {
  auto op = [](float a, float b) { return MAX ? fmaxf(a, b) : a + b; };
  v = op(v, dppf<kDppXor1>(v));
  v = op(v, dppf<kDppXor2>(v));
  if constexpr (SEG >= 8) v = op(v, dppf<kDppHalfMirror>(v));
  if constexpr (SEG >= 16) v = op(v, dppf<kDppMirror>(v));
  if constexpr (SEG >= 32) {
    const int u = __float_as_int(v);
    auto x = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    v = op(__int_as_float((int)x[0]), __int_as_float((int)x[1]));
  }
  if constexpr (SEG >= 64) {
    const int u = __float_as_int(v);
    auto x = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    v = op(__int_as_float((int)x[0]), __int_as_float((int)x[1]));
  }
  return v;
}

}  // namespace
}  // namespace pn2
