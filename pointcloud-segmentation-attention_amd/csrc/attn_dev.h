// Device functions shared by the attention reductions: attn.hip (K and V in tensors of their
// own) and attn_train.hip (training: K and V interleaved in one row). One definition of the
// streamed load here, and of the score product (dot4) and the segment reductions (seg_reduce)
// in common.h, so both files round identically.
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

}  // namespace
}  // namespace pn2
