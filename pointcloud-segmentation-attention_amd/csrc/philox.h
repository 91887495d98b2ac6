// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3",
// SC'11; the Random123 constants), for host and device code alike: plain integer C++, no HIP
// header. pn2_dropout (head_train.hip) and pn2cpu_dropout (cpu_dropout.cpp) share it, so the
// two masks are the same function of (seed, element).
//
// The dropout convention (include/pn2hip.h): key = (seed & 0xffffffff, seed >> 32), counter =
// (q & 0xffffffff, q >> 32, 0, 0) with q = e / 4; element e takes output word e % 4 and is kept
// iff word < floor(keep_prob * 2^32).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PN2_HD __host__ __device__ inline
#else
#define PN2_HD inline
#endif

namespace pn2 {

struct Philox4 {
  uint32_t w[4];
};

PN2_HD void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
  const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
  const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
  const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
  const uint32_t n1 = (uint32_t)p1;
  const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
  const uint32_t n3 = (uint32_t)p0;
  c[0] = n0;
  c[1] = n1;
  c[2] = n2;
  c[3] = n3;
}

PN2_HD Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                             uint32_t k1) {
  uint32_t c[4] = {c0, c1, c2, c3};
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int r = 0; r < 10; ++r) {
    philox_round(c, k0, k1);
    k0 += 0x9E3779B9u;  // the Weyl key schedule
    k1 += 0xBB67AE85u;
  }
  Philox4 o;
  o.w[0] = c[0];
  o.w[1] = c[1];
  o.w[2] = c[2];
  o.w[3] = c[3];
  return o;
}

// the four words of dropout quad q under `seed`
PN2_HD Philox4 dropout_words(uint64_t seed, uint64_t q) {
  return philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), 0u, 0u, (uint32_t)seed,
                       (uint32_t)(seed >> 32));
}

// floor(keep_prob * 2^32) in double: 2^32 at keep_prob = 1 (every word is below it), 0 for an
// argument outside (0, 1] (the callers reject it: NaN fails both comparisons)
inline uint64_t dropout_threshold(float keep_prob) {
  if (!(keep_prob > 0.f && keep_prob <= 1.f)) return 0;
  return (uint64_t)((double)keep_prob * 4294967296.0);
}

}  // namespace pn2
