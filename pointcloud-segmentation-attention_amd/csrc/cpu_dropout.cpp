// pn2cpu_dropout: the host twin of pn2_dropout (head_train.hip), the same function of
// (seed, element) in plain C++ (philox.h). The GPU result is compared against it bit for bit:
// the mask is integer arithmetic, the scaling one correctly rounded fp32 division.
#include "../../include/pn2hip.h"
#include "philox.h"

extern "C" int pn2cpu_dropout(const float* x, long long n, float keep_prob, uint64_t seed,
                              float* out) {
  if (n < 0 || !(keep_prob > 0.f && keep_prob <= 1.f)) return PN2_EINVAL;
  if (n == 0) return PN2_OK;
  if (!x || !out) return PN2_EINVAL;
  const uint64_t thr = pn2::dropout_threshold(keep_prob);
  const uint64_t un = (uint64_t)n;
  for (uint64_t q = 0; 4 * q < un; ++q) {
    const pn2::Philox4 r = pn2::dropout_words(seed, q);
    for (int j = 0; j < 4 && 4 * q + j < un; ++j) {
      const uint64_t e = 4 * q + j;
      out[e] = (uint64_t)r.w[j] < thr ? x[e] / keep_prob : 0.f;
    }
  }
  return PN2_OK;
}
