// pn2cpu_scene_vote, pn2cpu_scene_labels, pn2cpu_map_back_rows, pn2cpu_label_lut: the host twins
// of predict.hip in plain C++. Everything is integers and copied bytes, so the GPU results equal
// these bit for bit; the vote runs its rows in order with the same max, which is the GPU's
// atomic max in one of its possible orders.
#include <cstring>

#include "../../include/pn2hip.h"

namespace {
constexpr int kMaxC = 1 << PN2_VOTE_LABEL_BITS;
constexpr long long kMaxRows = 1LL << 55;
constexpr long long kMaxScene = 1LL << 31;

inline int32_t lut_of(int32_t v, const int32_t* lut, int nlut, int32_t dflt) {
  return v >= 0 && v < nlut ? lut[v] : dflt;
}
}  // namespace

extern "C" int pn2cpu_scene_vote(const float* logits, long long rows, int C, const uint8_t* mask,
                                 const int32_t* orig, long long row0, long long n_scene,
                                 long long* keys, int32_t* pred_rows) {
  if (logits && (C < 1 || C > kMaxC)) return PN2_EINVAL;
  if (rows < 0 || row0 < 0 || n_scene < 0 || n_scene >= kMaxScene) return PN2_EINVAL;
  if (rows >= kMaxRows || row0 >= kMaxRows - rows) return PN2_EINVAL;
  if (rows == 0) return PN2_OK;
  if (!mask || !orig || (n_scene > 0 && !keys)) return PN2_EINVAL;
  unsigned long long* k = reinterpret_cast<unsigned long long*>(keys);
  for (long long r = 0; r < rows; ++r) {
    int label = 0;
    if (logits) {
      const float* x = logits + r * C;
      float best = x[0];
      for (int c = 1; c < C; ++c)
        if (x[c] > best) {
          best = x[c];
          label = c;
        }
    }
    if (pred_rows) pred_rows[r] = label;
    const int32_t p = orig[r];
    if (mask[r] != 0 && p >= 0 && p < n_scene) {
      const unsigned long long key =
          ((unsigned long long)(row0 + r + 1) << PN2_VOTE_LABEL_BITS) | (unsigned)label;
      if (key > k[p]) k[p] = key;
    }
  }
  return PN2_OK;
}

extern "C" int pn2cpu_scene_labels(const long long* keys, long long n_scene, const int32_t* lut,
                                   int nlut, int32_t dflt, int32_t* labels, int32_t* mapped,
                                   long long* winner) {
  if (n_scene < 0 || n_scene >= kMaxScene || nlut < 0) return PN2_EINVAL;
  if (mapped && !lut) return PN2_EINVAL;
  if (n_scene == 0) return PN2_OK;
  if (!keys) return PN2_EINVAL;
  for (long long p = 0; p < n_scene; ++p) {
    const unsigned long long key = (unsigned long long)keys[p];
    const int32_t l = key ? (int32_t)(key & (kMaxC - 1)) : 0;
    if (labels) labels[p] = l;
    if (winner) winner[p] = key ? (long long)(key >> PN2_VOTE_LABEL_BITS) - 1 : -1;
    if (mapped) mapped[p] = lut_of(l, lut, nlut, dflt);
  }
  return PN2_OK;
}

extern "C" int pn2cpu_map_back_rows(const void* values, int row_bytes, long long row0,
                                    long long rows, const long long* keys, long long n_scene,
                                    void* out) {
  if (row_bytes <= 0 || (row_bytes & 3) || row0 < 0 || rows < 0) return PN2_EINVAL;
  if (n_scene < 0 || n_scene >= kMaxScene) return PN2_EINVAL;
  if (rows >= kMaxRows || row0 >= kMaxRows - rows) return PN2_EINVAL;
  if (n_scene == 0) return PN2_OK;
  if (!keys || !out || (rows > 0 && !values)) return PN2_EINVAL;
  const unsigned char* src = static_cast<const unsigned char*>(values);
  unsigned char* dst = static_cast<unsigned char*>(out);
  for (long long p = 0; p < n_scene; ++p) {
    const unsigned long long key = (unsigned long long)keys[p];
    if (key == 0) {
      std::memset(dst + p * row_bytes, 0, (size_t)row_bytes);
      continue;
    }
    const long long w = (long long)(key >> PN2_VOTE_LABEL_BITS) - 1 - row0;
    if (w < 0 || w >= rows) continue;  // another batch's row: left as it is
    std::memcpy(dst + p * row_bytes, src + w * row_bytes, (size_t)row_bytes);
  }
  return PN2_OK;
}

extern "C" int pn2cpu_label_lut(const int32_t* in, long long n, const int32_t* lut, int nlut,
                                int32_t dflt, int32_t* out) {
  if (n < 0 || nlut < 0 || (nlut > 0 && !lut)) return PN2_EINVAL;
  if (n == 0) return PN2_OK;
  if (!in || !out) return PN2_EINVAL;
  for (long long i = 0; i < n; ++i) out[i] = lut_of(in[i], lut, nlut, dflt);
  return PN2_OK;
}
