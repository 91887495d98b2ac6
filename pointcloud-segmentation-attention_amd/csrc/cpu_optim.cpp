// pn2cpu_adam_step, pn2cpu_seg_confusion, pn2cpu_mean_iou: the host twins of optim.hip in plain
// C++. The GPU results are compared against them bit for bit: Adam is seven fp32 operations per
// element, each rounded on its own (built with -ffp-contract=off; sqrtf and / are correctly
// rounded, denormals are kept); the confusion matrix is integers; the mean IoU is the same
// double-precision sum in class order.
#include <cmath>

#include "../../include/pn2hip.h"

extern "C" int pn2cpu_adam_step(const pn2_adam_slot* slots, int nslots, float alpha, float beta1,
                                float beta2, float epsilon) {
  if (nslots < 0 || (nslots > 0 && !slots)) return PN2_EINVAL;
  if (!(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f)) return PN2_EINVAL;
  if (!(epsilon >= 0.f) || !std::isfinite(alpha)) return PN2_EINVAL;
  for (int i = 0; i < nslots; ++i) {
    const pn2_adam_slot& s = slots[i];
    if (s.n < 0 || s.n > PN2_ADAM_MAX_N) return PN2_EINVAL;
    if (s.n > 0 && (!s.p || !s.g || !s.m || !s.v)) return PN2_EINVAL;
  }
  const float omb1 = 1.0f - beta1, omb2 = 1.0f - beta2;
  for (int i = 0; i < nslots; ++i) {
    const pn2_adam_slot& s = slots[i];
    for (long long e = 0; e < s.n; ++e) {
      const float g = s.g[e];
      const float m = s.m[e] + (g - s.m[e]) * omb1;
      const float v = s.v[e] + (g * g - s.v[e]) * omb2;
      s.m[e] = m;
      s.v[e] = v;
      s.p[e] = s.p[e] - (alpha * m) / (sqrtf(v) + epsilon);
    }
  }
  return PN2_OK;
}

extern "C" int pn2cpu_seg_confusion(const int32_t* labels, const int32_t* pred, long long rows,
                                    int C, long long* confusion, long long* counts) {
  if (C <= 0 || C > PN2_METRICS_MAX_C || rows < 0) return PN2_EINVAL;
  if (rows == 0) return PN2_OK;
  if (!labels || !pred || !confusion || !counts) return PN2_EINVAL;
  for (long long r = 0; r < rows; ++r) {
    const int32_t l = labels[r], q = pred[r];
    if (l > 0 && l < C && q >= 0 && q < C) {
      confusion[(long long)l * C + q] += 1;
      counts[1] += 1;
      counts[0] += q == l;
    }
  }
  return PN2_OK;
}

extern "C" int pn2cpu_mean_iou(const long long* confusion, int C, float* iou, float* per_class) {
  if (C <= 0 || C > PN2_METRICS_MAX_C || !confusion || !iou) return PN2_EINVAL;
  double sum = 0.0;
  int n = 0;
  for (int c = 0; c < C; ++c) {
    long long row = 0, col = 0;
    for (int k = 0; k < C; ++k) {
      row += confusion[c * C + k];
      col += confusion[k * C + c];
    }
    const long long tp = confusion[c * C + c], den = row + col - tp;
    const double v = den != 0 ? (double)tp / (double)den : 0.0;
    if (den != 0) {
      sum += v;
      ++n;
    }
    if (per_class) per_class[c] = (float)v;
  }
  *iou = n ? (float)(sum / (double)n) : 0.f;
  return PN2_OK;
}
