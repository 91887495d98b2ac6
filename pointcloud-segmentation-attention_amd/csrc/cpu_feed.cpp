// pn2cpu_feed_batch, pn2cpu_val_select, pn2cpu_val_chunks: the host twins of feed.hip and of
// pn2_val_select (scene.hip) in plain C++, compiled without contraction. Every fp32 operation
// is written on its own (two products, then one sum; one division), the box tests are float64
// comparisons and everything else is integers and copied bytes, so the GPU results equal these
// bit for bit. The twins need no workspace and no stream.
#include <cstring>

#include "../../include/pn2hip.h"

namespace {

inline float weight_of(int lab, const float* w, int L) { return lab >= 0 && lab < L ? w[lab] : 0.0f; }

inline void rotate_z(float x, float y, float c, float s, float* ox, float* oy) {
  const float xc = x * c, ys = y * s;
  const float yc = y * c, xs = x * s;
  *ox = xc + ys;
  *oy = yc - xs;
}

inline bool in_box_d(const float* q, const double* bd, double m) {
  bool ok = true;
  for (int c = 0; c < 3; ++c) {
    const double v = (double)q[c];
    ok = ok && (v >= bd[c] - m) && (v <= bd[3 + c] + m);
  }
  return ok;
}

inline int col_n(const int32_t* counts, int s, int N) { return counts[s] < N ? counts[s] : N; }

inline int draw_of(const int32_t* choice, const float* u, size_t at, int n) {
  int k;
  if (choice) {
    k = choice[at];
  } else {
    const float f = u[at] * (float)n;
    // the device's float -> int conversion saturates and gives 0 for NaN
    k = f != f ? 0 : (f >= 2147483648.0f ? 0x7fffffff : (f <= -2147483648.0f ? -0x7fffffff - 1 : (int)f));
  }
  k = k > 0 ? k : 0;
  return k < n - 1 ? k : n - 1;
}

}  // namespace

extern "C" int pn2cpu_feed_batch(const float* points, const int32_t* labels, const int32_t* colors,
                                 const float* normals, const float* sample_weight, const float* cs,
                                 const float* class_weights, int L, int B, int N, int use_color,
                                 int use_normal, float* xyz, float* features, float* smpw) {
  if (B < 0 || N < 0 || L < 0) return PN2_EINVAL;
  const long long rows = (long long)B * N;
  if (rows == 0) return PN2_OK;
  if (!points || !labels || !sample_weight || !xyz || !smpw) return PN2_EINVAL;
  if ((L > 0 && !class_weights) || (use_color && !colors) || (use_normal && !normals))
    return PN2_EINVAL;
  if ((use_color || use_normal) && !features) return PN2_EINVAL;
  const int F = (use_color ? 3 : 0) + (use_normal ? 3 : 0);
  for (long long r = 0; r < rows; ++r) {
    float c = 1.0f, s = 0.0f;
    if (cs) {
      const long long b = r / N;
      c = cs[b * 2];
      s = cs[b * 2 + 1];
    }
    float x = points[r * 3], y = points[r * 3 + 1];
    if (cs) rotate_z(x, y, c, s, &x, &y);
    xyz[r * 3] = x;
    xyz[r * 3 + 1] = y;
    xyz[r * 3 + 2] = points[r * 3 + 2];
    float* f = features + r * F;
    if (use_color) {
      for (int k = 0; k < 3; ++k) f[k] = (float)colors[r * 3 + k] / 255.0f;
      f += 3;
    }
    if (use_normal) {
      float nx = normals[r * 3], ny = normals[r * 3 + 1];
      if (cs) rotate_z(nx, ny, c, s, &nx, &ny);
      f[0] = nx;
      f[1] = ny;
      f[2] = normals[r * 3 + 2];
    }
    const float m = sample_weight[r] != 0.0f ? 1.0f : 0.0f;
    smpw[r] = weight_of(labels[r], class_weights, L) * m;
  }
  return PN2_OK;
}

extern "C" int pn2cpu_val_select(const float* points, int N, const double* bounds, int S,
                                 double margin, double inner_margin, int32_t* counts, int32_t* sel,
                                 uint8_t* inner) {
  if (N < 0 || S < 0) return PN2_EINVAL;
  if ((long long)N * S > 0x7fffffffLL || S > 65535) return PN2_EINVAL;
  if (S == 0) return PN2_OK;
  if (!counts) return PN2_EINVAL;
  if (N == 0) {
    std::memset(counts, 0, (size_t)S * sizeof(int32_t));
    return PN2_OK;
  }
  if (!points || !bounds || !sel || !inner) return PN2_EINVAL;
  for (int s = 0; s < S; ++s) {
    const double* bd = bounds + (size_t)s * 6;
    int n = 0;
    for (int i = 0; i < N; ++i) {
      const float* q = points + (size_t)i * 3;
      if (!in_box_d(q, bd, margin)) continue;
      sel[(size_t)s * N + n] = i;
      inner[(size_t)s * N + n] = in_box_d(q, bd, inner_margin) ? 1 : 0;
      ++n;
    }
    counts[s] = n;
  }
  return PN2_OK;
}

extern "C" int pn2cpu_val_chunks(const float* points, const int32_t* labels, const int32_t* colors,
                                 const float* normals, int N, const int32_t* counts,
                                 const int32_t* sel, const uint8_t* inner, int S,
                                 const int32_t* choice, const float* u, int K,
                                 const float* label_weights, int L, double min_inside,
                                 float* out_points, int32_t* out_labels, int32_t* out_colors,
                                 float* out_normals, float* out_weights, int32_t* column,
                                 int32_t* kept) {
  if (N < 0 || S < 0 || K < 0 || L < 0) return PN2_EINVAL;
  if ((long long)N * S > 0x7fffffffLL || (long long)K * S > 0x7fffffffLL || S > 65535)
    return PN2_EINVAL;
  if (!kept) return PN2_EINVAL;
  if (S == 0) {
    *kept = 0;
    return PN2_OK;
  }
  if (!counts || !column || (L > 0 && !label_weights)) return PN2_EINVAL;
  if (N > 0 && (!points || !labels || !sel || !inner)) return PN2_EINVAL;
  if (K > 0 && ((!choice && !u) || !out_points || !out_labels || !out_weights))
    return PN2_EINVAL;
  if ((colors && !out_colors) || (normals && !out_normals)) return PN2_EINVAL;
  int32_t* oc = colors ? out_colors : nullptr;
  float* on = normals ? out_normals : nullptr;
  int j = 0;
  for (int s = 0; s < S; ++s) {
    const int n = col_n(counts, s, N);
    if (n <= 0) continue;
    int msum = 0;
    for (int r = 0; r < K; ++r)
      msum += inner[(size_t)s * N + draw_of(choice, u, (size_t)s * K + r, n)] ? 1 : 0;
    if ((double)msum / (double)K < min_inside) continue;
    for (int r = 0; r < K; ++r) {
      const size_t o = (size_t)j * K + r;
      const int k = draw_of(choice, u, (size_t)s * K + r, n);
      int i = sel[(size_t)s * N + k];
      i = i > 0 ? i : 0;
      i = i < N - 1 ? i : N - 1;
      for (int c = 0; c < 3; ++c) {
        out_points[o * 3 + c] = points[(size_t)i * 3 + c];
        if (oc) oc[o * 3 + c] = colors[(size_t)i * 3 + c];
        if (on) on[o * 3 + c] = normals[(size_t)i * 3 + c];
      }
      const int lab = labels[i];
      out_labels[o] = lab;
      const float m = inner[(size_t)s * N + k] ? 1.0f : 0.0f;
      out_weights[o] = weight_of(lab, label_weights, L) * m;
    }
    column[j++] = s;
  }
  *kept = j;
  for (int jj = j; jj < S; ++jj) {
    column[jj] = -1;
    const size_t o = (size_t)jj * K;
    if (K > 0) {
      std::memset(out_points + o * 3, 0, (size_t)K * 3 * sizeof(float));
      std::memset(out_labels + o, 0, (size_t)K * sizeof(int32_t));
      std::memset(out_weights + o, 0, (size_t)K * sizeof(float));
      if (oc) std::memset(oc + o * 3, 0, (size_t)K * 3 * sizeof(int32_t));
      if (on) std::memset(on + o * 3, 0, (size_t)K * 3 * sizeof(float));
    }
  }
  return PN2_OK;
}
