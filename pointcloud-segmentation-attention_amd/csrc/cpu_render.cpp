// pn2cpu_render_ball, pn2cpu_render_project: the host twins of render.hip in plain C++, on the
// arithmetic of render_math.h. The splat runs the points in order with the same key and the same
// max, which is the GPU's atomic max in one of its possible orders, so the images are equal bit
// for bit.
#include <vector>

#include "../../include/pn2hip.h"
#include "render_math.h"

using namespace pn2::render;

extern "C" int pn2cpu_render_ball(const int32_t* ixyz, int F, long long n, const float* c0,
                                  const float* c1, const float* c2, const int32_t* labels,
                                  const float* palette, int npal, int r, int h, int w, int bg0,
                                  int bg1, int bg2, uint8_t* images) {
  if (F < 0 || n < 0 || n >= (1LL << 31) || h < 0 || w < 0 || r > kMaxRadius) return PN2_EINVAL;
  if ((long long)h * w >= (1LL << 31) || F > 65535) return PN2_EINVAL;
  if ((bg0 | bg1 | bg2) < 0 || bg0 > 255 || bg1 > 255 || bg2 > 255) return PN2_EINVAL;
  if (F == 0 || h == 0 || w == 0) return PN2_OK;
  if (!images) return PN2_EINVAL;
  if (n > 0) {
    if (!ixyz) return PN2_EINVAL;
    if (labels ? (!palette || npal < 1) : (!c0 || !c1 || !c2)) return PN2_EINVAL;
  }
  r = clamp_radius(r);
  const long long hw = (long long)h * w;
  const int rr = r * r;
  std::vector<uint64_t> keys((size_t)hw);
  for (int f = 0; f < F; ++f) {
    const int32_t* P = ixyz + (long long)f * n * 3;
    uint8_t* img = images + (long long)f * hw * 3;
    keys.assign((size_t)hw, 0);
    long long zlo = 0, zhi = 0;
    for (long long i = 0; i < n; ++i) {
      const int x = P[i * 3], y = P[i * 3 + 1], z = P[i * 3 + 2];
      zlo = i == 0 || z < zlo ? z : zlo;
      zhi = i == 0 || z > zhi ? z : zhi;
      const long long xa = x - (long long)(r - 1) > 0 ? x - (long long)(r - 1) : 0;
      const long long xb = x + (long long)(r - 1) < h - 1 ? x + (long long)(r - 1) : h - 1;
      const long long ya = y - (long long)(r - 1) > 0 ? y - (long long)(r - 1) : 0;
      const long long yb = y + (long long)(r - 1) < w - 1 ? y + (long long)(r - 1) : w - 1;
      for (long long x2 = xa; x2 <= xb; ++x2)
        for (long long y2 = ya; y2 <= yb; ++y2) {
          const int dx = (int)(x2 - x), dy = (int)(y2 - y);
          const int m = rr - dx * dx - dy * dy;
          if (m <= 0) continue;
          const long long z2 = (long long)z + isqrt(m);
          if (!draws(z2)) continue;
          const uint64_t key = key_of(z2, (uint32_t)i);
          uint64_t& slot = keys[(size_t)(x2 * w + y2)];
          if (key > slot) slot = key;
        }
    }
    const double zmin = (double)(zlo - r), zmax = (double)(zhi + r);
    for (long long p = 0; p < hw; ++p) {
      uint8_t* px = img + p * 3;
      const uint64_t key = keys[(size_t)p];
      if (key == 0) {
        px[0] = (uint8_t)bg0, px[1] = (uint8_t)bg1, px[2] = (uint8_t)bg2;
        continue;
      }
      const uint32_t i = key_point(key);
      const int dx = (int)(p / w) - P[(long long)i * 3], dy = (int)(p % w) - P[(long long)i * 3 + 1];
      float a, b, c;
      if (labels) {
        const int32_t l = labels[i];
        const float* row = palette + 3 * (l >= 0 && l < npal ? l : 0);
        a = row[0], b = row[1], c = row[2];
      } else {
        a = c0[i], b = c1[i], c = c2[i];
      }
      shade_pixel(rr - dx * dx - dy * dy, r, key_z2(key), zmin, zmax, a, b, c, px);
    }
  }
  return PN2_OK;
}

extern "C" int pn2cpu_render_project(const void* xyz, int is_f64, long long n, const double* mats,
                                     int F, int32_t* ixyz) {
  if (F < 0 || n < 0 || n >= (1LL << 31)) return PN2_EINVAL;
  if (F == 0 || n == 0) return PN2_OK;
  if (!xyz || !mats || !ixyz) return PN2_EINVAL;
  const float* x32 = static_cast<const float*>(xyz);
  const double* x64 = static_cast<const double*>(xyz);
  for (int f = 0; f < F; ++f)
    for (long long i = 0; i < n; ++i) {
      const double x = is_f64 ? x64[i * 3] : (double)x32[i * 3];
      const double y = is_f64 ? x64[i * 3 + 1] : (double)x32[i * 3 + 1];
      const double z = is_f64 ? x64[i * 3 + 2] : (double)x32[i * 3 + 2];
      int32_t* o = ixyz + ((long long)f * n + i) * 3;
      for (int k = 0; k < 3; ++k) o[k] = project(x, y, z, mats + (long long)f * 12, k);
    }
  return PN2_OK;
}
