// The arithmetic of the ball renderer, once, for render.hip and its host twin cpu_render.cpp
// (pointnet2_tensorflow/utils/render_balls_so.cpp and show3d_balls.py:72-74). Both files are
// compiled with -ffp-contract=off: every double expression below rounds operation by operation,
// as the reference's does under plain g++ -O2.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PN2_HD __host__ __device__ inline
#else
#define PN2_HD inline
#endif

namespace pn2 {
namespace render {

constexpr int kMaxRadius = PN2_RENDER_MAX_RADIUS;
constexpr long long kNoDraw = -2100000000LL;  // the reference's initial depth: z2 must exceed it

PN2_HD int clamp_radius(int r) { return r < 1 ? 1 : r; }

// ---- the pixel key: ((z2 + 2^31) << 32) | (0xFFFFFFFF - i). The greatest z2 wins and, among
// equal z2, the lowest point index: the serial loop's strict `depth < z2`. 0 = nothing drawn
// (a drawn z2 exceeds kNoDraw, so its high word is positive).
PN2_HD bool draws(long long z2) { return z2 > kNoDraw && z2 <= 2147483647LL; }
PN2_HD uint64_t key_of(long long z2, uint32_t i) {
  return ((uint64_t)(z2 + 2147483648LL) << 32) | (uint64_t)(0xFFFFFFFFu - i);
}
PN2_HD long long key_z2(uint64_t key) { return (long long)(key >> 32) - 2147483648LL; }
PN2_HD uint32_t key_point(uint64_t key) { return 0xFFFFFFFFu - (uint32_t)key; }

// ---- a disk entry (dx, dy) with m = r*r - dx*dx - dy*dy > 0: dz = sqrt(double(m)), the depth
// offset int(dz) and the shade float(dz / r). int(dz) is the integer square root: sqrt(m) of a
// non-square m < 2^31 lies at least 2^-17 below the next integer, far more than a double's
// rounding. The splat needs only this, and takes it without double arithmetic.
PN2_HD int isqrt(int m) {  // 0 < m <= kMaxRadius^2 < 2^30: the squares below fit an int
#if defined(__HIP_DEVICE_COMPILE__)
  int s = (int)__builtin_amdgcn_sqrtf((float)m);  // an estimate; the two loops make it exact
#else
  int s = (int)sqrtf((float)m);
#endif
  while (s * s > m) --s;
  while ((s + 1) * (s + 1) <= m) ++s;
  return s;
}
PN2_HD float shade_of(int m, int r) { return (float)(sqrt((double)m) / (double)r); }

// ---- the frame's depth range over all n points: zmin = min(z) - r, zmax = max(z) + r
PN2_HD double intensity_of(long long z2, double zmin, double zmax) {
  const double v = ((double)z2 - zmin) / (zmax - zmin) * 0.7 + 0.3;
  return v < 1.0 ? v : 1.0;  // min(1.0, v)
}

// Colours are expected in [0, 255]; anything else (NaN: 0) is clamped into it, because the
// reference's conversion of a double outside [0, 256) to unsigned char is undefined.
PN2_HD float clamp_colour(float c) { return c >= 0.f ? (c <= 255.f ? c : 255.f) : 0.f; }
// one channel: the float product shade * c, then the double product, then truncation
PN2_HD uint8_t channel(float shade, float c, double intensity) {
  const float sc = shade * c;
  return (uint8_t)(int)((double)sc * intensity);
}
// the pixel (b, g, r) = (c2, c0, c1) of the winning point, the reference's channel order
PN2_HD void shade_pixel(int m, int r, long long z2, double zmin, double zmax, float c0, float c1,
                        float c2, uint8_t* px) {
  const float s = shade_of(m, r);
  const double it = intensity_of(z2, zmin, zmax);
  px[0] = channel(s, clamp_colour(c2), it);
  px[1] = channel(s, clamp_colour(c0), it);
  px[2] = channel(s, clamp_colour(c1), it);
}

// ---- the viewer's projection: (x*R[0][k] + y*R[1][k]) + z*R[2][k] + off[k] in double, left to
// right, truncated as numpy's astype('int32') does (cvttsd2si: out of range or NaN gives
// INT32_MIN). mat: the 3x3 matrix row-major, then the offset.
PN2_HD int32_t trunc_i32(double v) {
  return v > -2147483649.0 && v < 2147483648.0 ? (int32_t)v : INT32_MIN;
}
PN2_HD int32_t project(double x, double y, double z, const double* mat, int k) {
  return trunc_i32((x * mat[k] + y * mat[3 + k]) + z * mat[6 + k] + mat[9 + k]);
}

}  // namespace render
}  // namespace pn2
