// The reference's ball renderer, headless and on the device (pointnet2_tensorflow/utils/
// render_balls_so.cpp render_ball, show3d_balls.py:51-86), gfx950. Host twins: cpu_render.cpp;
// the arithmetic both share: render_math.h.
//
// render_ball is one serial loop over points x disk entries in which a pixel keeps the first
// point that reaches the greatest depth (`depth[pixel] < z2`). Restated without an order, as
// pn2_scene_vote restates map_back: every pixel holds the 64-bit key
//     ((z2 + 2^31) << 32) | (0xFFFFFFFF - i)
// and every (point, disk entry) pair applies an unsigned 64-bit atomic max: the greatest z2 wins
// and among equal z2 the lowest point index, which is the serial loop's answer. An integer max
// commutes, so the keys, and the image, are the same bits in every run. No float atomics.
//
//   render_splat_kernel    grid (blocks, F). First every thread folds the z of its share of the
//                          frame's points into the frame's depth range: a wave reduction, then
//                          one 64-bit atomic max per wave for each end. Then a wave takes one point
//                          at a time and its lanes the disk's bounding box clipped to the image,
//                          row by row: consecutive lanes are consecutive columns of a row, so a
//                          wave's key reads and atomics fall on a few contiguous runs of 8-byte
//                          keys. The depth offset of an entry is an integer square root. A lane
//                          reads the key first and skips the atomic when the stored key is
//                          already >= its own: keys only grow and an aligned 8-byte load is not
//                          torn, so the skip never loses a winner (PN2_RENDER_SKIP=0 builds the
//                          plain form, one atomic per entry, for tools/bench_render.py). r = 1 is
//                          one entry per point: a thread per point.
//   render_resolve_kernel  a thread per pixel: key -> (z2, i), the entry (dx, dy) from the
//                          winner's coordinates, shade = float(sqrt(double(m)) / r), the frame's
//                          intensity, the colours (three channels, or labels through a palette,
//                          looked up here once per pixel), three bytes. An empty key gives the
//                          background.
//   render_project_kernel  a thread per (frame, point): the viewer's xyz.dot(rotmat) + offset,
//                          astype('int32').
#include "common.h"
#include "render_math.h"

#ifndef PN2_RENDER_SKIP
#define PN2_RENDER_SKIP 1
#endif

namespace pn2 {
namespace {

using namespace render;

constexpr int kSplatThreads = 256;
constexpr int kSplatWaves = kSplatThreads / kWave;
constexpr int kSplatMaxBlocks = 2048;  // per frame; points past them are grid-strided
constexpr int kBlock = 256;            // resolve and project
constexpr int kMaxBlocks = 4096;

// the frame's depth range as two keys under a 64-bit max, 0 = no point yet:
//   zr[0] = max(e(z)) + 1,  zr[1] = max(2^32 - e(z)),  e(z) = z + 2^31 in [0, 2^32)
PN2_DEV uint64_t zr_hi(int32_t z) { return (uint64_t)((long long)z + 2147483648LL) + 1u; }
PN2_DEV uint64_t zr_lo(int32_t z) { return 4294967296ULL - (uint64_t)((long long)z + 2147483648LL); }
PN2_DEV long long zr_max(uint64_t k) { return (long long)(k - 1u) - 2147483648LL; }
PN2_DEV long long zr_min(uint64_t k) { return (long long)(4294967296ULL - k) - 2147483648LL; }

PN2_DEV void vote(unsigned long long* slot, uint64_t key) {
#if PN2_RENDER_SKIP
  if (*reinterpret_cast<const volatile unsigned long long*>(slot) >= key) return;
#endif
  atomicMax(slot, (unsigned long long)key);
}

__global__ __launch_bounds__(kSplatThreads) void render_splat_kernel(
    const int32_t* __restrict__ ixyz, int n, int r, int h, int w,
    unsigned long long* __restrict__ keys, unsigned long long* __restrict__ zrange) {
  const int f = blockIdx.y;
  const int32_t* __restrict__ P = ixyz + (long long)f * n * 3;
  unsigned long long* K = keys + (long long)f * h * w;
  const int lane = threadIdx.x & (kWave - 1);
  const long long gthreads = (long long)gridDim.x * kSplatThreads;
  const long long gtid = (long long)blockIdx.x * kSplatThreads + threadIdx.x;

  uint64_t hi = 0, lo = 0;
  for (long long i = gtid; i < n; i += gthreads) {
    const int32_t z = P[i * 3 + 2];
    const uint64_t a = zr_hi(z), b = zr_lo(z);
    hi = a > hi ? a : hi;
    lo = b > lo ? b : lo;
  }
  hi = wave_max_u64(hi);
  lo = wave_max_u64(lo);
  if (lane == 0 && hi != 0) {
    atomicMax(&zrange[2 * f], (unsigned long long)hi);
    atomicMax(&zrange[2 * f + 1], (unsigned long long)lo);
  }

  if (r == 1) {  // the disk is its centre: dz = 1, one entry per point
    for (long long i = gtid; i < n; i += gthreads) {
      const int x = P[i * 3], y = P[i * 3 + 1];
      const long long z2 = (long long)P[i * 3 + 2] + 1;
      if (x >= 0 && x < h && y >= 0 && y < w && draws(z2))
        vote(&K[(long long)x * w + y], key_of(z2, (uint32_t)i));
    }
    return;
  }

  const int rr = r * r;
  const long long gwaves = (long long)gridDim.x * kSplatWaves;
  for (long long i = (long long)blockIdx.x * kSplatWaves + threadIdx.x / kWave; i < n;
       i += gwaves) {
    const int x = (int)uniform_u32((uint32_t)P[i * 3]), y = (int)uniform_u32((uint32_t)P[i * 3 + 1]);
    const int z = (int)uniform_u32((uint32_t)P[i * 3 + 2]);
    // the disk's rows and columns that lie in the image (64-bit: x, y are any int32)
    const long long xa = x - (long long)(r - 1) > 0 ? x - (long long)(r - 1) : 0;
    const long long xb = x + (long long)(r - 1) < h - 1 ? x + (long long)(r - 1) : h - 1;
    const long long ya = y - (long long)(r - 1) > 0 ? y - (long long)(r - 1) : 0;
    const long long yb = y + (long long)(r - 1) < w - 1 ? y + (long long)(r - 1) : w - 1;
    if (xa > xb || ya > yb) continue;  // wholly outside
    const unsigned bw = (unsigned)(yb - ya + 1);
    const unsigned cnt = (unsigned)(xb - xa + 1) * bw;  // <= h * w < 2^31
    // entry e = lane + 64 k of the box: row e / bw, column e % bw, stepped without a division
    // per entry
    const unsigned q = kWave / bw, rm = kWave - q * bw;
    unsigned row = (unsigned)lane / bw, col = (unsigned)lane - row * bw;
    for (unsigned e = lane; e < cnt; e += kWave, row += q, col += rm) {
      if (col >= bw) {
        col -= bw;
        ++row;
      }
      const int x2 = (int)xa + (int)row, y2 = (int)ya + (int)col;
      const int dx = x2 - x, dy = y2 - y;  // |dx|, |dy| < r
      const int m = rr - dx * dx - dy * dy;
      if (m <= 0) continue;
      const long long z2 = (long long)z + isqrt(m);
      if (draws(z2)) vote(&K[(long long)x2 * w + y2], key_of(z2, (uint32_t)i));
    }
  }
}

__global__ __launch_bounds__(kBlock) void render_resolve_kernel(
    const int32_t* __restrict__ ixyz, int n, const float* __restrict__ c0,
    const float* __restrict__ c1, const float* __restrict__ c2,
    const int32_t* __restrict__ labels, const float* __restrict__ palette, int npal, int r, int h,
    int w, int F, uint32_t bg, const unsigned long long* __restrict__ keys,
    const unsigned long long* __restrict__ zrange, uint8_t* __restrict__ images) {
  const long long hw = (long long)h * w, total = hw * F;
  for (long long p = (long long)blockIdx.x * kBlock + threadIdx.x; p < total;
       p += (long long)gridDim.x * kBlock) {
    const unsigned long long key = keys[p];
    uint8_t px[3] = {(uint8_t)bg, (uint8_t)(bg >> 8), (uint8_t)(bg >> 16)};
    if (key != 0) {
      const long long f = p / hw, q = p - f * hw;
      const int x2 = (int)(q / w), y2 = (int)(q - (long long)x2 * w);
      const uint32_t i = key_point(key);
      const int32_t* pt = ixyz + ((long long)f * n + i) * 3;
      const int dx = x2 - pt[0], dy = y2 - pt[1];
      const double zmin = (double)(zr_min(zrange[2 * f + 1]) - r);
      const double zmax = (double)(zr_max(zrange[2 * f]) + r);
      float a, b, c;
      if (labels) {
        const int32_t l = labels[i];
        const float* row = palette + 3 * (l >= 0 && l < npal ? l : 0);
        a = row[0], b = row[1], c = row[2];
      } else {
        a = c0[i], b = c1[i], c = c2[i];
      }
      shade_pixel(r * r - dx * dx - dy * dy, r, key_z2(key), zmin, zmax, a, b, c, px);
    }
    images[p * 3] = px[0];
    images[p * 3 + 1] = px[1];
    images[p * 3 + 2] = px[2];
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void render_project_kernel(const T* __restrict__ xyz, int n,
                                                                const double* __restrict__ mats,
                                                                int F, int32_t* __restrict__ ixyz) {
  const long long total = (long long)F * n;
  for (long long e = (long long)blockIdx.x * kBlock + threadIdx.x; e < total;
       e += (long long)gridDim.x * kBlock) {
    const long long f = e / n, i = e - f * n;
    const double x = (double)xyz[i * 3], y = (double)xyz[i * 3 + 1], z = (double)xyz[i * 3 + 2];
    const double* mat = mats + f * 12;
    ixyz[e * 3] = project(x, y, z, mat, 0);
    ixyz[e * 3 + 1] = project(x, y, z, mat, 1);
    ixyz[e * 3 + 2] = project(x, y, z, mat, 2);
  }
}

unsigned blocks_for(long long n, int per_block, int cap) {
  long long b = (n + per_block - 1) / per_block;
  return (unsigned)(b > cap ? cap : (b < 1 ? 1 : b));
}

}  // namespace
}  // namespace pn2

extern "C" {

size_t pn2_render_ball_workspace_size(int F, int h, int w) {
  if (F <= 0 || h <= 0 || w <= 0) return 0;
  return ((size_t)F * (size_t)h * (size_t)w + 2 * (size_t)F) * sizeof(unsigned long long);
}

int pn2_render_ball(const int32_t* ixyz, int F, long long n, const float* c0, const float* c1,
                    const float* c2, const int32_t* labels, const float* palette, int npal, int r,
                    int h, int w, int bg0, int bg1, int bg2, uint8_t* images, void* workspace,
                    size_t workspace_bytes, pn2_stream_t stream) {
  using namespace pn2;
  if (F < 0 || n < 0 || n >= (1LL << 31) || h < 0 || w < 0 || r > kMaxRadius) return PN2_EINVAL;
  if ((long long)h * w >= (1LL << 31) || F > 65535) return PN2_EINVAL;
  if ((bg0 | bg1 | bg2) < 0 || bg0 > 255 || bg1 > 255 || bg2 > 255) return PN2_EINVAL;
  if (F == 0 || h == 0 || w == 0) return PN2_OK;
  if (!images) return PN2_EINVAL;
  if (n > 0) {
    if (!ixyz) return PN2_EINVAL;
    if (labels ? (!palette || npal < 1) : (!c0 || !c1 || !c2)) return PN2_EINVAL;
  }
  const size_t need = pn2_render_ball_workspace_size(F, h, w);
  if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 7)) return PN2_EINVAL;
  r = clamp_radius(r);
  hipStream_t s = (hipStream_t)stream;
  unsigned long long* keys = static_cast<unsigned long long*>(workspace);
  unsigned long long* zrange = keys + (size_t)F * h * w;
  hipError_t e = hipMemsetAsync(workspace, 0, need, s);
  if (e != hipSuccess) return (int)e;
  if (n > 0) {
    const unsigned per = r == 1 ? kSplatThreads : kSplatWaves;
    hipLaunchKernelGGL(render_splat_kernel, dim3(blocks_for(n, per, kSplatMaxBlocks), F),
                       dim3(kSplatThreads), 0, s, ixyz, (int)n, r, h, w, keys, zrange);
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  const uint32_t bg = (uint32_t)bg0 | ((uint32_t)bg1 << 8) | ((uint32_t)bg2 << 16);
  hipLaunchKernelGGL(render_resolve_kernel, dim3(blocks_for((long long)F * h * w, kBlock, kMaxBlocks)),
                     dim3(kBlock), 0, s, ixyz, (int)n, c0, c1, c2, labels, palette, npal, r, h, w,
                     F, bg, keys, zrange, images);
  PN2_RETURN_LAUNCH();
}

int pn2_render_project(const void* xyz, int is_f64, long long n, const double* mats, int F,
                       int32_t* ixyz, pn2_stream_t stream) {
  using namespace pn2;
  if (F < 0 || n < 0 || n >= (1LL << 31)) return PN2_EINVAL;
  if (F == 0 || n == 0) return PN2_OK;
  if (!xyz || !mats || !ixyz) return PN2_EINVAL;
  if (((uintptr_t)mats & 7) || (is_f64 && ((uintptr_t)xyz & 7))) return PN2_EINVAL;
  const dim3 grid(blocks_for((long long)F * n, kBlock, kMaxBlocks)), block(kBlock);
  if (is_f64)
    hipLaunchKernelGGL(render_project_kernel<double>, grid, block, 0, (hipStream_t)stream,
                       static_cast<const double*>(xyz), (int)n, mats, F, ixyz);
  else
    hipLaunchKernelGGL(render_project_kernel<float>, grid, block, 0, (hipStream_t)stream,
                       static_cast<const float*>(xyz), (int)n, mats, F, ixyz);
  PN2_RETURN_LAUNCH();
}

}  // extern "C"
