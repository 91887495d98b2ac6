// Whole-scene prediction (attention_points/benchmark/generate_predictions.py:139-186) and the
// label look-ups of the ScanNet score (benchmark/evaluate.py:58-108), gfx950. Host twins:
// cpu_predict.cpp.
//
// The reference takes the argmax of every chunk's logits on the host, concatenates a scene's
// chunks and runs map_back (:19-37): res = zeros; res[orig[mask]] = values[mask]. numpy writes
// repeated indices in order, so of the masked rows that name one point the LAST one in
// concatenation order wins. Here each scene point holds a 64-bit key
//     ((global_row + 1) << PN2_VOTE_LABEL_BITS) | label
// and every masked row applies an unsigned 64-bit atomic max to its point's key: the largest
// global row wins, which is numpy's order, and an integer max commutes, so the keys are the same
// bits for any launch order and any split of the scene into batches. A scene streams through the
// model batch by batch and its logits never leave the device; no float atomics anywhere.
//
//   pn2_scene_vote     argmax per row (lowest index on ties) and the vote. A workgroup's four
//                      waves each own 64 consecutive rows. A wave stages its rows through LDS in
//                      column tiles of at most kTileC: for C <= kTileC the 64 rows are one
//                      contiguous block of global memory, read with consecutive lanes on
//                      consecutive dwords; for larger C every row contributes one 128-byte
//                      segment per tile. Then lane l scans row l of the tile. The LDS row stride
//                      is the tile width made odd, so the 32 lanes of a half-wave read 32
//                      different banks (ds_read_b32: bank = dword address mod 32) whether C is odd
//                      or even. No lane issues a strided global load stream.
//   pn2_scene_labels   keys -> labels, the winning global row, and a table look-up of the label.
//   pn2_map_back_rows  the generic map_back: out[p] = values[winner(p) - row0], 4 or 16 bytes
//                      per thread as pn2_gather_rows copies them.
//   pn2_label_lut      out = 0 <= in < nlut ? lut[in] : dflt.
#include "common.h"

namespace pn2 {
namespace {

constexpr int kVoteThreads = 256;
constexpr int kVoteWaves = kVoteThreads / kWave;
constexpr int kTileC = 32;                 // columns staged at once
constexpr int kTileStride = kTileC + 1;    // the largest odd row stride
constexpr int kMaxC = 1 << PN2_VOTE_LABEL_BITS;
constexpr int kVoteMaxBlocks = 2048;       // rows past 2048 x 256 are grid-strided
constexpr int kBlock = 256;                // the element-wise kernels
static_assert(kVoteWaves * kWave * kTileStride * 4 <= 64 * 1024, "static LDS of the vote kernel");

__global__ __launch_bounds__(kVoteThreads) void scene_vote_kernel(
    const float* __restrict__ logits, long long rows, int C, const uint8_t* __restrict__ mask,
    const int32_t* __restrict__ orig, long long row0, int n_scene,
    unsigned long long* __restrict__ keys, int32_t* __restrict__ pred_rows) {
  __shared__ float tile[kVoteWaves][kWave * kTileStride];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  float* t = tile[wave];
  const int tc0 = C < kTileC ? C : kTileC;
  const int stride = tc0 | 1;
  const long long per_pass = (long long)gridDim.x * kVoteThreads;
  // every wave of a workgroup runs the same number of passes (the barriers below)
  for (long long base = (long long)blockIdx.x * kVoteThreads; base < rows; base += per_pass) {
    const long long wrow = base + (long long)wave * kWave;  // this wave's first row
    const long long r = wrow + lane;
    int label = 0;
    if (logits) {
      const long long left = rows - wrow;
      const int nr = left >= kWave ? kWave : (left > 0 ? (int)left : 0);  // rows of this wave
      float best = 0.f;
      for (int c0 = 0; c0 < C; c0 += kTileC) {
        const int tc = C - c0 < kTileC ? C - c0 : kTileC;
        // element e = lane + 64 k of the (64, tc) tile: row e / tc, column e % tc, stepped
        // without a division per element
        const int q = kWave / tc, rm = kWave % tc;
        int row = lane / tc, col = lane - row * tc;
        const float* src = logits + wrow * C + c0;
        __syncthreads();  // the previous tile's scans are done
        for (int k = 0; k < tc; ++k) {
          if (row < nr) t[row * stride + col] = src[(long long)row * C + col];
          row += q;
          col += rm;
          if (col >= tc) {
            col -= tc;
            ++row;
          }
        }
        __syncthreads();
        if (lane < nr) {
          const float* mine = t + lane * stride;
          int c = 0;
          if (c0 == 0) {
            best = mine[0];
            c = 1;
          }
          for (; c < tc; ++c) {
            const float v = mine[c];
            if (v > best) {  // strict: the lowest index of a tie stays
              best = v;
              label = c0 + c;
            }
          }
        }
      }
    }
    if (r < rows) {
      if (pred_rows) pred_rows[r] = label;
      const int32_t p = orig[r];
      if (mask[r] != 0 && p >= 0 && p < n_scene) {
        const unsigned long long key =
            ((unsigned long long)(row0 + r + 1) << PN2_VOTE_LABEL_BITS) | (unsigned)label;
        atomicMax(&keys[p], key);
      }
    }
  }
}

PN2_DEV int32_t lut_of(int32_t v, const int32_t* __restrict__ lut, int nlut, int32_t dflt) {
  return v >= 0 && v < nlut ? lut[v] : dflt;
}

__global__ __launch_bounds__(kBlock) void scene_labels_kernel(
    const unsigned long long* __restrict__ keys, int n_scene, const int32_t* __restrict__ lut,
    int nlut, int32_t dflt, int32_t* __restrict__ labels, int32_t* __restrict__ mapped,
    long long* __restrict__ winner) {
  for (long long p = (long long)blockIdx.x * kBlock + threadIdx.x; p < n_scene;
       p += (long long)gridDim.x * kBlock) {
    const unsigned long long key = keys[p];
    const int32_t l = key ? (int32_t)(key & (kMaxC - 1)) : 0;
    if (labels) labels[p] = l;
    if (winner) winner[p] = key ? (long long)(key >> PN2_VOTE_LABEL_BITS) - 1 : -1;
    if (mapped) mapped[p] = lut_of(l, lut, nlut, dflt);
  }
}

__global__ __launch_bounds__(kBlock) void map_back_rows_kernel(
    const uint8_t* __restrict__ values, int row_bytes, long long row0, long long rows,
    const unsigned long long* __restrict__ keys, int n_scene, uint8_t* __restrict__ out) {
  const bool v16 = (row_bytes & 15) == 0 && aligned16(values, out);
  const int units = v16 ? row_bytes / 16 : row_bytes / 4;
  const long long total = (long long)n_scene * units;
  for (long long e = (long long)blockIdx.x * kBlock + threadIdx.x; e < total;
       e += (long long)gridDim.x * kBlock) {
    const long long p = e / units;
    const int u = (int)(e - p * units);
    const unsigned long long key = keys[p];
    const long long w = (long long)(key >> PN2_VOTE_LABEL_BITS) - 1 - row0;  // key 0: < 0
    if (key != 0 && (w < 0 || w >= rows)) continue;  // another batch's row: left as it is
    if (v16)
      reinterpret_cast<uint4*>(out + p * row_bytes)[u] =
          key ? reinterpret_cast<const uint4*>(values + w * row_bytes)[u] : make_uint4(0, 0, 0, 0);
    else
      reinterpret_cast<uint32_t*>(out + p * row_bytes)[u] =
          key ? reinterpret_cast<const uint32_t*>(values + w * row_bytes)[u] : 0u;
  }
}

// in and out may be the same buffer: each element is read once, then written
__global__ __launch_bounds__(kBlock) void label_lut_kernel(const int32_t* in, long long n,
                                                           const int32_t* __restrict__ lut,
                                                           int nlut, int32_t dflt, int32_t* out) {
  for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n;
       i += (long long)gridDim.x * kBlock)
    out[i] = lut_of(in[i], lut, nlut, dflt);
}

unsigned blocks_for(long long n, int per_block, int cap = 4096) {
  long long b = (n + per_block - 1) / per_block;
  return (unsigned)(b > cap ? cap : b);
}

}  // namespace
}  // namespace pn2

extern "C" {

int pn2_scene_vote(const float* logits, long long rows, int C, const uint8_t* mask,
                   const int32_t* orig, long long row0, long long n_scene, long long* keys,
                   int32_t* pred_rows, pn2_stream_t stream) {
  using namespace pn2;
  if (logits && (C < 1 || C > kMaxC)) return PN2_EINVAL;
  if (rows < 0 || row0 < 0 || n_scene < 0 || n_scene >= (1LL << 31)) return PN2_EINVAL;
  if (rows >= (1LL << 55) || row0 >= (1LL << 55) - rows) return PN2_EINVAL;
  if (rows == 0) return PN2_OK;
  if (!mask || !orig || (n_scene > 0 && !keys)) return PN2_EINVAL;
  hipLaunchKernelGGL(scene_vote_kernel, dim3(blocks_for(rows, kVoteThreads, kVoteMaxBlocks)),
                     dim3(kVoteThreads), 0, (hipStream_t)stream, logits, rows, logits ? C : 1, mask, orig, row0,
                     (int)n_scene, reinterpret_cast<unsigned long long*>(keys), pred_rows);
  PN2_RETURN_LAUNCH();
}

int pn2_scene_labels(const long long* keys, long long n_scene, const int32_t* lut, int nlut,
                     int32_t dflt, int32_t* labels, int32_t* mapped, long long* winner,
                     pn2_stream_t stream) {
  using namespace pn2;
  if (n_scene < 0 || n_scene >= (1LL << 31) || nlut < 0) return PN2_EINVAL;
  if (mapped && !lut) return PN2_EINVAL;
  if (n_scene == 0) return PN2_OK;
  if (!keys) return PN2_EINVAL;
  if (!labels && !mapped && !winner) return PN2_OK;
  hipLaunchKernelGGL(scene_labels_kernel, dim3(blocks_for(n_scene, kBlock)), dim3(kBlock), 0,
                     (hipStream_t)stream, reinterpret_cast<const unsigned long long*>(keys),
                     (int)n_scene, lut, nlut, dflt, labels, mapped, winner);
  PN2_RETURN_LAUNCH();
}

int pn2_map_back_rows(const void* values, int row_bytes, long long row0, long long rows,
                      const long long* keys, long long n_scene, void* out, pn2_stream_t stream) {
  using namespace pn2;
  if (row_bytes <= 0 || (row_bytes & 3) || row0 < 0 || rows < 0) return PN2_EINVAL;
  if (n_scene < 0 || n_scene >= (1LL << 31)) return PN2_EINVAL;
  if (rows >= (1LL << 55) || row0 >= (1LL << 55) - rows) return PN2_EINVAL;
  if (n_scene == 0) return PN2_OK;
  if (!keys || !out || (rows > 0 && !values)) return PN2_EINVAL;
  hipLaunchKernelGGL(map_back_rows_kernel, dim3(blocks_for(n_scene * (row_bytes / 4), kBlock)),
                     dim3(kBlock), 0, (hipStream_t)stream, static_cast<const uint8_t*>(values),
                     row_bytes, row0, rows, reinterpret_cast<const unsigned long long*>(keys),
                     (int)n_scene, static_cast<uint8_t*>(out));
  PN2_RETURN_LAUNCH();
}

int pn2_label_lut(const int32_t* in, long long n, const int32_t* lut, int nlut, int32_t dflt,
                  int32_t* out, pn2_stream_t stream) {
  using namespace pn2;
  if (n < 0 || nlut < 0 || (nlut > 0 && !lut)) return PN2_EINVAL;
  if (n == 0) return PN2_OK;
  if (!in || !out) return PN2_EINVAL;
  hipLaunchKernelGGL(label_lut_kernel, dim3(blocks_for(n, kBlock)), dim3(kBlock), 0,
                     (hipStream_t)stream, in, n, lut, nlut, dflt, out);
  PN2_RETURN_LAUNCH();
}

}  // extern "C"
