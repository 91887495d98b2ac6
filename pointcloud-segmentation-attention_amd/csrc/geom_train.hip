// Training-mode geometry of the SA and FP modules: the gradients of group_point and
// three_interpolate as ordered gathers, gfx950.
//
// pn2_group_point_grad (group.hip) and pn2_three_interpolate_grad (interp.hip) scatter with float
// atomicAdd into a zero-filled buffer, like the reference's GPU grouping gradient
// (tf_grouping_g.cu:61-78): the order of the adds, and so the last bits of the sums, change from
// run to run. The entry points here turn the scatter round. An inverse index lists, per
// destination row ("key"), the source rows ("slots") that name it, in ascending slot order; the
// gradient kernels then give every destination element to one thread that adds its slots in that
// order, starting from +0.0f, one __fadd_rn per slot:
//
//   grad[b][key][c] = ((+0.0f + g[s0]) + g[s1]) + ...          s0 < s1 < ... the key's slots
//
// which is the sequential loop of the reference's CPU ThreeInterpolateGrad
// (tf_interpolate.cpp:131-153, pn2cpu_three_interpolate_grad) for every destination element.
// No float atomics, no zero-fill pass (every element is written once), and the source is read in
// place through a row stride and a column offset, so the gradient of a concatenation needs no
// slice copy.
//
// Inverse index (pn2_inverse_index_build), workspace of pn2_inverse_index_size bytes:
//   int32 offsets[B][K + 1]     exclusive prefix of the keys' counts; offsets[b][K] = the number
//                               of slots of cloud b with a key in [0, K)
//   (padding to 16 bytes)
//   int32 slots[B][S]           cloud b's slots grouped by key: key k's are
//                               slots[b][offsets[b][k] .. offsets[b][k + 1]), ascending
// Two launches. inv_build_kernel: one workgroup of 1024 threads per cloud counts the keys in LDS
// (integer atomics: exact), scans the counts (each thread a contiguous run of keys, a wave scan
// and the 16 wave totals), and places every slot at its key's LDS cursor (an integer atomic
// again: the position inside a segment depends on arrival order). inv_sort_kernel then makes
// every segment a pure function of the keys, one wave per key: a segment of at most 512 slots is
// ranked in registers, up to eight per lane (slot numbers are distinct, so "how many are
// smaller" is a permutation; cfg2's FP4 reaches 83 slots on a key: with one register per lane
// those keys took the scan below and FP4's build 67 us instead of 46);
// a longer one is not sorted at all but written again as the stream compaction of
// `keys[s] == k` over the cloud's S slots in ascending s (ballot + popcount), which is ascending
// by construction and takes S / 64 steps however long the segment is: a cloud whose slots all
// share one key costs one wave S / 64 steps, never a quadratic sort.
#include "common.h"

namespace pn2 {
namespace {

constexpr int kInvBlock = 1024;              // inv_build_kernel: one workgroup per cloud
constexpr int kInvWaves = kInvBlock / kWave;
constexpr int kInvUnroll = 8;                // key loads a thread issues before their LDS atomics
constexpr int kSortBlock = 256;              // inv_sort_kernel: four waves, one key each
constexpr int kSortWaves = kSortBlock / kWave;
constexpr int kSortMaxGridX = 4096;          // then the waves stride over the keys
constexpr int kRankRegs = 8;                 // a segment of up to 64 x 8 slots is ranked in registers
constexpr int kSortUnroll = 4;               // key chunks a long segment's scan has in flight
constexpr int kGradBlock = 256;
constexpr int kGradUnroll = 4;               // slots whose loads are issued before their adds
constexpr int kMaxBatch = 65535;             // clouds are grid y

inline size_t align4(size_t words) { return (words + 3) & ~(size_t)3; }
inline size_t inv_slot_base(int B, int K) { return align4((size_t)B * ((size_t)K + 1)); }

__global__ __launch_bounds__(kInvBlock) void inv_build_kernel(const int32_t* __restrict__ keys,
                                                              int S, int K,
                                                              int32_t* __restrict__ offsets,
                                                              int32_t* __restrict__ slots) {
  extern __shared__ int s_inv[];  // K counts (then cursors), kInvWaves wave totals
  int* s_cnt = s_inv;
  int* s_wave = s_inv + K;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int32_t* key = keys + (size_t)blockIdx.x * S;
  int32_t* off = offsets + (size_t)blockIdx.x * ((size_t)K + 1);
  int32_t* slot = slots + (size_t)blockIdx.x * S;
  for (int k = tid; k < K; k += kInvBlock) s_cnt[k] = 0;
  __syncthreads();
  // (a thread's kInvUnroll key loads are issued together, not one per trip: DESIGN.md 3.9)
  for (int s0 = tid; s0 < S; s0 += kInvBlock * kInvUnroll) {
    int k[kInvUnroll];
#pragma unroll
    for (int u = 0; u < kInvUnroll; ++u) {
      const int s = s0 + u * kInvBlock;
      k[u] = s < S ? key[s] : -1;
    }
#pragma unroll
    for (int u = 0; u < kInvUnroll; ++u)
      if ((unsigned)k[u] < (unsigned)K) atomicAdd(&s_cnt[k[u]], 1);  // outside [0, K): left out
  }
  __syncthreads();
  // exclusive scan of the counts: thread t owns keys [t * per, (t + 1) * per)
  const int per = (K + kInvBlock - 1) / kInvBlock;
  const int k0 = min(tid * per, K), k1 = min(k0 + per, K);
  int sum = 0;
  for (int k = k0; k < k1; ++k) sum += s_cnt[k];
  int inc = sum;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const int v = __shfl_up(inc, o, kWave);
    if (lane >= o) inc += v;
  }
  if (lane == kWave - 1) s_wave[wave] = inc;
  __syncthreads();
  int base = inc - sum;
  for (int w = 0; w < wave; ++w) base += s_wave[w];
  for (int k = k0; k < k1; ++k) {
    const int c = s_cnt[k];
    off[k] = base;
    s_cnt[k] = base;  // the key's cursor
    base += c;
  }
  if (tid == kInvBlock - 1) off[K] = base;  // (the last thread's prefix is the total)
  __syncthreads();
  for (int s0 = tid; s0 < S; s0 += kInvBlock * kInvUnroll) {
    int k[kInvUnroll];
#pragma unroll
    for (int u = 0; u < kInvUnroll; ++u) {
      const int s = s0 + u * kInvBlock;
      k[u] = s < S ? key[s] : -1;
    }
#pragma unroll
    for (int u = 0; u < kInvUnroll; ++u)
      if ((unsigned)k[u] < (unsigned)K)
        slot[atomicAdd(&s_cnt[k[u]], 1)] = s0 + u * kInvBlock;  // position < off[K] <= S
  }
}

// Sorts a segment of L <= 64 * R distinct slot numbers in place, a lane holding elements lane,
// lane + 64, ...: the rank of an element is how many of the segment are smaller.
template <int R>
PN2_DEV void rank_segment(int32_t* seg, int L, int lane) {
  int x[R], rank[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int e = r * kWave + lane;
    x[r] = e < L ? seg[e] : INT32_MAX;
    rank[r] = 0;
  }
#pragma unroll
  for (int q = 0; q < R; ++q) {
    const int nq = min(L - q * kWave, kWave);  // elements held in register q
    for (int j = 0; j < nq; ++j) {
      const int v = __builtin_amdgcn_readlane(x[q], j);
#pragma unroll
      for (int r = 0; r < R; ++r) rank[r] += v < x[r] ? 1 : 0;
    }
  }
  // (every load of the wave is done: each x fed the ranks)
#pragma unroll
  for (int r = 0; r < R; ++r)
    if (r * kWave + lane < L) seg[rank[r]] = x[r];
}

__global__ __launch_bounds__(kSortBlock) void inv_sort_kernel(const int32_t* __restrict__ keys,
                                                              int S, int K,
                                                              const int32_t* __restrict__ offsets,
                                                              int32_t* __restrict__ slots) {
  const int lane = threadIdx.x & (kWave - 1);
  const int32_t* key = keys + (size_t)blockIdx.y * S;
  const int32_t* off = offsets + (size_t)blockIdx.y * ((size_t)K + 1);
  int32_t* slot = slots + (size_t)blockIdx.y * S;
  const int nwaves = gridDim.x * kSortWaves;
  for (int k = blockIdx.x * kSortWaves + threadIdx.x / kWave; k < K; k += nwaves) {
    const int o0 = (int)uniform_u32((uint32_t)off[k]);
    const int L = (int)uniform_u32((uint32_t)off[k + 1]) - o0;
    if (L <= 1) continue;
    if (L <= kWave) {
      rank_segment<1>(slot + o0, L, lane);
    } else if (L <= kWave * 2) {
      rank_segment<2>(slot + o0, L, lane);
    } else if (L <= kWave * 4) {
      rank_segment<4>(slot + o0, L, lane);
    } else if (L <= kWave * kRankRegs) {
      rank_segment<kRankRegs>(slot + o0, L, lane);
    } else {
      // the segment again as the compaction of keys[s] == k over ascending s
      int p = o0;
      for (int s0 = 0; s0 < S; s0 += kWave * kSortUnroll) {
        int kk[kSortUnroll];
#pragma unroll
        for (int u = 0; u < kSortUnroll; ++u) {
          const int s = s0 + u * kWave + lane;
          kk[u] = s < S ? key[s] : -1;  // (k >= 0: -1 never matches)
        }
#pragma unroll
        for (int u = 0; u < kSortUnroll; ++u) {
          const bool hit = kk[u] == k;
          const uint64_t mask = __ballot(hit);
          const int q = p + __popcll(mask & (((uint64_t)1 << lane) - 1));
          if (hit && q < o0 + L) slot[q] = s0 + u * kWave + lane;
          p += __popcll(mask);
        }
      }
    }
  }
}

// One thread per destination element (b, key, c): `cpl` = 2^cpl_log2 lanes share a row (the next
// power of two >= min(C, 256), so the row and channel of a thread are a shift and a mask), a
// workgroup holds 256 / cpl rows and a thread strides over the channels beyond cpl. The slot
// numbers of a row are the same address in all its lanes (one request), the source row is read
// across the lanes. The adds of a row are sequential by contract; the loads of kGradUnroll slots
// are issued before their adds. offsets == nullptr: no slots at all (every row is +0.0f).
template <bool kWeighted>
__global__ __launch_bounds__(kGradBlock) void grad_ordered_kernel(
    const float* __restrict__ grad_out, int ld, int col0, const int32_t* __restrict__ offsets,
    const int32_t* __restrict__ slots, const float* __restrict__ weight, int K, int C, int S,
    int cpl_log2, float* __restrict__ grad_points) {
  const int cpl = 1 << cpl_log2, rpb = kGradBlock >> cpl_log2;
  const int rl = threadIdx.x >> cpl_log2, c0 = threadIdx.x & (cpl - 1);
  const size_t b = blockIdx.y;
  // source rows of cloud b: one per slot (grouping), one per three slots (interpolation)
  const float* go = grad_out + b * (size_t)(kWeighted ? S / 3 : S) * ld + col0;
  const int32_t* off = offsets ? offsets + b * ((size_t)K + 1) : nullptr;
  const int32_t* slot = slots + b * S;
  const float* w = kWeighted ? weight + b * S : nullptr;
  float* gp = grad_points + b * K * C;
  for (int t = blockIdx.x; t * rpb < K; t += gridDim.x) {
    const int k = t * rpb + rl;
    if (k >= K) continue;
    const int o0 = off ? off[k] : 0, o1 = off ? off[k + 1] : 0;
    for (int c = c0; c < C; c += cpl) {
      float acc = 0.0f;
      int j = o0;
      for (; j + kGradUnroll <= o1; j += kGradUnroll) {
        float g[kGradUnroll];
#pragma unroll
        for (int u = 0; u < kGradUnroll; ++u) {
          const int s = slot[j + u];
          if (kWeighted) g[u] = __fmul_rn(go[(size_t)(s / 3) * ld + c], w[s]);
          else g[u] = go[(size_t)s * ld + c];
        }
#pragma unroll
        for (int u = 0; u < kGradUnroll; ++u) acc = __fadd_rn(acc, g[u]);
      }
      for (; j < o1; ++j) {
        const int s = slot[j];
        const float g = kWeighted ? __fmul_rn(go[(size_t)(s / 3) * ld + c], w[s])
                                  : go[(size_t)s * ld + c];
        acc = __fadd_rn(acc, g);
      }
      gp[(size_t)k * C + c] = acc;
    }
  }
}

// Shared argument check and launch of the two gradients: K keys (destination rows) and S slots
// per cloud, source rows of `ld` floats read at columns [col0, col0 + C).
int grad_ordered(const float* grad_out, int ld, int col0, const void* inv, const float* weight,
                 bool weighted, int B, int K, int C, long long S, float* grad_points,
                 hipStream_t s) {
  if (B < 0 || K < 0 || C < 0 || S < 0 || ld < 0 || col0 < 0) return PN2_EINVAL;
  if ((long long)col0 + C > ld) return PN2_EINVAL;
  if (B > kMaxBatch || K > PN2_INV_MAX_KEYS || S > PN2_INV_MAX_SLOTS) return PN2_EINVAL;
  if ((long long)B * K * C == 0) return PN2_OK;
  if (!grad_points) return PN2_EINVAL;
  if (S > 0 && (!grad_out || !inv || (weighted && !weight))) return PN2_EINVAL;
  if (!aligned16(inv)) return PN2_EINVAL;
  const int32_t* offsets = S > 0 ? (const int32_t*)inv : nullptr;
  const int32_t* slots = S > 0 ? (const int32_t*)inv + inv_slot_base(B, K) : nullptr;
  int cpl_log2 = 0;
  while ((1 << cpl_log2) < C && (1 << cpl_log2) < kGradBlock) ++cpl_log2;
  const int rpb = kGradBlock >> cpl_log2;
  const dim3 grid((unsigned)((K + rpb - 1) / rpb), (unsigned)B);
  if (weighted)
    hipLaunchKernelGGL(grad_ordered_kernel<true>, grid, dim3(kGradBlock), 0, s, grad_out, ld, col0,
                       offsets, slots, weight, K, C, (int)S, cpl_log2, grad_points);
  else
    hipLaunchKernelGGL(grad_ordered_kernel<false>, grid, dim3(kGradBlock), 0, s, grad_out, ld,
                       col0, offsets, slots, weight, K, C, (int)S, cpl_log2, grad_points);
  PN2_RETURN_LAUNCH();
}

}  // namespace
}  // namespace pn2

extern "C" {

size_t pn2_inverse_index_size(int B, int S, int K) {
  if (B <= 0 || S < 0 || K < 0) return 0;
  return 4 * (pn2::inv_slot_base(B, K) + pn2::align4((size_t)B * (size_t)S));
}

int pn2_inverse_index_build(const int32_t* keys, int B, int S, int K, void* inv, size_t inv_bytes,
                            pn2_stream_t stream) {
  if (B < 0 || S < 0 || K < 0) return PN2_EINVAL;
  if (B > pn2::kMaxBatch || K > PN2_INV_MAX_KEYS || S > PN2_INV_MAX_SLOTS) return PN2_EINVAL;
  if (B == 0 || S == 0) return PN2_OK;
  if (!keys || !inv || !pn2::aligned16(inv)) return PN2_EINVAL;
  if (inv_bytes < pn2_inverse_index_size(B, S, K)) return PN2_EINVAL;
  constexpr int kLdsMax = (PN2_INV_MAX_KEYS + pn2::kInvWaves) * 4;
  static const hipError_t attr = hipFuncSetAttribute(
      reinterpret_cast<const void*>(&pn2::inv_build_kernel),
      hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax);
  if (attr != hipSuccess) return (int)attr;
  hipStream_t s = (hipStream_t)stream;
  int32_t* offsets = (int32_t*)inv;
  int32_t* slots = offsets + pn2::inv_slot_base(B, K);
  hipLaunchKernelGGL(pn2::inv_build_kernel, dim3((unsigned)B), dim3(pn2::kInvBlock),
                     (size_t)(K + pn2::kInvWaves) * 4, s, keys, S, K, offsets, slots);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  if (K == 0) return PN2_OK;
  const int gx = (K + pn2::kSortWaves - 1) / pn2::kSortWaves;
  hipLaunchKernelGGL(pn2::inv_sort_kernel,
                     dim3((unsigned)(gx < pn2::kSortMaxGridX ? gx : pn2::kSortMaxGridX),
                          (unsigned)B),
                     dim3(pn2::kSortBlock), 0, s, keys, S, K, offsets, slots);
  PN2_RETURN_LAUNCH();
}

int pn2_group_point_grad_ordered(const float* grad_out, int ld, int col0, const void* inv, int B,
                                 int N, int C, int M, int nsample, float* grad_points,
                                 pn2_stream_t stream) {
  if (M < 0 || nsample < 0) return PN2_EINVAL;
  return pn2::grad_ordered(grad_out, ld, col0, inv, nullptr, false, B, N, C,
                           (long long)M * nsample, grad_points, (hipStream_t)stream);
}

int pn2_three_interpolate_grad_ordered(const float* grad_out, int ld, int col0, const void* inv,
                                       const float* weight, int B, int n, int C, int m,
                                       float* grad_points, pn2_stream_t stream) {
  if (n < 0) return PN2_EINVAL;
  return pn2::grad_ordered(grad_out, ld, col0, inv, weight, true, B, m, C, 3LL * n, grad_points,
                           (hipStream_t)stream);
}

}  // extern "C"
