// What the reference's training loop runs after the gradients exist
// (attention_points/train.py:288-387), gfx950: tf.train.AdamOptimizer's update of every variable
// and get_metrics' confusion matrix, accuracy counts and mean IoU. Host twins: cpu_optim.cpp.
//
//   pn2_adam_step      TF 1.x ApplyAdam over a table of (p, g, m, v, n) slots. The table travels
//                      by value in the kernel arguments (AdamArgs, PN2_ADAM_SLOTS slots and their
//                      first chunks): no device-side table, no copy, a step is
//                      ceil(nslots / PN2_ADAM_SLOTS) launches. Workgroup b owns chunk b: it finds
//                      its slot by a binary search of the chunk starts (scalar loads of the
//                      arguments, uniform over the workgroup) and streams PN2_ADAM_CHUNK elements,
//                      16 bytes read and 12 written per element, one float4 per thread and array
//                      when the slot's four pointers are 16-byte aligned. A chunk starts at a
//                      multiple of PN2_ADAM_CHUNK elements, so it is aligned when the slot is. No
//                      LDS, no atomics; each element is a function of its own inputs, so the
//                      launch shape cannot change a bit.
//   pn2_seg_confusion  a C x C histogram of 32-bit counters in LDS per PN2_CONFUSION_BLOCK_ROWS
//                      rows, flushed with 64-bit integer atomic adds (commutative: two runs give
//                      equal bits); the accuracy counts are the histogram's trace and total.
//   pn2_mean_iou       one workgroup: thread c owns class c, thread 0 adds in class order.
#include <math.h>

#include "common.h"

namespace pn2 {
namespace {

constexpr int kAdamThreads = 256;
constexpr int kAdamChunk = PN2_ADAM_CHUNK;
constexpr int kAdamSlots = PN2_ADAM_SLOTS;
static_assert(kAdamChunk % (4 * kAdamThreads) == 0, "a chunk is whole float4 rounds");
// 64 slots of at most 2^24 chunks: the grid stays below 2^31
static_assert(PN2_ADAM_MAX_N / kAdamChunk * kAdamSlots <= (1LL << 30), "grid bound");

// The kernel's only argument. start[i] is slot i's first chunk, start[nslots] the grid.
struct AdamArgs {
  pn2_adam_slot slot[kAdamSlots];
  uint32_t start[kAdamSlots + 1];
  float alpha, omb1, omb2, epsilon;
  int nslots;
};
static_assert(sizeof(AdamArgs) <= 4096, "the by-value argument block of one launch");

// ApplyAdam on one element; every operation rounds on its own (the file compiles with
// contraction off; sqrtf and / are the correctly rounded forms, denormals kept)
PN2_DEV void adam_elem(float& p, float g, float& m, float& v, float alpha, float omb1, float omb2,
                       float epsilon) {
  m = __fadd_rn(m, __fmul_rn(__fsub_rn(g, m), omb1));
  v = __fadd_rn(v, __fmul_rn(__fsub_rn(__fmul_rn(g, g), v), omb2));
  p = __fsub_rn(p, __fdiv_rn(__fmul_rn(alpha, m), __fadd_rn(sqrtf(v), epsilon)));
}

__global__ __launch_bounds__(kAdamThreads) void adam_kernel(const AdamArgs a) {
  const uint32_t b = blockIdx.x;
  // the last slot with start <= b (empty slots share their successor's start and never win)
  int lo = 0, hi = a.nslots;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a.start[mid] <= b) lo = mid;
    else hi = mid;
  }
  const pn2_adam_slot s = a.slot[lo];
  const long long e0 = (long long)(b - a.start[lo]) * kAdamChunk;
  const long long left = s.n - e0;
  if (left <= 0) return;  // (unreachable for a table the launcher built)
  const int len = left < kAdamChunk ? (int)left : kAdamChunk;
  float* p = s.p + e0;
  const float* g = s.g + e0;
  float* m = s.m + e0;
  float* v = s.v + e0;
  const float alpha = a.alpha, omb1 = a.omb1, omb2 = a.omb2, eps = a.epsilon;
  const bool vec = aligned16(s.p, s.g, s.m, s.v);
  int done = 0;
  if (vec) {  // uniform over the workgroup
    const int len4 = len >> 2;
    for (int q = threadIdx.x; q < len4; q += kAdamThreads) {
      float4 P = reinterpret_cast<float4*>(p)[q];
      const float4 G = reinterpret_cast<const float4*>(g)[q];
      float4 M = reinterpret_cast<float4*>(m)[q];
      float4 V = reinterpret_cast<float4*>(v)[q];
      adam_elem(P.x, G.x, M.x, V.x, alpha, omb1, omb2, eps);
      adam_elem(P.y, G.y, M.y, V.y, alpha, omb1, omb2, eps);
      adam_elem(P.z, G.z, M.z, V.z, alpha, omb1, omb2, eps);
      adam_elem(P.w, G.w, M.w, V.w, alpha, omb1, omb2, eps);
      reinterpret_cast<float4*>(m)[q] = M;
      reinterpret_cast<float4*>(v)[q] = V;
      reinterpret_cast<float4*>(p)[q] = P;
    }
    done = len4 << 2;
  }
  // the scalar path, or the chunk's last len % 4 elements
  for (int e = done + threadIdx.x; e < len; e += kAdamThreads) {
    float P = p[e], M = m[e], V = v[e];
    adam_elem(P, g[e], M, V, alpha, omb1, omb2, eps);
    m[e] = M;
    v[e] = V;
    p[e] = P;
  }
}

// ---------------------------------------------------------------- metrics ---------------
constexpr int kConfThreads = 256;
constexpr int kConfRows = PN2_CONFUSION_BLOCK_ROWS;
constexpr int kMaxC = PN2_METRICS_MAX_C;

__global__ __launch_bounds__(kConfThreads) void confusion_kernel(
    const int32_t* __restrict__ labels, const int32_t* __restrict__ pred, long long rows, int C,
    unsigned long long* __restrict__ confusion, unsigned long long* __restrict__ counts) {
  __shared__ uint32_t hist[kMaxC * kMaxC];
  __shared__ uint32_t tot[2];  // correct, assigned
  const int tid = threadIdx.x;
  const int cells = C * C;
  for (int k = tid; k < cells; k += kConfThreads) hist[k] = 0u;
  if (tid < 2) tot[tid] = 0u;
  __syncthreads();
  const long long r0 = (long long)blockIdx.x * kConfRows;
  const long long left = rows - r0;
  const int nr = left < kConfRows ? (int)left : kConfRows;
  for (int i = tid; i < nr; i += kConfThreads) {
    const int l = labels[r0 + i], q = pred[r0 + i];
    if (l > 0 && l < C && q >= 0 && q < C) atomicAdd(&hist[l * C + q], 1u);
  }
  __syncthreads();
  uint32_t correct = 0u, assigned = 0u;
  for (int k = tid; k < cells; k += kConfThreads) {
    const uint32_t n = hist[k];
    if (n) {
      atomicAdd(&confusion[k], (unsigned long long)n);
      assigned += n;
      if (k / C == k % C) correct += n;
    }
  }
  if (assigned) {
    atomicAdd(&tot[1], assigned);
    if (correct) atomicAdd(&tot[0], correct);
  }
  __syncthreads();
  if (tid < 2 && tot[tid]) atomicAdd(&counts[tid], (unsigned long long)tot[tid]);
}

__global__ __launch_bounds__(kMaxC) void mean_iou_kernel(const long long* __restrict__ cm, int C,
                                                         float* __restrict__ iou,
                                                         float* __restrict__ per_class) {
  __shared__ double val[kMaxC];
  __shared__ int valid[kMaxC];
  const int c = threadIdx.x;
  if (c < C) {
    long long row = 0, col = 0;
    for (int k = 0; k < C; ++k) {
      row += cm[c * C + k];
      col += cm[k * C + c];
    }
    const long long tp = cm[c * C + c], den = row + col - tp;
    const double v = den != 0 ? (double)tp / (double)den : 0.0;
    val[c] = v;
    valid[c] = den != 0;
    if (per_class) per_class[c] = (float)v;
  }
  __syncthreads();
  if (c == 0) {
    double s = 0.0;
    int n = 0;
    for (int k = 0; k < C; ++k)
      if (valid[k]) {
        s += val[k];
        ++n;
      }
    *iou = n ? (float)(s / (double)n) : 0.f;
  }
}

}  // namespace
}  // namespace pn2

extern "C" {

int pn2_adam_step(const pn2_adam_slot* slots, int nslots, float alpha, float beta1, float beta2,
                  float epsilon, pn2_stream_t stream) {
  using namespace pn2;
  if (nslots < 0 || (nslots > 0 && !slots)) return PN2_EINVAL;
  if (!(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f)) return PN2_EINVAL;
  if (!(epsilon >= 0.f) || !__builtin_isfinite(alpha)) return PN2_EINVAL;
  for (int i = 0; i < nslots; ++i) {
    const pn2_adam_slot& s = slots[i];
    if (s.n < 0 || s.n > PN2_ADAM_MAX_N) return PN2_EINVAL;
    if (s.n > 0 && (!s.p || !s.g || !s.m || !s.v)) return PN2_EINVAL;
  }
  bool launched = false;
  for (int i0 = 0; i0 < nslots; i0 += kAdamSlots) {
    AdamArgs a = {};
    a.nslots = nslots - i0 < kAdamSlots ? nslots - i0 : kAdamSlots;
    uint32_t chunks = 0;
    for (int i = 0; i < a.nslots; ++i) {
      a.slot[i] = slots[i0 + i];
      a.start[i] = chunks;
      chunks += (uint32_t)((slots[i0 + i].n + kAdamChunk - 1) / kAdamChunk);
    }
    a.start[a.nslots] = chunks;
    if (chunks == 0) continue;  // every slot of this launch is empty
    a.alpha = alpha;
    a.omb1 = 1.0f - beta1;
    a.omb2 = 1.0f - beta2;
    a.epsilon = epsilon;
    hipLaunchKernelGGL(adam_kernel, dim3(chunks), dim3(kAdamThreads), 0, (hipStream_t)stream, a);
    launched = true;
  }
  if (!launched) return PN2_OK;  // no slots, or none with an element
  PN2_RETURN_LAUNCH();
}

int pn2_seg_confusion(const int32_t* labels, const int32_t* pred, long long rows, int C,
                      long long* confusion, long long* counts, pn2_stream_t stream) {
  using namespace pn2;
  if (C <= 0 || C > kMaxC || rows < 0) return PN2_EINVAL;
  if (rows == 0) return PN2_OK;
  if (!labels || !pred || !confusion || !counts) return PN2_EINVAL;
  const long long nblk = (rows + kConfRows - 1) / kConfRows;
  if (nblk > 0x7fffffffLL) return PN2_EINVAL;
  hipLaunchKernelGGL(confusion_kernel, dim3((unsigned)nblk), dim3(kConfThreads), 0,
                     (hipStream_t)stream, labels, pred, rows, C,
                     reinterpret_cast<unsigned long long*>(confusion),
                     reinterpret_cast<unsigned long long*>(counts));
  PN2_RETURN_LAUNCH();
}

int pn2_mean_iou(const long long* confusion, int C, float* iou, float* per_class,
                 pn2_stream_t stream) {
  using namespace pn2;
  if (C <= 0 || C > kMaxC || !confusion || !iou) return PN2_EINVAL;
  hipLaunchKernelGGL(mean_iou_kernel, dim3(1), dim3(kMaxC), 0, (hipStream_t)stream, confusion, C,
                     iou, per_class);
  PN2_RETURN_LAUNCH();
}

}  // extern "C"
