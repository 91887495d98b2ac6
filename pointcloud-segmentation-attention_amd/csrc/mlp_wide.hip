// One conv / Dense layer over rows at ANY input width, gfx950: the K-streamed twin of the fused
// MLP's single-layer rows path (mlp.hip), for the layers whose input row does not fit that
// kernel's LDS (pn2_shared_mlp refuses them: 1,280 channels and up).
//
//   out[r][o] = act((sum_f x[r][f] * W[f][o]) * scale[o] + shift[o])
//
// over pn2_mlp_pack's packed layer, unchanged: Wp[to][c][h][i][s] = W[8c + 4h + s][32 to + i],
// then scale and shift (see mlp.hip).
//
// A workgroup of 256 threads owns 32*R rows and T output tiles of 32 columns (grid x = row
// blocks, grid y = tile groups). It walks K in slabs of KS columns: the rows' slab of x is staged
// into LDS (row stride KS + 4 floats, = 4 mod 32 as in mlp.hip's plan(), so the 16-byte reads of
// 8 consecutive rows hit distinct bank quads), two slab buffers: slab s + 1's global loads are
// issued before slab s's MFMAs and land in registers, are written to the other buffer after
// them, and one barrier per slab publishes it. Every wave keeps RG x TW accumulators of one
// 32 x 32 tile each in registers across all slabs: RG row tiles share each weight fragment (read
// from global memory, one float4 per lane per chunk, one group of chunks ahead), TW output tiles
// share each activation fragment. The four waves are laid out WR along the rows and 4 / WR
// along the output tiles, so R = RG * WR and T = TW * 4 / WR.
//
// Summation order. A row of up to 1,248 channels (156 chunks of 8: every row the fused kernel
// takes) is ONE chain per accumulator over the chunks in ascending order, four
// v_mfma_f32_32x32x2_f32 per chunk in mma_item's order (k = 8c + 4h + s, s = 0..3), in mma_item's
// non-LAST orientation (A = weights, B = activations: the staged single-layer rows path of
// pn2_shared_mlp): on a shape both kernels take the bits are pn2_shared_mlp's
// (tests/test_gpu_dense_wide.py). A wider row, which only this kernel takes, is cut into segments
// of 512 channels (64 chunks): one such chain per segment, and the segments' chains added in
// ascending order in a second set of registers (sum += chain). No reduction across waves or
// workgroups, no split-K, no atomics: the bits depend on cin alone, never on the launch shape.
// Why segments: one chain over 4,099 channels is 2,050 dependent fp32 additions, and its rounding
// error (measured: 4.5x that of numpy's blocked fp32 sum at 70 x 4,099 -> 21, and 4.2x in the
// input gradient of a 32 -> 1,280 training layer, one chain of 640 additions) misses the
// project's 4x bar; chains of 256 additions keep every width inside it.
//
// Budget (MI355X: 160 KiB LDS and 512 VGPRs per SIMD lane and CU). A slab buffer holds 8,192
// floats of x whatever R is (KS = 8192 / (32 R): 256, 128, 64 or 32 columns), so a workgroup
// takes 2 * (32 KiB + 512 R bytes) <= 72 KiB and two workgroups share a CU. A wave holds at most
// 4 accumulators and their 4 segment sums (128 VGPRs), 32 VGPRs of staged x, two groups of weight
// fragments (<= 32) and one of activation fragments (<= 16): under the 256 VGPRs that two waves
// per SIMD leave each.
// A chunk is 4 x RG x TW MFMAs of 64 cycles; the weight fragments are loaded one group of
// G chunks (>= 1,024 MFMA cycles) ahead.
#include <type_traits>

#include "common.h"

namespace pn2 {
namespace {

constexpr int kBlock = 256;
constexpr int kSlabFloats = 8192;  // floats of x per slab buffer
constexpr long long kFillBlocks = 256;  // workgroups that fill the chip (one per CU)
// A row of more than kOneChainChunks chunks of 8 channels (the widest the fused kernel takes) is
// summed in segments of kSegChunks chunks (see "Summation order").
constexpr int kOneChainChunks = 156, kSegChunks = 64;
constexpr int kMaxCin = 1 << 22;  // a thread's offset into its 256 rows of x is 32-bit (Stage)

struct WideParams {
  const float* x;
  const float4* w;     // packed weights [cout32][cin8][64] x 16 bytes
  const float* scale;  // [cout32*32]
  const float* shift;  // [cout32*32]
  float* out;
  long long rows;
  int cin, cin8, cout, cout32, relu, vec_out;
  int segmented;  // cin8 > kOneChainChunks
};

// The launch shape of a layer: RG row tiles x TW output tiles per wave, WR waves along the rows.
struct WideShape {
  int RG, TW, WR;
  int R() const { return RG * WR; }
  int T() const { return TW * (4 / WR); }
  int P() const { return 32 * R(); }
  int KS() const { return kSlabFloats / P(); }
  size_t lds() const { return 2 * (size_t)P() * (KS() + 4) * sizeof(float); }
};

// The waves go along the output tiles as far as the layer has tiles (cout32), the rest along
// the rows. Of the three accumulator shapes the largest that still gives kFillBlocks workgroups
// wins: 2 x 2 reads each weight and each activation fragment for two tiles, 1 x 2 and 1 x 1 give
// a layer over few rows two and four times the workgroups.
WideShape wide_shape(long long rows, int cout32) {
  static const int kAcc[3][2] = {{2, 2}, {1, 2}, {1, 1}};
  WideShape s = {};
  for (int i = 0; i < 3; ++i) {
    s.RG = kAcc[i][0];
    s.TW = kAcc[i][1];
    const int per = (cout32 + s.TW - 1) / s.TW;  // waves the tiles can use
    const int wt = per >= 4 ? 4 : per >= 2 ? 2 : 1;
    s.WR = 4 / wt;
    const long long blocks = (rows + s.P() - 1) / s.P();
    const long long groups = (cout32 + s.T() - 1) / s.T();
    if (blocks * groups >= kFillBlocks) break;
  }
  return s;
}

PN2_DEV float act(float v, int relu) { return relu ? fmaxf(v, 0.f) : v; }

// The slab of x that starts at column k0, for the workgroup's P rows from row0: issued as loads
// into registers (load), written to an LDS buffer later (store). Rows past `rows` and columns
// from cin up are zeros. VEC: 16-byte loads (cin % 4 == 0 and x 16-byte aligned), else one
// float per load with the same bits.
template <int P, int KS, bool VEC>
struct Stage {
  static constexpr int S = KS + 4;
  static constexpr int N = VEC ? kSlabFloats / 4 / kBlock : kSlabFloats / kBlock;
  using T = typename std::conditional<VEC, float4, float>::type;
  T v[N];
  // Unit e = tid + u * 256 lies in row e / U: rows p0 + u * (256 / U) for U <= 256 units per
  // row, so a thread's offset into the slab (p0 * cin + its column) is one 32-bit number for
  // the whole kernel and the rows' bases are uniform.
  PN2_DEV void load(const WideParams& prm, long long row0, int k0) {
    constexpr int U = VEC ? KS / 4 : KS;  // units per row
    static_assert(U <= kBlock, "a pass of the block covers whole rows");
    constexpr int RPU = kBlock / U;       // rows per pass
    const int p0 = (int)threadIdx.x / U, j = (int)threadIdx.x % U;
    const int col = k0 + (VEC ? 4 * j : j);
    const uint32_t toff = (uint32_t)p0 * (uint32_t)prm.cin + (uint32_t)(VEC ? 4 * j : j);
    const bool col_ok = col < prm.cin;
#pragma unroll
    for (int u = 0; u < N; ++u) {
      const long long rowu = row0 + u * RPU;  // uniform
      const float* base = prm.x + (size_t)rowu * prm.cin + k0;
      const bool ok = col_ok && rowu + p0 < prm.rows;
      if constexpr (VEC) {
        v[u] = ok ? *reinterpret_cast<const float4*>(base + toff)
                  : make_float4(0.f, 0.f, 0.f, 0.f);
      } else {
        v[u] = ok ? base[toff] : 0.f;
      }
    }
  }
  PN2_DEV void store(float* buf) const {
    constexpr int U = VEC ? KS / 4 : KS;
#pragma unroll
    for (int u = 0; u < N; ++u) {
      const int e = (int)threadIdx.x + u * kBlock;
      const int p = e / U, j = e % U;
      if constexpr (VEC) *reinterpret_cast<float4*>(buf + p * S + 4 * j) = v[u];
      else buf[p * S + j] = v[u];
    }
  }
};

template <int RG, int TW, int WR, bool VEC>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(2, 2))) void
dense_wide_kernel(const WideParams prm) {
  constexpr int WT = 4 / WR, P = 32 * RG * WR, KS = kSlabFloats / P, S = KS + 4;
  constexpr int T = TW * WT, CPS = KS / 8;                // chunks per slab
  constexpr int G = RG * TW >= 4 ? 2 : 4;                 // chunks per weight group
  static_assert(CPS % G == 0, "a slab holds whole groups");
  static_assert(kSegChunks % CPS == 0, "a segment holds whole slabs");
  extern __shared__ __attribute__((aligned(16))) float smem[];  // [2][P][S]

  const int lane = lane_id(), wave = (int)uniform_u32(threadIdx.x / kWave);
  const int col = lane & 31, h = lane >> 5;
  const int wr = wave % WR, wt = wave / WR;
  const long long row0 = (long long)blockIdx.x * P;
  const int cin8 = prm.cin8;

  // the wave's output tiles; one past the layer's last repeats it (loads stay in the pack)
  // and is neither multiplied nor stored
  int to[TW];
  bool tv[TW];
  const float4* wp[TW];
#pragma unroll
  for (int t = 0; t < TW; ++t) {
    const int want = (int)blockIdx.y * T + wt * TW + t;
    tv[t] = want < prm.cout32;
    to[t] = tv[t] ? want : prm.cout32 - 1;
    wp[t] = prm.w + (size_t)to[t] * cin8 * kWave + lane;
  }
  // this lane's activation row (+4h) of the wave's first row tile, in slab buffer 0
  const float* ap = smem + (32 * (wr * RG) + col) * S + 4 * h;

  // acc: the chain of the current segment of kSegChunks chunks; sum: the segments before it
  f32x16 acc[TW][RG], sum[TW][RG];
#pragma unroll
  for (int t = 0; t < TW; ++t)
#pragma unroll
    for (int r = 0; r < RG; ++r)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[t][r][i] = sum[t][r][i] = 0.f;

  auto mma4 = [&](const float4& w, const float4& a, f32x16& c) {
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(w.x, a.x, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(w.y, a.y, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(w.z, a.z, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(w.w, a.w, c, 0, 0, 0);
  };
  // chunk c of K lies in slab c / CPS, buffer (c / CPS) & 1, at column 8 (c % CPS)
  auto act4 = [&](int r, int c) {
    const int s = c / CPS;
    return *reinterpret_cast<const float4*>(ap + (s & 1) * (P * S) + r * (32 * S) +
                                            8 * (c - s * CPS));
  };
  auto load_w = [&](float4 (*w)[TW], int c) {
#pragma unroll
    for (int u = 0; u < G; ++u)
#pragma unroll
      for (int t = 0; t < TW; ++t) w[u][t] = wp[t][(size_t)(c + u) * kWave];
  };

  const int nslab = (cin8 + CPS - 1) / CPS;
  Stage<P, KS, VEC> st;
  st.load(prm, row0, 0);
  st.store(smem);
  __syncthreads();
  if (nslab > 1) st.load(prm, row0, KS);

  const int cg = cin8 - cin8 % G;
  float4 wA[G][TW], wB[G][TW];
  if (cg > 0) load_w(wA, 0);
  for (int c = 0; c < cg; c += G) {
    load_w(wB, c + G < cg ? c + G : c);  // the next group's weights (the last re-loads itself)
    float4 a[G][RG];
#pragma unroll
    for (int u = 0; u < G; ++u)
#pragma unroll
      for (int r = 0; r < RG; ++r) a[u][r] = act4(r, c + u);
#pragma unroll
    for (int u = 0; u < G; ++u)
#pragma unroll
      for (int t = 0; t < TW; ++t)
        if (tv[t]) {
#pragma unroll
          for (int r = 0; r < RG; ++r) mma4(wA[u][t], a[u][r], acc[t][r]);
        }
#pragma unroll
    for (int u = 0; u < G; ++u)
#pragma unroll
      for (int t = 0; t < TW; ++t) wA[u][t] = wB[u][t];
    const int c2 = c + G;
    if (c2 % CPS == 0 && c2 < cin8) {
      // slab s = c2 / CPS: its loads were issued a slab ago; its buffer was last read two slabs
      // ago, before the previous barrier
      const int s = c2 / CPS;
      // a segment ends: its chain joins the sum, a new one starts
      if (prm.segmented && c2 % kSegChunks == 0) {
#pragma unroll
        for (int t = 0; t < TW; ++t)
#pragma unroll
          for (int r = 0; r < RG; ++r) {
            sum[t][r] = sum[t][r] + acc[t][r];
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[t][r][i] = 0.f;
          }
      }
      st.store(smem + (s & 1) * (P * S));
      __syncthreads();
      if (s + 1 < nslab) st.load(prm, row0, (s + 1) * KS);
    }
  }
  for (int c = cg; c < cin8; ++c) {  // < G single chunks, all in the last slab
#pragma unroll
    for (int t = 0; t < TW; ++t) {
      const float4 w = wp[t][(size_t)c * kWave];
      if (tv[t]) {
#pragma unroll
        for (int r = 0; r < RG; ++r) mma4(w, act4(r, c), acc[t][r]);
      }
    }
  }

  // the last segment (one chain: 0 + the chain, its own bits)
#pragma unroll
  for (int t = 0; t < TW; ++t)
#pragma unroll
    for (int r = 0; r < RG; ++r) acc[t][r] = sum[t][r] + acc[t][r];

  // epilogue: register i of a tile = feature 32 to + 8 (i >> 2) + 4h + (i & 3) of row `col`
#pragma unroll
  for (int t = 0; t < TW; ++t) {
    if (!tv[t]) continue;
    float4 sc[4], sh[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int fb = 32 * to[t] + 8 * q + 4 * h;
      sc[q] = *reinterpret_cast<const float4*>(prm.scale + fb);
      sh[q] = *reinterpret_cast<const float4*>(prm.shift + fb);
    }
#pragma unroll
    for (int r = 0; r < RG; ++r) {
      const long long row = row0 + 32 * (wr * RG + r) + col;
      if (row >= prm.rows) continue;
      float* op = prm.out + (size_t)row * prm.cout;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int fb = 32 * to[t] + 8 * q + 4 * h;
        float4 y;
        y.x = act(acc[t][r][4 * q + 0] * sc[q].x + sh[q].x, prm.relu);
        y.y = act(acc[t][r][4 * q + 1] * sc[q].y + sh[q].y, prm.relu);
        y.z = act(acc[t][r][4 * q + 2] * sc[q].z + sh[q].z, prm.relu);
        y.w = act(acc[t][r][4 * q + 3] * sc[q].w + sh[q].w, prm.relu);
        if (prm.vec_out) {  // cout % 4 == 0: a quad is inside the row or past its end
          if (fb < prm.cout) *reinterpret_cast<float4*>(op + fb) = y;
        } else {
          if (fb + 0 < prm.cout) op[fb + 0] = y.x;
          if (fb + 1 < prm.cout) op[fb + 1] = y.y;
          if (fb + 2 < prm.cout) op[fb + 2] = y.z;
          if (fb + 3 < prm.cout) op[fb + 3] = y.w;
        }
      }
    }
  }
}

// Dynamic LDS beyond the 64 KiB default is opted into once per instantiation.
template <int RG, int TW, int WR, bool VEC>
int launch_wide(const WideParams& prm, const WideShape& sh, dim3 grid, hipStream_t s) {
  static const hipError_t attr = hipFuncSetAttribute(
      reinterpret_cast<const void*>(&dense_wide_kernel<RG, TW, WR, VEC>),
      hipFuncAttributeMaxDynamicSharedMemorySize, (int)WideShape{RG, TW, WR}.lds());
  if (attr != hipSuccess) return (int)attr;
  hipLaunchKernelGGL((dense_wide_kernel<RG, TW, WR, VEC>), grid, dim3(kBlock), sh.lds(), s, prm);
  PN2_RETURN_LAUNCH();
}

template <int RG, int TW, bool VEC>
int launch_wide_WR(const WideParams& prm, const WideShape& sh, dim3 grid, hipStream_t s) {
  if (sh.WR == 1) return launch_wide<RG, TW, 1, VEC>(prm, sh, grid, s);
  if (sh.WR == 2) return launch_wide<RG, TW, 2, VEC>(prm, sh, grid, s);
  return launch_wide<RG, TW, 4, VEC>(prm, sh, grid, s);
}

template <bool VEC>
int launch_wide_acc(const WideParams& prm, const WideShape& sh, dim3 grid, hipStream_t s) {
  if (sh.RG == 2) return launch_wide_WR<2, 2, VEC>(prm, sh, grid, s);
  if (sh.TW == 2) return launch_wide_WR<1, 2, VEC>(prm, sh, grid, s);
  return launch_wide_WR<1, 1, VEC>(prm, sh, grid, s);
}

// The checks that pn2_dense_wide and pn2_dense_wide_plan share; fills the launch shape and the
// grid (both 0 for rows = 0).
int wide_prepare(long long rows, int cin, const pn2_mlp_layer* layer, WideShape* sh,
                 long long* blocks, long long* groups) {
  *sh = WideShape{};
  *blocks = *groups = 0;
  if (rows < 0 || cin <= 0 || cin > kMaxCin || !layer) return PN2_EINVAL;
  if (!layer->packed || !aligned16(layer->packed)) return PN2_EINVAL;
  if (layer->cin != cin || layer->cout <= 0) return PN2_EINVAL;
  if (layer->flags & PN2_MLP_BF16) return PN2_EINVAL;  // fp32 only
  if (rows == 0) return PN2_OK;
  if (rows > 0x7fffffffLL) return PN2_EINVAL;
  const int cout32 = (layer->cout + 31) / 32;
  *sh = wide_shape(rows, cout32);
  *blocks = (rows + sh->P() - 1) / sh->P();
  *groups = (cout32 + sh->T() - 1) / sh->T();
  if (*groups > 65535) return PN2_EINVAL;  // grid y
  return PN2_OK;
}

}  // namespace
}  // namespace pn2

extern "C" {

int pn2_dense_wide_plan(long long rows, int cin, const pn2_mlp_layer* layer, int* row_tiles,
                        int* k_slab, int* out_tiles_per_wg) {
  using namespace pn2;
  if (!row_tiles || !k_slab || !out_tiles_per_wg) return PN2_EINVAL;
  *row_tiles = *k_slab = *out_tiles_per_wg = 0;
  WideShape sh;
  long long blocks, groups;
  const int rc = wide_prepare(rows, cin, layer, &sh, &blocks, &groups);
  if (rc || !blocks) return rc;
  *row_tiles = sh.R();
  *k_slab = sh.KS();
  *out_tiles_per_wg = sh.T();
  return PN2_OK;
}

int pn2_dense_wide(const float* x, long long rows, int cin, const pn2_mlp_layer* layer, float* out,
                   pn2_stream_t stream) {
  using namespace pn2;
  WideShape sh;
  long long blocks, groups;
  if (rows > 0 && (!x || !out)) return PN2_EINVAL;
  const int rc = wide_prepare(rows, cin, layer, &sh, &blocks, &groups);
  if (rc || !blocks) return rc;
  const int cin8 = (cin + 7) / 8, cout32 = (layer->cout + 31) / 32;
  const float* base = static_cast<const float*>(layer->packed);
  WideParams prm = {};
  prm.x = x;
  prm.w = reinterpret_cast<const float4*>(base);
  prm.scale = base + (size_t)cout32 * cin8 * 256;
  prm.shift = prm.scale + cout32 * 32;
  prm.out = out;
  prm.rows = rows;
  prm.cin = cin;
  prm.cin8 = cin8;
  prm.cout = layer->cout;
  prm.cout32 = cout32;
  prm.relu = (layer->flags & PN2_MLP_RELU) ? 1 : 0;
  prm.vec_out = layer->cout % 4 == 0 && aligned16(out);
  prm.segmented = cin8 > kOneChainChunks;
  const dim3 grid((unsigned)blocks, (unsigned)groups);
  if (cin % 4 == 0 && aligned16(x)) return launch_wide_acc<true>(prm, sh, grid, (hipStream_t)stream);
  return launch_wide_acc<false>(prm, sh, grid, (hipStream_t)stream);
}

}  // extern "C"
