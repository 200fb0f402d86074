// Byzantine-robust aggregation of a sync round's W gathered dense wires (--aggregate trimmed /
// median / krum): one fp32 estimate e of the workers' mean gradient that a minority of bad wires
// (diverged, bit-flipped, inf / NaN) cannot move, written as agg = e * c for the dense entry of
// every server optimizer (c = 1 / weight, so that the rule's weight * agg is e).
//
// x_(0) <= ... <= x_(W-1): the W decoded values of one coordinate, sorted, NaN counted as +inf.
//   trimmed : e = (sum_{r=T}^{W-1-T} x_(r)) * fl(1 / (W - 2T)), the sum in fp32 in rank order from 0
//   median  : e = x_((W-1)/2) (odd W), 0.5f * (x_(W/2-1) + x_(W/2)) (even W)
//   krum    : multi-Krum (Blanchard et al. 2017). G = X X^T over the whole arena, d2_ij = G_ii + G_jj
//             - 2 G_ij (non-finite: +inf), score_i = sum of the W-F-2 smallest d2_ij, j != i; the m =
//             W-F smallest scores are selected (ties: lower index; a non-finite score ranks last);
//             e = (sum of the selected wires, fp32, source order) * fl(1 / m)
//
// robust_rank_kernel: one streaming pass over the wires. A lane holds its 8 coordinates of all
// sources in registers (fp16 wires: 4 packed registers per source, two coordinates per v_pk_min_f16
// / v_pk_max_f16; fp16 ordering is exact, values widen to fp32 only when they are summed) and sorts
// them with Batcher's odd-even merge network of NW = 4, 8, 16 or 32 inputs (5, 19, 63, 191
// compare-exchanges). No loop over memory, no LDS, no branch on data. W < NW is padded:
//   trimmed : with +inf, so ranks 0..W-1 are the real values; the window is summed under
//             grid-uniform predicates on the rank;
//   median  : with floor((NW-W)/2) times -inf below and the rest +inf above, which puts the middle
//             of the real values at the fixed ranks NW/2-1 and NW/2: only two outputs of the network
//             are live, and the compiler drops every compare-exchange they do not depend on.
// NaN -> +inf is two v_min with +inf on load (IEEE mode: the first quiets a signalling NaN, the
// second returns the other operand). fp32 wires at NW = 32 take the group of 8 in two passes of 4
// (128 value registers, as the fp16 form). The scalar form (chunk head and tail, unaligned sources)
// runs the same network on one coordinate: same values, same order, same bits. -0 and +0 compare
// equal; which one a min / max returns is not specified.
//
// robust_gram_kernel: G = X X^T on MFMA, X = the sources as rows of a [32 x n] operand (rows >= W
// zero). A workgroup owns kGramSlice consecutive arena elements, stages them [W x kGramTile] at a
// time through LDS (each wave whole rows: 16-byte loads, coalesced), and every wave multiplies a
// quarter of the tile's k-steps: fp16 wires feed v_mfma_f32_16x16x32_f16 directly, fp32 wires the
// exact-fp32 16x16x4. A 16-row fragment serves as A and as B operand; only the upper 16x16 tiles
// are computed (3 of 4; 1 when W <= 16). The four waves' accumulators are summed in wave order
// through LDS, and the workgroup writes its fp32 partial [32][32] (upper tiles). No atomics; slice
// and grid depend on n alone.
//
// robust_krum_select_kernel: one workgroup reduces the partials in block order in double, forms
// d2, the scores and the selection, writes sel[32] (0 / 1 floats) and bumps the per-worker
// selection counters of the state block with plain stores.
//
// robust_select_sum_kernel: the chunk walk of the other update kernels; an unselected wire is not
// read (0 * inf would poison the sum).
#include <utility>

#include "wire.hpp"

namespace psx {

constexpr int kGramSlice = 16384;  // arena elements per workgroup of the Gram kernel: the longest fp32 chain
constexpr int kGramTile = 512;     // elements per source staged through LDS at a time
constexpr int kKindTrimmed = 0, kKindMedian = 1;

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

struct RobustState {
  long long selected[kMaxSrc];  // rounds in which multi-Krum selected worker k
};

// ---- the rank kernel ----

// min / max of a value register: a packed pair of halves (fp16 wires) or one float. Spelled as
// instructions: the generic builtins canonicalise both operands first (three instructions for one).
PSX_DEV uint32_t vmin(uint32_t a, uint32_t b) {
  uint32_t d;
  asm("v_pk_min_f16 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
  return d;
}
PSX_DEV uint32_t vmax(uint32_t a, uint32_t b) {
  uint32_t d;
  asm("v_pk_max_f16 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
  return d;
}
PSX_DEV float vmin(float a, float b) {
  float d;
  asm("v_min_f32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
  return d;
}
PSX_DEV float vmax(float a, float b) {
  float d;
  asm("v_max_f32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
  return d;
}

template <typename V>
PSX_DEV V vinf(bool neg);
template <>
PSX_DEV uint32_t vinf<uint32_t>(bool neg) {
  return neg ? 0xfc00fc00u : 0x7c007c00u;
}
template <>
PSX_DEV float vinf<float>(bool neg) {
  return neg ? -__builtin_inff() : __builtin_inff();
}

// coordinate c of the NV value registers of one rank as fp32
template <int NV>
PSX_DEV float widen(const uint32_t (&v)[NV], int c) {
  const uint32_t w = v[c >> 1];
  return (float)__builtin_bit_cast(_Float16, (uint16_t)((c & 1) ? (w >> 16) : (w & 0xffff)));
}
template <int NV>
PSX_DEV float widen(const float (&v)[NV], int c) {
  return v[c];
}

// Batcher's odd-even merge sort of NW rows of NV registers each, ascending in every coordinate.
// Step (p, k) holds the compare-exchange (a, a + k) iff a >= k % p, ((a - k % p) mod 2k) < k, a + k <
// NW and both fall into one block of 2p. The steps are expanded at compile time (a fold over the
// flattened (p, k, a) index), so the network is straight-line code on registers whatever the
// unroller's size limits are.
template <int... I, typename F>
PSX_DEV void static_for_seq(std::integer_sequence<int, I...>, F&& f) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int NW, int NV, typename V>
PSX_DEV void sort_net(V (&v)[NW][NV]) {
  constexpr int LOG = NW == 4 ? 2 : NW == 8 ? 3 : NW == 16 ? 4 : 5;
  static_for_seq(std::make_integer_sequence<int, LOG * LOG * NW>{}, [&](auto S) {
    constexpr int s = decltype(S)::value, lp = s / (LOG * NW), lq = s / NW % LOG, a = s % NW;
    constexpr int p = 1 << lp, lk = lp - lq, k = lk >= 0 ? 1 << lk : NW, o = k % p, b = a + k;
    if constexpr (lk >= 0 && a >= o && ((a - o) % (2 * k)) < k && b < NW && a / (2 * p) == b / (2 * p)) {
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        const V lo = vmin(v[a][j], v[b][j]), hi = vmax(v[a][j], v[b][j]);
        v[a][j] = lo;
        v[b][j] = hi;
      }
    }
  });
}

struct RankArgs {
  int trim;     // T (trimmed)
  float recip;  // fl(1 / (W - 2T)) (trimmed)
  float c;      // the scale on the estimate
};

// NC consecutive coordinates at arena element i (NC = 8 or 4: vector loads, every source + i 16-byte
// aligned; NC = 1: scalar) of all sources: loaded, NaN -> +inf, padded, sorted, estimated into e
template <typename GT, int NW, int KIND, int NC>
PSX_DEV void rank_coords(const WireSrcs& srcs, long i, const RankArgs& ra, float (&e)[NC]) {
  constexpr bool H = sizeof(GT) == 2;
  using V = std::conditional_t<H, uint32_t, float>;
  constexpr int NV = H ? (NC + 1) / 2 : NC;
  static_assert(NC == 1 || (H ? NC == 8 : (NC == 8 || NC == 4)), "rank_coords NC");
  const int W = srcs.n, nlo = KIND == kKindMedian ? (NW - W) >> 1 : 0;
  const V inf = vinf<V>(false);
  V v[NW][NV];
#pragma unroll
  for (int k = 0; k < NW; ++k) {
    if (k < W) {  // grid-uniform
      const GT* g = reinterpret_cast<const GT*>(srcs.p[k]) + i;
      if constexpr (NC == 1) {
        if constexpr (H) v[k][0] = (uint32_t)g[0];
        else v[k][0] = g[0];
      } else if constexpr (H) {
        const u32x4 w = *reinterpret_cast<const u32x4*>(g);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[k][j] = w[j];
      } else {
#pragma unroll
        for (int q = 0; q < NC / 4; ++q) {
          const f32x4 w = *reinterpret_cast<const f32x4*>(g + 4 * q);
#pragma unroll
          for (int j = 0; j < 4; ++j) v[k][4 * q + j] = w[j];
        }
      }
#pragma unroll
      for (int j = 0; j < NV; ++j) v[k][j] = vmin(vmin(v[k][j], inf), inf);
    } else {
      const V pad = vinf<V>(k - W < nlo);
#pragma unroll
      for (int j = 0; j < NV; ++j) v[k][j] = pad;
    }
  }
  sort_net<NW, NV>(v);
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    if constexpr (KIND == kKindMedian) {
      const float lo = widen<NV>(v[NW / 2 - 1], c), hi = widen<NV>(v[NW / 2], c);
      e[c] = ((W & 1) ? lo : 0.5f * (lo + hi)) * ra.c;
    } else {
      float s = 0.f;
#pragma unroll
      for (int r = 0; r < NW; ++r)
        if (r >= ra.trim && r < W - ra.trim) s += widen<NV>(v[r], c);  // grid-uniform
      e[c] = (s * ra.recip) * ra.c;
    }
  }
}

template <typename GT, int NW, int KIND, bool VEC>
__global__ __launch_bounds__(256) void robust_rank_kernel(WireSrcs srcs, float* __restrict__ agg, long n, long off,
                                                          long cnt, RankArgs ra) {
  const ChunkRange r = chunk_range(off, cnt, blockIdx.x, n);
  for_chunk<VEC>(
      r,
      [&](long i) {
        float e[1];
        rank_coords<GT, NW, KIND, 1>(srcs, i, ra, e);
        agg[i] = e[0];
      },
      [&](long i) {
        if constexpr (sizeof(GT) == 4 && NW == 32) {  // the register budget: 4 coordinates at a time
#pragma unroll 1
          for (int h = 0; h < 2; ++h) {
            float e[4];
            rank_coords<GT, NW, KIND, 4>(srcs, i + 4 * h, ra, e);
            *reinterpret_cast<f32x4*>(agg + i + 4 * h) = (f32x4){e[0], e[1], e[2], e[3]};
          }
        } else {
          float e[8];
          rank_coords<GT, NW, KIND, 8>(srcs, i, ra, e);
          st8(agg + i, e);
        }
      });
}

// ---- multi-Krum ----

// GT: wire element. VEC: every source 16-byte aligned (full tiles are staged with 16-byte loads).
template <typename GT, bool VEC>
__global__ __launch_bounds__(256) void robust_gram_kernel(WireSrcs srcs, long n, float* __restrict__ partials) {
  constexpr bool H = sizeof(GT) == 2;
  constexpr int EPV = 16 / (int)sizeof(GT);  // elements per 16 bytes
  constexpr int LD = kGramTile + EPV;        // row stride: 16-byte aligned, rows 16 bytes apart in the banks
  constexpr int KS = H ? 32 : 16;            // elements of one k-step: one f16 MFMA, or four 16x16x4
  __shared__ __attribute__((aligned(16))) GT xs[kMaxSrc * LD];
  static_assert(sizeof(xs) >= 4 * 3 * 256 * sizeof(float), "the wave sums reuse the staging buffer");
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int W = srcs.n;
  const bool two = W > 16;
  const long a0 = (long)blockIdx.x * kGramSlice, a1 = min(n, a0 + kGramSlice);
  for (int q = tid; q < kMaxSrc * LD; q += 256) xs[q] = GT(0);  // rows >= W stay zero
  f32x4 acc[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};  // tiles (0,0), (0,1), (1,1)
  const GT* frag = xs + (lane & 15) * LD + EPV * (lane >> 4);
  for (long t0 = a0; t0 < a1; t0 += kGramTile) {
    __syncthreads();  // the zeroes, or the last tile's fragment reads
    const bool full = VEC && t0 + kGramTile <= a1;
    for (int r = wave; r < W; r += 4) {
      const GT* g = reinterpret_cast<const GT*>(srcs.p[r]) + t0;
      GT* row = xs + r * LD;
      if (full) {
#pragma unroll
        for (int q = 0; q < kGramTile / EPV / 64; ++q) {
          const int x = EPV * (lane + 64 * q);
          *reinterpret_cast<u32x4*>(row + x) = *reinterpret_cast<const u32x4*>(g + x);
        }
      } else {
        for (int x = lane; x < kGramTile; x += 64) row[x] = t0 + x < a1 ? g[x] : GT(0);
      }
    }
    __syncthreads();
    for (int ks = wave; ks < kGramTile / KS; ks += 4) {
      const u32x4 f0 = *reinterpret_cast<const u32x4*>(frag + ks * KS);
      u32x4 f1 = f0;
      if (two) f1 = *reinterpret_cast<const u32x4*>(frag + 16 * LD + ks * KS);
      if constexpr (H) {
        const f16x8 h0 = __builtin_bit_cast(f16x8, f0), h1 = __builtin_bit_cast(f16x8, f1);
        acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(h0, h0, acc[0], 0, 0, 0);
        if (two) {
          acc[1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(h0, h1, acc[1], 0, 0, 0);
          acc[2] = __builtin_amdgcn_mfma_f32_16x16x32_f16(h1, h1, acc[2], 0, 0, 0);
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float x0 = __uint_as_float(f0[j]), x1 = __uint_as_float(f1[j]);
          acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(x0, x0, acc[0], 0, 0, 0);
          if (two) {
            acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(x0, x1, acc[1], 0, 0, 0);
            acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(x1, x1, acc[2], 0, 0, 0);
          }
        }
      }
    }
  }
  // the four waves in order; thread (j, l) of tile t holds G[4 * (l >> 4) + j][l & 15] of that tile
  __syncthreads();
  float* red = reinterpret_cast<float*>(xs);
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int j = 0; j < 4; ++j) red[((wave * 3 + t) * 4 + j) * 64 + lane] = acc[t][j];
  __syncthreads();
  float* out = partials + (size_t)blockIdx.x * (kMaxSrc * kMaxSrc);
  const int row = 4 * (lane >> 4) + (tid >> 6), col = lane & 15;
  for (int t = 0; t < (two ? 3 : 1); ++t) {
    const int f = t * 256 + tid;
    const float s = ((red[f] + red[768 + f]) + red[2 * 768 + f]) + red[3 * 768 + f];
    out[(row + (t == 2 ? 16 : 0)) * kMaxSrc + col + (t >= 1 ? 16 : 0)] = s;
  }
}

__global__ __launch_bounds__(256) void robust_krum_select_kernel(const float* __restrict__ partials, int nblocks,
                                                                 int W, int F, float* __restrict__ sel,
                                                                 RobustState* __restrict__ state) {
  __shared__ double G[kMaxSrc][kMaxSrc + 1], d2[kMaxSrc][kMaxSrc + 1], score[kMaxSrc];
  const int tid = threadIdx.x;
  for (int q = tid; q < kMaxSrc * kMaxSrc; q += 256) {
    const int i = q >> 5, j = q & 31;
    if (i <= j && j < W) {  // the tiles the Gram kernel wrote
      double a = 0.0;
      for (int b = 0; b < nblocks; ++b) a += (double)partials[(size_t)b * (kMaxSrc * kMaxSrc) + q];
      G[i][j] = G[j][i] = a;
    }
  }
  __syncthreads();
  for (int q = tid; q < kMaxSrc * kMaxSrc; q += 256) {
    const int i = q >> 5, j = q & 31;
    if (i < W && j < W) {
      const double d = G[i][i] + G[j][j] - 2.0 * G[i][j];
      d2[i][j] = __builtin_isfinite(d) ? d : __builtin_inf();
    }
  }
  __syncthreads();
  const double inf = __builtin_inf();
  if (tid < W) {  // score: the W-F-2 nearest others, by rank (ties: lower index), summed in index order
    const int i = tid, keep = W - F - 2;
    double s = 0.0;
    for (int j = 0; j < W; ++j) {
      if (j == i) continue;
      int rank = 0;
      for (int l = 0; l < W; ++l)
        if (l != i && l != j && (d2[i][l] < d2[i][j] || (d2[i][l] == d2[i][j] && l < j))) ++rank;
      if (rank < keep) s += d2[i][j];
    }
    score[i] = __builtin_isfinite(s) ? s : inf;
  }
  __syncthreads();
  if (tid < kMaxSrc) {
    float on = 0.f;
    if (tid < W) {
      int rank = 0;
      for (int l = 0; l < W; ++l)
        if (l != tid && (score[l] < score[tid] || (score[l] == score[tid] && l < tid))) ++rank;
      on = rank < W - F ? 1.f : 0.f;
      if (on != 0.f) state->selected[tid] += 1;
    }
    sel[tid] = on;
  }
}

template <typename GT, bool VEC>
__global__ __launch_bounds__(256) void robust_select_sum_kernel(WireSrcs srcs, const float* __restrict__ sel,
                                                                float* __restrict__ agg, long n, float inv_m,
                                                                float c) {
  const ChunkRange r = chunk_range(0, n, blockIdx.x, n);
  for_chunk<VEC>(
      r,
      [&](long i) {
        float s = 0.f;
        for (int k = 0; k < srcs.n; ++k)
          if (sel[k] != 0.f) s += ld_wire(reinterpret_cast<const GT*>(srcs.p[k]), i);
        agg[i] = (s * inv_m) * c;
      },
      [&](long i) {
        float s[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) s[j] = 0.f;
        for (int k = 0; k < srcs.n; ++k) {
          if (sel[k] == 0.f) continue;  // grid-uniform
          float g[8];
          ld_wire8(reinterpret_cast<const GT*>(srcs.p[k]) + i, g);
#pragma unroll
          for (int j = 0; j < 8; ++j) s[j] += g[j];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) s[j] = (s[j] * inv_m) * c;
        st8(agg + i, s);
      });
}

}  // namespace psx

using namespace psx;

template <typename GT, int NW, bool VEC>
static void rank_launch_kind(int kind, int grid, hipStream_t st, const WireSrcs& sl, float* agg, long n, long off,
                             long cnt, const RankArgs& ra) {
  if (kind == kKindMedian)
    hipLaunchKernelGGL((robust_rank_kernel<GT, NW, kKindMedian, VEC>), dim3(grid), dim3(256), 0, st, sl, agg, n, off,
                       cnt, ra);
  else
    hipLaunchKernelGGL((robust_rank_kernel<GT, NW, kKindTrimmed, VEC>), dim3(grid), dim3(256), 0, st, sl, agg, n, off,
                       cnt, ra);
}

template <typename GT, bool VEC>
static void rank_launch(int kind, int grid, hipStream_t st, const WireSrcs& sl, float* agg, long n, long off, long cnt,
                        const RankArgs& ra) {
  if (sl.n <= 4) rank_launch_kind<GT, 4, VEC>(kind, grid, st, sl, agg, n, off, cnt, ra);
  else if (sl.n <= 8) rank_launch_kind<GT, 8, VEC>(kind, grid, st, sl, agg, n, off, cnt, ra);
  else if (sl.n <= 16) rank_launch_kind<GT, 16, VEC>(kind, grid, st, sl, agg, n, off, cnt, ra);
  else rank_launch_kind<GT, 32, VEC>(kind, grid, st, sl, agg, n, off, cnt, ra);
}

extern "C" {

int psx_robust_gram_slice() { return kGramSlice; }
int psx_robust_state_bytes() { return (int)sizeof(RobustState); }

// agg[off : off + cnt) = c * the coordinate-wise estimate of nsrc gathered wires (host array of nsrc
// <= 32 device pointers, all fp16 or all fp32, >= n elements each; agg fp32 [n], sharing no byte
// with a source). kind 0: trimmed mean without the `trim` smallest and largest values (nsrc > 2 *
// trim), kind 1: median. One launch on `st`. Invalid arguments: an error, nothing launched.
int psx_robust_rank(const void* const* srcs, int nsrc, int grad_fp16, float* agg, long n, long off, long cnt, int kind,
                    int trim, float c, hipStream_t st) {
  if (!agg || n <= 0 || off < 0 || cnt <= 0 || off + cnt > n) return (int)hipErrorInvalidValue;
  if (kind != kKindTrimmed && kind != kKindMedian) return (int)hipErrorInvalidValue;
  if (kind == kKindTrimmed && (trim < 0 || nsrc <= 2 * trim)) return (int)hipErrorInvalidValue;
  WireSrcs sl{};
  bool vec = al16(agg);
  if (!fill_srcs(srcs, nsrc, grad_fp16 ? 2 : 4, n, sl, vec, agg, {agg})) return (int)hipErrorInvalidValue;
  const RankArgs ra{trim, kind == kKindTrimmed ? 1.0f / (float)(nsrc - 2 * trim) : 1.0f, c};
  const int grid = (int)((cnt + kChunk - 1) / kChunk);
  dispatch2(grad_fp16 != 0, vec, [&](auto H, auto V) {
    rank_launch<wire_t<decltype(H)>, decltype(V)::value>(kind, grid, st, sl, agg, n, off, cnt, ra);
  });
  return (int)hipGetLastError();
}

// partials [ceil(n / psx_robust_gram_slice())][32][32] fp32: per workgroup, the upper 16x16 tiles of
// G_ij = <src_i, src_j> over its slice (entries i <= j < nsrc; the rest is not written).
int psx_robust_gram(const void* const* srcs, int nsrc, int grad_fp16, long n, float* partials, hipStream_t st) {
  if (!partials || n <= 0 || n > (long)kGramSlice * 0x7fffffffL) return (int)hipErrorInvalidValue;
  WireSrcs sl{};
  bool vec = true;
  if (!fill_srcs(srcs, nsrc, grad_fp16 ? 2 : 4, n, sl, vec, partials)) return (int)hipErrorInvalidValue;
  const int grid = (int)((n + kGramSlice - 1) / kGramSlice);
  dispatch2(grad_fp16 != 0, vec, [&](auto H, auto V) {
    hipLaunchKernelGGL((robust_gram_kernel<wire_t<decltype(H)>, decltype(V)::value>), dim3(grid), dim3(256), 0, st, sl,
                       n, partials);
  });
  return (int)hipGetLastError();
}

// sel [32] fp32: 1 for the nsrc - byzantine workers multi-Krum selects from the Gram partials, else
// 0; state (psx_robust_state_bytes(), zeroed once by the caller) counts the selections per worker.
int psx_robust_krum_select(const float* partials, int nblocks, int nsrc, int byzantine, float* sel, void* state,
                           hipStream_t st) {
  if (!partials || !sel || !state || nblocks < 1 || nsrc > kMaxSrc || byzantine < 0 || nsrc < 2 * byzantine + 3)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(robust_krum_select_kernel, dim3(1), dim3(256), 0, st, partials, nblocks, nsrc, byzantine, sel,
                     (RobustState*)state);
  return (int)hipGetLastError();
}

// agg = c * fl(1 / m) * the fp32 sum, in source order, of the wires with sel[k] != 0 (m of them).
int psx_robust_select_sum(const void* const* srcs, int nsrc, int grad_fp16, const float* sel, float* agg, long n,
                          int m, float c, hipStream_t st) {
  if (!agg || !sel || n <= 0 || m < 1 || m > nsrc || n > (long)kChunk * 0x7fffffffL) return (int)hipErrorInvalidValue;
  WireSrcs sl{};
  bool vec = al16(agg);
  if (!fill_srcs(srcs, nsrc, grad_fp16 ? 2 : 4, n, sl, vec, agg, {agg})) return (int)hipErrorInvalidValue;
  const int grid = (int)((n + kChunk - 1) / kChunk);
  dispatch2(grad_fp16 != 0, vec, [&](auto H, auto V) {
    hipLaunchKernelGGL((robust_select_sum_kernel<wire_t<decltype(H)>, decltype(V)::value>), dim3(grid), dim3(256), 0,
                       st, sl, sel, agg, n, 1.0f / (float)m, c);
  });
  return (int)hipGetLastError();
}

}  // extern "C"
