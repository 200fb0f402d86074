// Iterative whole-vector robust aggregation of a sync round's W gathered dense wires (--aggregate
// geomed / cclip): an fp32 estimate e of the workers' mean gradient, written as agg = e * c like the
// rules of robust.hip (c = 1 / weight).
//
// g_k is wire k decoded to fp32, k = 0..W-1. d_k(v) = sqrt(sum_i (g_k[i] - v[i])^2); a non-finite
// d_k^2 counts as +inf.
//   geomed : the geometric median by smoothed Weiszfeld steps (RFA, Pillutla et al. 2019;
//            --robust-iters L, --geomed-eps nu). v_0 = 0, so the first distances are the wires' norms.
//            For t = 1..L: w_k = 1 / max(d_k(v_{t-1}), nu), 0 where d_k = +inf; a_k = fl32(w_k / sum_j
//            w_j); v_t = sum_k a_k g_k. e = v_L.
//   cclip  : centred clipping (Karimireddy, He, Jaggi 2021; --cclip-tau tau, --robust-iters L). v_0 is
//            the centre the previous round ended with (zeros before the first round). For t = 1..L:
//            a_k = fl32(min(1, tau / d_k(v_{t-1})) / W) (1/W at d_k = 0, 0 at +inf); b = fl32(1 -
//            sum_k a_k); v_t = b v_{t-1} + sum_k a_k g_k. e = v_L, kept as the next round's centre.
// Every combination is evaluated in fp32 per coordinate: it starts from fl(b v) (or 0) and adds
// fl(a_k g_k) in source order, the product rounded before the add. A wire with a_k == 0 is skipped
// (0 * inf would poison the sum). Weight sums and distances are formed in double, in index order;
// the sum behind b runs over the rounded a_k. All a_k zero (every wire non-finite): e = 0 (geomed),
// e = the old centre (cclip, b = 1), and the round counts as degenerate. No fall-back to the mean.
//
// robust_iter_step_kernel: one streaming pass over the wires, one workgroup per kChunk elements. A
// lane loads its 8 coordinates of all W sources once and keeps them in registers (fp16 wires: 4
// packed registers per source; fp32 wires at NW = 32: two passes of 4 coordinates), forms the new
// centre s[8] from the device-resident a[32], b, and sweeps the registers a second time, adding
// (g_k - s)^2 by fma into one fp32 accumulator per source: the distances to the *new* centre come out
// of the pass that made it, so a round is L + 1 passes over the wires, not 2 L + 1.
//   INIT : no combination; the distances to the starting centre (zero, or the stored one)
//   MID  : the new centre (stored in place, cclip only) and the distances to it
//   LAST : the new centre and agg = c * s; no second sweep, no reduction, nothing held: the plain
//          streaming form, which does not read a wire with a_k == 0 at all
// A lane's fp32 chain per source is its head element, its at most 32 body elements in arena order and
// its tail element. From the cross-lane step on everything is double: the accumulators go through
// LDS, wave w owns the sources k = w, w + 4, ..; lane l adds the four quarters ((x[l] + x[l + 64]) +
// x[l + 128]) + x[l + 192], then the xor shuffle tree; the workgroup writes partials[block][32]. The
// scalar form (chunk tail, unaligned sources) does the same operations in the same order: same bits.
//
// robust_iter_weights_kernel: one workgroup. Partials are summed in double in block order within 32
// segments of ceil(nblocks / 32) consecutive blocks, the segment sums in order; then the definitions
// above; a[32], b and the distances go into the state block with plain stores. The last call of a
// round bumps the counters. No atomics anywhere.
//
// A round: INIT, weights, (MID, weights) x (L - 1), LAST: 2 L + 1 launches on one stream, no host
// synchronisation.
#include "wire.hpp"

#pragma clang fp contract(off)  // a_k g_k is rounded before it is added, in both forms; the squares are explicit fmas

namespace psx {

constexpr int kIterInit = 0, kIterMid = 1, kIterLast = 2;
constexpr int kRuleGeomed = 0, kRuleCclip = 1;

struct IterState {
  float a[kMaxSrc];             // the weights of the next step
  float b;                      // the centre's coefficient of the next step
  float pad;
  double d[kMaxSrc];            // the distances behind them (+inf: non-finite)
  long long rounds;             // completed rounds
  long long degenerate_rounds;  // rounds whose final weights were all zero
  long long clipped[kMaxSrc];   // cclip: rounds with d_k > tau at the last weights step
  double wsum[kMaxSrc];         // geomed: sum over rounds of the final a_k
};

// coordinate c of one source's value registers as fp32
PSX_DEV float iter_widen(const uint32_t* v, int c) {
  const uint32_t w = v[c >> 1];
  return (float)__builtin_bit_cast(_Float16, (uint16_t)((c & 1) ? (w >> 16) : (w & 0xffff)));
}
PSX_DEV float iter_widen(const float* v, int c) { return v[c]; }

// NC consecutive coordinates at arena element i (NC = 8 or 4: vector accesses, every pointer + i
// 16-byte aligned; NC = 1: scalar) of all sources: loaded once, combined into the new centre
// (KIND MID), measured against it into acc
template <typename GT, int NW, bool CENTRE, int KIND, int NC>
PSX_DEV void iter_coords(const WireSrcs& srcs, long i, const IterState* __restrict__ st, float* __restrict__ centre,
                         float (&acc)[NW]) {
  constexpr bool H = sizeof(GT) == 2;
  using V = std::conditional_t<H, uint32_t, float>;
  constexpr int NV = H ? (NC + 1) / 2 : NC;
  static_assert(NC == 1 || (H ? NC == 8 : (NC == 8 || NC == 4)), "iter_coords NC");
  static_assert(KIND == kIterInit || KIND == kIterMid, "iter_coords KIND");
  const int W = srcs.n;
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
    }
  }
  float s[NC];
#pragma unroll
  for (int j = 0; j < NC; ++j) s[j] = 0.f;
  if constexpr (CENTRE) {
    if constexpr (NC == 1) {
      s[0] = centre[i];
    } else {
#pragma unroll
      for (int q = 0; q < NC / 4; ++q) {
        const f32x4 w = *reinterpret_cast<const f32x4*>(centre + i + 4 * q);
#pragma unroll
        for (int j = 0; j < 4; ++j) s[4 * q + j] = w[j];
      }
    }
  }
  if constexpr (KIND == kIterMid) {
    if constexpr (CENTRE) {
      const float b = st->b;
#pragma unroll
      for (int j = 0; j < NC; ++j) s[j] = b * s[j];
    }
#pragma unroll
    for (int k = 0; k < NW; ++k) {
      if (k < W) {
        const float a = st->a[k];
        if (a != 0.f) {  // grid-uniform
#pragma unroll
          for (int j = 0; j < NC; ++j) s[j] = s[j] + a * iter_widen(v[k], j);
        }
      }
    }
    if constexpr (CENTRE) {
      if constexpr (NC == 1) {
        centre[i] = s[0];
      } else {
#pragma unroll
        for (int q = 0; q < NC / 4; ++q)
          *reinterpret_cast<f32x4*>(centre + i + 4 * q) = (f32x4){s[4 * q], s[4 * q + 1], s[4 * q + 2], s[4 * q + 3]};
      }
    }
  }
#pragma unroll
  for (int k = 0; k < NW; ++k) {
    if (k < W) {
#pragma unroll
      for (int j = 0; j < NC; ++j) {
        const float d = iter_widen(v[k], j) - s[j];
        acc[k] = __builtin_fmaf(d, d, acc[k]);
      }
    }
  }
}

// the new centre of 1 or 8 coordinates by the plain streaming form (KIND LAST): same values, same order
template <typename GT, bool CENTRE, int NC>
PSX_DEV void iter_last(const WireSrcs& srcs, long i, const IterState* __restrict__ st, float* __restrict__ centre,
                       float* __restrict__ agg, float c) {
  float s[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) s[j] = 0.f;
  if constexpr (CENTRE) {
    if constexpr (NC == 1) s[0] = centre[i];
    else ld8(centre + i, s);
    const float b = st->b;
#pragma unroll
    for (int j = 0; j < NC; ++j) s[j] = b * s[j];
  }
  for (int k = 0; k < srcs.n; ++k) {
    const float a = st->a[k];
    if (a == 0.f) continue;  // grid-uniform: the wire is not read
    const GT* g = reinterpret_cast<const GT*>(srcs.p[k]);
    if constexpr (NC == 1) {
      s[0] = s[0] + a * ld_wire(g, i);
    } else {
      float x[8];
      ld_wire8(g + i, x);
#pragma unroll
      for (int j = 0; j < 8; ++j) s[j] = s[j] + a * x[j];
    }
  }
  if constexpr (NC == 1) {
    if constexpr (CENTRE) centre[i] = s[0];
    agg[i] = c * s[0];
  } else {
    if constexpr (CENTRE) st8(centre + i, s);
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = c * s[j];
    st8(agg + i, s);
  }
}

// GT: wire element. NW: the register file's source count, >= W (LAST: unused). CENTRE: a centre
// buffer is read and (MID, LAST) rewritten in place. VEC: every pointer 16-byte aligned.
template <typename GT, int NW, bool CENTRE, int KIND, bool VEC>
__global__ __launch_bounds__(256) void robust_iter_step_kernel(WireSrcs srcs, const IterState* __restrict__ st,
                                                               float* __restrict__ centre, float* __restrict__ agg,
                                                               double* __restrict__ partials, long n, float c) {
  const ChunkRange r = chunk_range(0, n, blockIdx.x, n);
  if constexpr (KIND == kIterLast) {
    for_chunk<VEC>(
        r, [&](long i) { iter_last<GT, CENTRE, 1>(srcs, i, st, centre, agg, c); },
        [&](long i) { iter_last<GT, CENTRE, 8>(srcs, i, st, centre, agg, c); });
  } else {
    __shared__ float red[NW][256];
    float acc[NW];
#pragma unroll
    for (int k = 0; k < NW; ++k) acc[k] = 0.f;
    for_chunk<VEC>(
        r, [&](long i) { iter_coords<GT, NW, CENTRE, KIND, 1>(srcs, i, st, centre, acc); },
        [&](long i) {
          if constexpr (sizeof(GT) == 4 && NW == 32) {  // the register budget: 4 coordinates at a time
#pragma unroll 1
            for (int h = 0; h < 2; ++h) iter_coords<GT, NW, CENTRE, KIND, 4>(srcs, i + 4 * h, st, centre, acc);
          } else {
            iter_coords<GT, NW, CENTRE, KIND, 8>(srcs, i, st, centre, acc);
          }
        });
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
#pragma unroll
    for (int k = 0; k < NW; ++k) red[k][tid] = acc[k];
    __syncthreads();
    for (int k = wave; k < srcs.n; k += 4) {
      const double q = (((double)red[k][lane] + (double)red[k][lane + 64]) + (double)red[k][lane + 128]) +
                       (double)red[k][lane + 192];
      const double t = wave_sum_f64(q);
      if (lane == 0) partials[(size_t)blockIdx.x * kMaxSrc + k] = t;
    }
  }
}

constexpr int kWeightSegs = 32;  // segments the partials are summed in: one per 32 threads of the weights kernel

__global__ __launch_bounds__(32 * kWeightSegs) void robust_iter_weights_kernel(const double* __restrict__ partials,
                                                                               int nblocks, int W, int rule,
                                                                               double tau, double nu, int final,
                                                                               IterState* __restrict__ st) {
  __shared__ double seg[kWeightSegs][kMaxSrc], wt[kMaxSrc];
  __shared__ float af[kMaxSrc];
  const int tid = threadIdx.x, k = tid & 31, sub = tid >> 5;
  const double inf = __builtin_inf();
  const int per = (nblocks + kWeightSegs - 1) / kWeightSegs, b1 = min(nblocks, (sub + 1) * per);
  double sum = 0.0;
  if (k < W) {
    int b = sub * per;
    for (; b + 8 <= b1; b += 8) {  // eight loads in flight, added in block order
      double x[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) x[j] = partials[(size_t)(b + j) * kMaxSrc + k];
#pragma unroll
      for (int j = 0; j < 8; ++j) sum += x[j];
    }
    for (; b < b1; ++b) sum += partials[(size_t)b * kMaxSrc + k];
  }
  seg[sub][k] = sum;
  __syncthreads();
  double d = inf;
  if (tid < kMaxSrc) {
    double w = 0.0;
    if (tid < W) {
      double d2 = seg[0][tid];
      for (int s = 1; s < kWeightSegs; ++s) d2 += seg[s][tid];
      if (__builtin_isfinite(d2)) d = __builtin_sqrt(d2);
      if (d != inf) w = rule == kRuleGeomed ? 1.0 / fmax(d, nu) : fmin(1.0, tau / d) / (double)W;
    }
    wt[tid] = w;
  }
  __syncthreads();
  if (tid < kMaxSrc) {
    double w = wt[tid];
    if (rule == kRuleGeomed) {
      double S = 0.0;
      for (int j = 0; j < W; ++j) S += wt[j];
      w = S > 0.0 ? w / S : 0.0;
    }
    const float a = (float)w;
    af[tid] = a;
    st->a[tid] = a;
    st->d[tid] = d;
    if (final && tid < W) {
      if (rule == kRuleGeomed) st->wsum[tid] += (double)a;
      else if (d > tau) st->clipped[tid] += 1;
    }
  }
  __syncthreads();
  if (tid == 0) {
    double S = 0.0;
    bool none = true;
    for (int j = 0; j < W; ++j) {
      S += (double)af[j];
      none = none && af[j] == 0.f;
    }
    st->b = rule == kRuleGeomed ? 0.f : (float)(1.0 - S);
    if (final) {
      st->rounds += 1;
      if (none) st->degenerate_rounds += 1;
    }
  }
}

}  // namespace psx

using namespace psx;

template <typename GT, int NW, bool VEC>
static void iter_launch_kind(int kind, bool has_centre, int grid, hipStream_t st, const WireSrcs& sl,
                             const IterState* state, float* centre, double* partials, long n) {
  auto go = [&](auto C, auto K) {
    hipLaunchKernelGGL((robust_iter_step_kernel<GT, NW, decltype(C)::value, decltype(K)::value, VEC>), dim3(grid),
                       dim3(256), 0, st, sl, state, centre, (float*)nullptr, partials, n, 1.0f);
  };
  if (has_centre && kind == kIterInit) go(std::true_type{}, std::integral_constant<int, kIterInit>{});
  else if (has_centre) go(std::true_type{}, std::integral_constant<int, kIterMid>{});
  else if (kind == kIterInit) go(std::false_type{}, std::integral_constant<int, kIterInit>{});
  else go(std::false_type{}, std::integral_constant<int, kIterMid>{});
}

template <typename GT, bool VEC>
static void iter_launch(int kind, bool has_centre, int grid, hipStream_t st, const WireSrcs& sl, const IterState* state,
                        float* centre, float* agg, double* partials, long n, float c) {
  if (kind == kIterLast) {  // the streaming form holds nothing: one instantiation serves every W
    if (has_centre)
      hipLaunchKernelGGL((robust_iter_step_kernel<GT, 32, true, kIterLast, VEC>), dim3(grid), dim3(256), 0, st, sl,
                         state, centre, agg, partials, n, c);
    else
      hipLaunchKernelGGL((robust_iter_step_kernel<GT, 32, false, kIterLast, VEC>), dim3(grid), dim3(256), 0, st, sl,
                         state, centre, agg, partials, n, c);
  } else if (sl.n <= 4) {
    iter_launch_kind<GT, 4, VEC>(kind, has_centre, grid, st, sl, state, centre, partials, n);
  } else if (sl.n <= 8) {
    iter_launch_kind<GT, 8, VEC>(kind, has_centre, grid, st, sl, state, centre, partials, n);
  } else if (sl.n <= 16) {
    iter_launch_kind<GT, 16, VEC>(kind, has_centre, grid, st, sl, state, centre, partials, n);
  } else {
    iter_launch_kind<GT, 32, VEC>(kind, has_centre, grid, st, sl, state, centre, partials, n);
  }
}

extern "C" {

int psx_robust_iter_state_bytes() { return (int)sizeof(IterState); }

// One pass over nsrc gathered wires (host array of nsrc <= 32 device pointers, all fp16 or all fp32,
// >= n elements each) with the weights a[32], b of `state` (psx_robust_iter_state_bytes()).
//   kind 0 INIT: partials[ceil(n / kChunk)][32] (double) = per workgroup the squared distances of the
//     wires to `centre` (fp32 [n]; null: to zero);
//   kind 1 MID : centre <- b centre + sum_k a_k g_k in place (null: sum_k a_k g_k, not stored), and
//     partials = the squared distances to that new centre;
//   kind 2 LAST: the same new centre, and agg (fp32 [n]) = c * it; partials unused.
// agg and centre share no byte with a source or each other. One launch on `st`. Invalid arguments:
// an error, nothing launched.
int psx_robust_iter_step(const void* const* srcs, int nsrc, int grad_fp16, long n, int kind, float* centre,
                         const void* state, double* partials, float* agg, float c, hipStream_t st) {
  if (!state || n <= 0 || n > (long)kChunk * 0x7fffffffL) return (int)hipErrorInvalidValue;
  if (kind != kIterInit && kind != kIterMid && kind != kIterLast) return (int)hipErrorInvalidValue;
  if (kind == kIterLast ? !agg : !partials) return (int)hipErrorInvalidValue;
  if (kind != kIterLast) agg = nullptr;
  if (agg && centre && ranges_overlap(agg, (size_t)n * 4, centre, (size_t)n * 4)) return (int)hipErrorInvalidValue;
  WireSrcs sl{};
  bool vec = (!agg || al16(agg)) && (!centre || al16(centre));
  if (!fill_srcs(srcs, nsrc, grad_fp16 ? 2 : 4, n, sl, vec, agg)) return (int)hipErrorInvalidValue;
  for (int k = 0; k < nsrc; ++k)
    for (const void* b : {(const void*)agg, (const void*)centre})
      if (b && ranges_overlap(srcs[k], (size_t)n * (grad_fp16 ? 2 : 4), b, (size_t)n * 4))
        return (int)hipErrorInvalidValue;
  const int grid = (int)((n + kChunk - 1) / kChunk);
  dispatch2(grad_fp16 != 0, vec, [&](auto H, auto V) {
    iter_launch<wire_t<decltype(H)>, decltype(V)::value>(kind, centre != nullptr, grid, st, sl,
                                                         (const IterState*)state, centre, agg, partials, n, c);
  });
  return (int)hipGetLastError();
}

// state.a, state.b, state.d from the partials of an INIT or MID pass (nblocks = ceil(n / kChunk)) by
// the rule's definition: rule 0 geomed (nu > 0), rule 1 cclip (tau > 0). final: the last weights step
// of a round bumps the counters of the state block (zeroed once by the caller).
int psx_robust_iter_weights(const double* partials, int nblocks, int nsrc, int rule, double tau, double nu, int final,
                            void* state, hipStream_t st) {
  if (!partials || !state || nblocks < 1 || nsrc < 1 || nsrc > kMaxSrc) return (int)hipErrorInvalidValue;
  if (rule != kRuleGeomed && rule != kRuleCclip) return (int)hipErrorInvalidValue;
  if (rule == kRuleGeomed ? !(nu > 0.0) : !(tau > 0.0)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(robust_iter_weights_kernel, dim3(1), dim3(32 * kWeightSegs), 0, st, partials, nblocks, nsrc, rule, tau, nu,
                     final, (IterState*)state);
  return (int)hipGetLastError();
}

}  // extern "C"
