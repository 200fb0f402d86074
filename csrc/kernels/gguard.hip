// Global-norm gradient clipping and the non-finite guard of the server update (--clip-norm,
// --skip-nonfinite).
//
// The SGD kernels (optim.hip, q8.hip) apply whatever the wires carry. The guard needs one number
// before the first parameter moves: the L2 norm of the fp32 sum of the round's wires over the
// whole trainable prefix. Three launches on one stream, no host synchronisation, over a flat grid
// of one workgroup per chunk of kGuardChunk elements:
//
//   guard_norms  : s = sum_k decode(g_k) in fp32 in source order k = 0..W-1 (exactly the sum of
//                  sgd_apply_multi), written as fp32 to the staging buffer; one double partial of
//                  sum s^2 per workgroup. The dense entry takes s already in the staging buffer
//                  (decoded q8 / top-k payloads, an accumulated loopback round) and only reduces.
//   guard_finish : one workgroup sums the partials and decides the round into the state block:
//                    S = sum s^2; norm = gscale * sqrt(S); skip = !isfinite(S);
//                    coef = skip ? 0 : clip_norm > 0 ? min(1, clip_norm / (norm + 1e-6)) : 1
//                  (torch's clip_grad_norm_ form, rounded to float), and keeps the running counters.
//   guard_apply  : returns at once when skip is set (p, buf and the image are not written at all);
//                  otherwise the shared update tail (sgd_tail.hpp) with gscale * coef (one fp32
//                  multiply), so with coef == 1 the bits are those of sgd_apply_multi. Weight decay
//                  is added after the scaling: it is not clipped, as in torch.
//
// S is not finite when any s is inf / NaN (+inf and -inf of two workers meeting included), or when
// a lane's fp32 partial of squares overflows (a gradient norm above about 1e19): that round is
// skipped too.
//
// Determinism (the project's default mode): no atomics. A lane accumulates its elements serially
// with explicit fma in a fixed element order, partials are double from the cross-lane step on
// (xor shuffle tree over the wave, the four waves summed in order through LDS), and the partials
// are summed with a fixed lane assignment and the same trees. Which element a lane owns depends
// only on the element's position in the arena, never on pointer alignment, so the multi-source
// and the dense entry end in the same bits for the same s.
//
// A chunk starts at a multiple of kGuardChunk arena elements, so the scalar head that lars.hip
// needs for tensors at arbitrary offsets is always empty here: a chunk is 8-element groups (one
// 16-byte fp16 load per source, two 16-byte fp32 accesses per lane when every base pointer is
// 16-byte aligned; the same 8 elements with scalar accesses otherwise) and a scalar tail of n % 8
// elements in the last chunk.
#include "common.hpp"
#include "sgd_tail.hpp"

namespace psx {

constexpr int kGuardChunk = 8192;  // elements per workgroup: 32 body elements per lane
constexpr int kGuardMaxSrc = 32;   // reference server.py:424-426 caps the job at 32 workers

struct GuardSrcs {
  const void* p[kGuardMaxSrc];
  int n;
};

// the device state block (mirrored by ops/kernels.py GuardState): the last round's decision and
// the running counters; norm_max / norm_sum cover finite rounds only
struct GuardState {
  double S, norm;
  float coef;
  int skip;
  long long rounds, clipped_rounds, skipped_rounds;
  double norm_last, norm_max, norm_sum;
};

// arena range [a0, a1) of one chunk: 8-element groups [a0, tb), scalar tail [tb, a1)
struct GuardRange {
  long a0, tb, a1;
};
PSX_DEV GuardRange guard_range(long n) {
  GuardRange r;
  r.a0 = (long)blockIdx.x * kGuardChunk;
  r.a1 = min(r.a0 + kGuardChunk, n);
  r.tb = r.a0 + ((r.a1 - r.a0) & ~7L);
  return r;
}

PSX_DEV float guard_ld(const uint16_t* g, long i) { return (float)__builtin_bit_cast(_Float16, g[i]); }
PSX_DEV float guard_ld(const float* g, long i) { return g[i]; }

PSX_DEV double guard_wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// block-wide sum in double: wave trees, then the four waves in order (every thread gets it)
PSX_DEV double guard_block_sum(double a, double* red) {
  a = guard_wave_sum_f64(a);
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  if (l == 0) red[w] = a;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// GT: wire element (fp16 bits or fp32). DENSE: s is already in `stage` (no sources, no rewrite).
// VEC: 16-byte accesses in the body (every base pointer 16-byte aligned).
template <typename GT, bool DENSE, bool VEC>
__global__ __launch_bounds__(256) void guard_norms_kernel(GuardSrcs srcs, float* __restrict__ stage, long n,
                                                          double* __restrict__ partials) {
  __shared__ double red[4];
  const GuardRange r = guard_range(n);
  const int tid = threadIdx.x;
  float ss = 0.f;
  auto one = [&](long i) {
    float s;
    if constexpr (DENSE) {
      s = stage[i];
    } else {
      s = 0.f;
      for (int k = 0; k < srcs.n; ++k) s += guard_ld(reinterpret_cast<const GT*>(srcs.p[k]), i);
      stage[i] = s;
    }
    ss = __builtin_fmaf(s, s, ss);
  };
  const long ng = (r.tb - r.a0) >> 3;
  for (long q = tid; q < ng; q += 256) {
    const long i = r.a0 + 8 * q;
    if constexpr (VEC) {
      float s[8];
      if constexpr (DENSE) {
        ld8(stage + i, s);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) s[j] = 0.f;
        for (int k = 0; k < srcs.n; ++k) {
          if constexpr (sizeof(GT) == 2) {
            const u32x4 gv = *reinterpret_cast<const u32x4*>(reinterpret_cast<const uint16_t*>(srcs.p[k]) + i);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              s[2 * j] += (float)__builtin_bit_cast(_Float16, (uint16_t)(gv[j] & 0xffff));
              s[2 * j + 1] += (float)__builtin_bit_cast(_Float16, (uint16_t)(gv[j] >> 16));
            }
          } else {
            float g[8];
            ld8(reinterpret_cast<const float*>(srcs.p[k]) + i, g);
#pragma unroll
            for (int j = 0; j < 8; ++j) s[j] += g[j];
          }
        }
        st8(stage + i, s);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) ss = __builtin_fmaf(s[j], s[j], ss);  // the scalar form's order
    } else {
      for (int j = 0; j < 8; ++j) one(i + j);
    }
  }
  if (tid < r.a1 - r.tb) one(r.tb + tid);
  const double d = guard_block_sum((double)ss, red);
  if (tid == 0) partials[blockIdx.x] = d;
}

// one workgroup: partial j on lane j % 256, lane-serial, then the fixed trees; thread 0 decides
// the round and updates the counters with plain stores
__global__ __launch_bounds__(256) void guard_finish_kernel(const double* __restrict__ partials, int nblocks,
                                                           GuardState* __restrict__ state, float gscale,
                                                           float clip_norm) {
  __shared__ double red[4];
  double acc = 0.0;
  for (int j = threadIdx.x; j < nblocks; j += 256) acc += partials[j];
  const double S = guard_block_sum(acc, red);
  if (threadIdx.x != 0) return;
  const bool skip = !__builtin_isfinite(S);
  const double norm = (double)gscale * sqrt(S);
  float coef = 1.f;
  if (skip)
    coef = 0.f;
  else if (clip_norm > 0.f)
    coef = (float)fmin(1.0, (double)clip_norm / (norm + 1e-6));
  state->S = S;
  state->norm = norm;
  state->coef = coef;
  state->skip = skip ? 1 : 0;
  state->rounds += 1;
  state->norm_last = norm;
  if (skip) {
    state->skipped_rounds += 1;
  } else {
    if (coef < 1.f) state->clipped_rounds += 1;
    state->norm_max = fmax(state->norm_max, norm);
    state->norm_sum += norm;
  }
}

template <bool MOM, bool VEC>
__global__ __launch_bounds__(256) void guard_apply_kernel(float* __restrict__ p, const float* __restrict__ stage,
                                                          float* __restrict__ buf, long n,
                                                          const GuardState* __restrict__ state, float lr, float gscale,
                                                          float momentum, float wd, int first,
                                                          uint16_t* __restrict__ img) {
  if (state->skip) return;  // grid-uniform: nothing is written
  const float gs = gscale * state->coef;
  const GuardRange r = guard_range(n);
  const int tid = threadIdx.x;
  auto one = [&](long i) {
    const float pv = p[i];
    const float nv = sgd_tail<MOM>(stage[i], pv, buf + i, lr, gs, momentum, wd, first);
    p[i] = nv;
    if (img) img[i] = f2bf(nv);
  };
  const long ng = (r.tb - r.a0) >> 3;
  for (long q = tid; q < ng; q += 256) {
    const long i = r.a0 + 8 * q;
    if constexpr (VEC) {
      float s[8], pv[8], bv[8];
      ld8(stage + i, s);
      ld8(p + i, pv);
      if (MOM && !first) ld8(buf + i, bv);
#pragma unroll
      for (int j = 0; j < 8; ++j) pv[j] = sgd_tail<MOM>(s[j], pv[j], &bv[j], lr, gs, momentum, wd, first);
      st8(p + i, pv);
      if (MOM) st8(buf + i, bv);
      if (img) {
        const u32x4 o = {pack_bf2(pv[0], pv[1]), pack_bf2(pv[2], pv[3]), pack_bf2(pv[4], pv[5]),
                         pack_bf2(pv[6], pv[7])};
        *reinterpret_cast<u32x4*>(img + i) = o;
      }
    } else {
      for (int j = 0; j < 8; ++j) one(i + j);
    }
  }
  if (tid < r.a1 - r.tb) one(r.tb + tid);
}

}  // namespace psx

using namespace psx;

static bool guard_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static bool guard_args_ok(const void* p, const void* stage, long n, const void* partials, const void* state,
                          float clip_norm) {
  return p && stage && partials && state && n > 0 && n <= (long)kGuardChunk * 0x7fffffffL && clip_norm >= 0.f;
}

// guard_finish + guard_apply, after either norms entry
static int guard_launch_tail(float* p, float* stage, float* buf, long n, int nblocks, double* partials, void* state,
                             float lr, float gscale, float momentum, float wd, float clip_norm, int first, void* img,
                             hipStream_t st) {
  GuardState* gst = (GuardState*)state;
  hipLaunchKernelGGL(guard_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)partials, nblocks, gst, gscale,
                     clip_norm);
  const int rc = (int)hipGetLastError();
  if (rc) return rc;
  const bool mom = buf != nullptr && momentum != 0.f;
  const bool vec = guard_al16(p) && guard_al16(stage) && (!mom || guard_al16(buf)) && guard_al16(img);
  uint16_t* im = (uint16_t*)img;
#define PSX_GA(M, V)                                                                                              \
  hipLaunchKernelGGL((guard_apply_kernel<M, V>), dim3(nblocks), dim3(256), 0, st, p, (const float*)stage, buf, n, \
                     (const GuardState*)gst, lr, gscale, momentum, wd, first, im)
  if (mom && vec) PSX_GA(true, true);
  else if (mom) PSX_GA(true, false);
  else if (vec) PSX_GA(false, true);
  else PSX_GA(false, false);
#undef PSX_GA
  return (int)hipGetLastError();
}

extern "C" {

int psx_guard_chunk() { return kGuardChunk; }
int psx_guard_state_bytes() { return (int)sizeof(GuardState); }

// The guarded update from nsrc gathered gradient wires (host array of nsrc <= 32 device pointers,
// all fp16 or all fp32, >= n elements each): three launches on `st`, no host synchronisation.
//   stage    : fp32 [n], receives the fp32 sum of the sources (must not alias a source)
//   partials : double [ceil(n / psx_guard_chunk())] scratch
//   state    : psx_guard_state_bytes() bytes, zeroed once by the caller; the round's decision and
//              the running counters
//   clip_norm: 0 = no clipping (the non-finite guard alone)
//   buf / first / img: as psx_sgd_apply_multi
int psx_guard_apply_multi(float* p, const void* const* srcs, int nsrc, int grad_fp16, float* stage, float* buf, long n,
                          double* partials, void* state, float lr, float gscale, float momentum, float wd,
                          float clip_norm, int first, void* img, hipStream_t st) {
  if (nsrc < 1 || nsrc > kGuardMaxSrc || !srcs) return (int)hipErrorInvalidValue;
  if (!guard_args_ok(p, stage, n, partials, state, clip_norm)) return (int)hipErrorInvalidValue;
  GuardSrcs sl{};
  sl.n = nsrc;
  bool vec = guard_al16(stage);
  for (int k = 0; k < nsrc; ++k) {
    if (!srcs[k] || srcs[k] == (const void*)stage) return (int)hipErrorInvalidValue;
    sl.p[k] = srcs[k];
    vec = vec && guard_al16(srcs[k]);
  }
  const int nblocks = (int)((n + kGuardChunk - 1) / kGuardChunk);
#define PSX_GN(G, V) \
  hipLaunchKernelGGL((guard_norms_kernel<G, false, V>), dim3(nblocks), dim3(256), 0, st, sl, stage, n, partials)
  if (grad_fp16 && vec) PSX_GN(uint16_t, true);
  else if (grad_fp16) PSX_GN(uint16_t, false);
  else if (vec) PSX_GN(float, true);
  else PSX_GN(float, false);
#undef PSX_GN
  const int rc = (int)hipGetLastError();
  if (rc) return rc;
  return guard_launch_tail(p, stage, buf, n, nblocks, partials, state, lr, gscale, momentum, wd, clip_norm, first, img,
                           st);
}

// The dense entry: `stage` already holds the fp32 gradient sum (q8 / top-k payloads decoded into
// it, or an accumulated round); norms only, no rewrite, then the same finish and apply.
int psx_guard_apply(float* p, float* stage, float* buf, long n, double* partials, void* state, float lr, float gscale,
                    float momentum, float wd, float clip_norm, int first, void* img, hipStream_t st) {
  if (!guard_args_ok(p, stage, n, partials, state, clip_norm)) return (int)hipErrorInvalidValue;
  const GuardSrcs sl{};
  const int nblocks = (int)((n + kGuardChunk - 1) / kGuardChunk);
  if (guard_al16(stage))
    hipLaunchKernelGGL((guard_norms_kernel<float, true, true>), dim3(nblocks), dim3(256), 0, st, sl, stage, n,
                       partials);
  else
    hipLaunchKernelGGL((guard_norms_kernel<float, true, false>), dim3(nblocks), dim3(256), 0, st, sl, stage, n,
                       partials);
  const int rc = (int)hipGetLastError();
  if (rc) return rc;
  return guard_launch_tail(p, stage, buf, n, nblocks, partials, state, lr, gscale, momentum, wd, clip_norm, first, img,
                           st);
}

}  // extern "C"
