// Global-norm gradient clipping and the non-finite guard of the server update (--clip-norm,
// --skip-nonfinite).
//
// The SGD kernels (optim.hip, q8.hip) apply whatever the wires carry. The guard needs one number
// before the first parameter moves: the L2 norm of the fp32 sum of the round's wires over the
// whole trainable prefix. Three launches on one stream, no host synchronisation, over a flat grid
// of one workgroup per chunk of kChunk elements:
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
// A chunk starts at a multiple of kChunk arena elements, so the scalar head of the chunk walk
// (wire.hpp), which lars.hip needs for tensors at arbitrary offsets, is always empty here: a chunk is 8-element groups (one
// 16-byte fp16 load per source, two 16-byte fp32 accesses per lane when every base pointer is
// 16-byte aligned; the same 8 elements with scalar accesses otherwise) and a scalar tail of n % 8
// elements in the last chunk.
#include "wire.hpp"

namespace psx {

// the device state block (mirrored by ops/kernels.py GuardState): the last round's decision and
// the running counters; norm_max / norm_sum cover finite rounds only
struct GuardState {
  double S, norm;
  float coef;
  int skip;
  long long rounds, clipped_rounds, skipped_rounds;
  double norm_last, norm_max, norm_sum;
};

// this workgroup's chunk of the whole arena; it starts at a multiple of kChunk, so its head is
// empty, which the compiler cannot see through chunk_range's clamps
PSX_DEV ChunkRange guard_range(long n) {
  const ChunkRange r = chunk_range(0, n, blockIdx.x, n);
  __builtin_assume(r.ha == r.a0);
  return r;
}

// GT: wire element (fp16 bits or fp32). DENSE: s is already in `stage` (no sources, no rewrite).
// VEC: 16-byte accesses in the body (every base pointer 16-byte aligned).
template <typename GT, bool DENSE, bool VEC>
__global__ __launch_bounds__(256) void guard_norms_kernel(WireSrcs srcs, float* __restrict__ stage, long n,
                                                          double* __restrict__ partials) {
  __shared__ double red[4];
  const ChunkRange r = guard_range(n);
  const int tid = threadIdx.x;
  float ss = 0.f;
  for_chunk<VEC>(
      r,
      [&](long i) {
        float s;
        if constexpr (DENSE) {
          s = stage[i];
        } else {
          s = wire_sum1<GT>(srcs, i);
          stage[i] = s;
        }
        ss = __builtin_fmaf(s, s, ss);
      },
      [&](long i) {
        float s[8];
        if constexpr (DENSE) {
          ld8(stage + i, s);
        } else {
          wire_sum8<GT>(srcs, i, s);
          st8(stage + i, s);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) ss = __builtin_fmaf(s[j], s[j], ss);  // the scalar form's order
      });
  const double d = block_sum_f64((double)ss, red);
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
  const double S = block_sum_f64(acc, red);
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
  sgd_stage_chunk<MOM, VEC>(guard_range(n), p, stage, buf, lr, gs, momentum, wd, first, img);
}

}  // namespace psx

using namespace psx;

static bool guard_args_ok(const void* p, const void* stage, long n, const void* partials, const void* state,
                          float clip_norm) {
  return p && stage && partials && state && n > 0 && n <= (long)kChunk * 0x7fffffffL && clip_norm >= 0.f;
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
  const bool vec = al16(p) && al16(stage) && (!mom || al16(buf)) && al16(img);
  uint16_t* im = (uint16_t*)img;
  dispatch2(mom, vec, [&](auto M, auto V) {
    hipLaunchKernelGGL((guard_apply_kernel<decltype(M)::value, decltype(V)::value>), dim3(nblocks), dim3(256), 0, st, p,
                       (const float*)stage, buf, n, (const GuardState*)gst, lr, gscale, momentum, wd, first, im);
  });
  return (int)hipGetLastError();
}

extern "C" {

int psx_guard_chunk() { return kChunk; }
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
  if (!guard_args_ok(p, stage, n, partials, state, clip_norm)) return (int)hipErrorInvalidValue;
  WireSrcs sl{};
  bool vec = al16(stage);
  if (!fill_srcs(srcs, nsrc, grad_fp16 ? 2 : 4, n, sl, vec, stage)) return (int)hipErrorInvalidValue;
  const int nblocks = (int)((n + kChunk - 1) / kChunk);
  dispatch2(grad_fp16 != 0, vec, [&](auto H, auto V) {
    hipLaunchKernelGGL((guard_norms_kernel<wire_t<decltype(H)>, false, decltype(V)::value>), dim3(nblocks), dim3(256),
                       0, st, sl, stage, n, partials);
  });
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
  const WireSrcs sl{};
  const int nblocks = (int)((n + kChunk - 1) / kChunk);
  if (al16(stage))
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
