// LAMB server update (You et al. 2020), --optimizer lamb: the AdamW moments under the LARS
// segment table. Per tensor of the trainable prefix, for update number t:
//   g = gscale * s;  m' = beta1 m + (1 - beta1) g;  v' = beta2 v + (1 - beta2) g g
//   r = (m' / (1 - beta1^t)) / (sqrt(v') / sqrt(1 - beta2^t) + eps)
//   u = r + wd * w,  phi = |w| / |u| (1 if either norm is 0)      tensors with ndim > 1
//   u = r,           phi = 1                                       1-D tensors (the LARS convention)
//   p' = p - lr * phi * u
// No clamp on |w| and no global gradient normalisation (the paper's optional phi(z) = min(max(z,
// lo), hi) and pre-normalisation are left out).
//
// Two launches over the flat grid of (tensor, chunk of kChunk elements) workgroups of
// lars_seg.hpp, on the caller's stream, no host synchronisation:
//
//   lamb_moments : s = sum_k decode(g_k) in fp32 in source order k = 0..W-1 (exactly the sum of
//                  sgd_apply_multi, lars_norms and adamw_apply); reads p, m, v, writes m', v' in
//                  place and u as fp32 into the staging buffer; one {sum u^2, sum w^2} double
//                  partial per workgroup. The dense entry takes s from the staging buffer itself
//                  (q8 / top-k payloads decoded by their own kernels, an accumulated round) and
//                  overwrites it with u element by element. 2W + 24 bytes per parameter (fp16).
//   lamb_apply   : every workgroup re-derives its tensor's phi from the tensor's partials, stores
//                  it into the ratio table, and applies p' = p - (lr * phi) * u; the optional bf16
//                  image is written in the same pass. 12 (+2) bytes per parameter.
//
// The per-element arithmetic is lamb_tail.hpp (the moments are adamw_tail.hpp's, bit for bit).
// Determinism and layout as lars.hip: no atomics, lane-serial fp32 fma accumulation in a fixed
// element order, double from the cross-lane step on, fixed trees; scalar head to the next
// multiple of 8 arena elements, 8 elements per lane in the body (16-byte accesses when every
// base pointer is 16-byte aligned, the same 8 elements with scalar accesses otherwise), scalar
// tail. The multi-source and the dense entry, every alignment and image on or off end in the
// same bits.
#include <math.h>

#include "lamb_tail.hpp"
#include "lars_seg.hpp"

namespace psx {

// GT: wire element (fp16 bits or fp32). DENSE: s is already in `stage` (no sources).
// VEC: 16-byte accesses in the body (every base pointer 16-byte aligned).
template <typename GT, bool DENSE, bool VEC>
__global__ __launch_bounds__(256) void lamb_moments_kernel(const float* __restrict__ p, WireSrcs srcs,
                                                           float* __restrict__ stage, float* __restrict__ m,
                                                           float* __restrict__ v, long n,
                                                           const LarsSeg* __restrict__ table, int ntensors,
                                                           int nblocks, double* __restrict__ partials, float gscale,
                                                           float wd, AdamwScalars c) {
  __shared__ int sh_t;
  __shared__ double red[2][4];
  const int t = lars_find(table, ntensors, nblocks, &sh_t);
  if (t < 0) return;  // block-uniform
  const LarsSeg seg = table[t];
  const ChunkRange r = chunk_range(seg.offset, seg.numel, blockIdx.x - seg.first_block, n);
  const int tid = threadIdx.x;
  const bool adapt = seg.adapt != 0;  // block-uniform
  float uu = 0.f, ww = 0.f;
  // one element: u from (s, w, m, v), the moments replaced, both sums advanced
  auto tail = [&](float s, float w, float& mv, float& vv) {
    const float u = lamb_update(s, w, mv, vv, gscale, wd, adapt, c);
    uu = __builtin_fmaf(u, u, uu);
    ww = __builtin_fmaf(w, w, ww);
    return u;
  };
  for_chunk<VEC>(
      r,
      [&](long i) {
        float s;
        if constexpr (DENSE) s = stage[i];
        else s = wire_sum1<GT>(srcs, i);
        float mv = m[i], vv = v[i];
        stage[i] = tail(s, p[i], mv, vv);
        m[i] = mv;
        v[i] = vv;
      },
      [&](long i) {
        float s[8], w[8], mv[8], vv[8];
        if constexpr (DENSE) ld8(stage + i, s);
        else wire_sum8<GT>(srcs, i, s);
        ld8(p + i, w);
        ld8(m + i, mv);
        ld8(v + i, vv);
#pragma unroll
        for (int j = 0; j < 8; ++j) s[j] = tail(s[j], w[j], mv[j], vv[j]);  // the scalar form's order
        st8(stage + i, s);
        st8(m + i, mv);
        st8(v + i, vv);
      });
  double duu = (double)uu, dww = (double)ww;
  block_sum2_f64(duu, dww, red);
  if (tid == 0) {
    partials[2 * (long)blockIdx.x] = duu;
    partials[2 * (long)blockIdx.x + 1] = dww;
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void lamb_apply_kernel(float* __restrict__ p, const float* __restrict__ stage,
                                                         long n, const LarsSeg* __restrict__ table, int ntensors,
                                                         int nblocks, const double* __restrict__ partials,
                                                         float* __restrict__ ratios, float lr,
                                                         uint16_t* __restrict__ img) {
  __shared__ int sh_t;
  __shared__ double red[2][4];
  const int t = lars_find(table, ntensors, nblocks, &sh_t);
  if (t < 0) return;  // block-uniform
  const LarsSeg seg = table[t];
  const int chunk = blockIdx.x - seg.first_block;
  const ChunkRange r = chunk_range(seg.offset, seg.numel, chunk, n);
  const int tid = threadIdx.x;
  float phi = 1.f;
  if (seg.adapt) {  // block-uniform
    double uu, ww;  // the tensor's partials through the fixed trees (lars_seg.hpp)
    lars_tensor_sum2(seg, partials, uu, ww, red);
    const double un = sqrt(uu), wn = sqrt(ww);
    if (wn > 0.0 && un > 0.0) phi = (float)(wn / un);
  }
  if (chunk == 0 && tid == 0) ratios[t] = phi;
  const float step = lr * phi;
  for_chunk<VEC>(
      r,
      [&](long i) {
        const float nv = lamb_step(p[i], stage[i], step);
        p[i] = nv;
        if (img) img[i] = f2bf(nv);
      },
      [&](long i) {
        float u[8], pv[8];
        ld8(stage + i, u);
        ld8(p + i, pv);
#pragma unroll
        for (int j = 0; j < 8; ++j) pv[j] = lamb_step(pv[j], u[j], step);
        st8(p + i, pv);
        if (img) st_bf8(img + i, pv);
      });
}

}  // namespace psx

using namespace psx;

extern "C" int psx_adamw_scalars(double lr, double beta1, double beta2, double eps, double wd, long t, float* out);

// the arguments both entries share; the four fp32 [n] buffers must be pairwise disjoint
static bool lamb_args_ok(const void* p, const void* stage, const void* m, const void* v, long n, const void* table,
                         int ntensors, int nblocks, const void* partials, const void* ratios, long t) {
  if (!p || !stage || !m || !v || !table || !partials || !ratios || n <= 0 || ntensors <= 0 || nblocks <= 0 || t < 1)
    return false;
  const void* b[4] = {p, stage, m, v};
  const size_t nb = (size_t)n * 4;
  for (int i = 0; i < 4; ++i)
    for (int j = i + 1; j < 4; ++j)
      if (ranges_overlap(b[i], nb, b[j], nb)) return false;
  return true;
}

// the bias-correction scalars: psx_adamw_scalars' computation with lr = 1, wd = 0 (lamb_tail.hpp)
static int lamb_scalars(double beta1, double beta2, double eps, long t, AdamwScalars& c) {
  float sc[8];
  const int rc = psx_adamw_scalars(1.0, beta1, beta2, eps, 0.0, t, sc);
  c = AdamwScalars{sc[0], sc[1], sc[2], sc[3], sc[4], sc[5], sc[6], sc[7]};
  return rc;
}

static int lamb_launch_apply(float* p, float* stage, long n, const void* table, int ntensors, int nblocks,
                             double* partials, float* ratios, float lr, void* img, hipStream_t st) {
  const LarsSeg* tb = (const LarsSeg*)table;
  uint16_t* im = (uint16_t*)img;
  if (al16(p) && al16(stage) && al16(img))
    hipLaunchKernelGGL((lamb_apply_kernel<true>), dim3(nblocks), dim3(256), 0, st, p, (const float*)stage, n, tb,
                       ntensors, nblocks, (const double*)partials, ratios, lr, im);
  else
    hipLaunchKernelGGL((lamb_apply_kernel<false>), dim3(nblocks), dim3(256), 0, st, p, (const float*)stage, n, tb,
                       ntensors, nblocks, (const double*)partials, ratios, lr, im);
  return (int)hipGetLastError();
}

extern "C" {

// The LAMB update, number t >= 1, from nsrc gathered gradient wires (host array of 1..32 device
// pointers, all fp16 or all fp32, >= n elements each): two launches on `st`, no host
// synchronisation.
//   stage    : fp32 [n], receives u (must not alias a source)
//   m, v     : fp32 [n] first and second moment, read and replaced
//   table, ntensors, nblocks, partials, ratios : as psx_lars_apply_multi; ratios receives phi
//   img      : optional bf16 [n] image of the updated parameters
// A source overlapping p, m or v is refused, as are p, stage, m, v overlapping one another.
int psx_lamb_apply_multi(float* p, const void* const* srcs, int nsrc, int grad_fp16, float* stage, float* m, float* v,
                         long n, const void* table, int ntensors, int nblocks, double* partials, float* ratios,
                         float lr, float gscale, float wd, double beta1, double beta2, double eps, long t, void* img,
                         hipStream_t st) {
  if (!lamb_args_ok(p, stage, m, v, n, table, ntensors, nblocks, partials, ratios, t)) return (int)hipErrorInvalidValue;
  WireSrcs sl{};
  bool vec = al16(p) && al16(stage) && al16(m) && al16(v);
  if (!fill_srcs(srcs, nsrc, grad_fp16 ? 2 : 4, n, sl, vec, stage, {p, m, v})) return (int)hipErrorInvalidValue;
  AdamwScalars c;
  if (lamb_scalars(beta1, beta2, eps, t, c)) return (int)hipErrorInvalidValue;
  const LarsSeg* tb = (const LarsSeg*)table;
  dispatch2(grad_fp16 != 0, vec, [&](auto H, auto V) {
    hipLaunchKernelGGL((lamb_moments_kernel<wire_t<decltype(H)>, false, decltype(V)::value>), dim3(nblocks), dim3(256),
                       0, st, (const float*)p, sl, stage, m, v, n, tb, ntensors, nblocks, partials, gscale, wd, c);
  });
  const int rc = (int)hipGetLastError();
  if (rc) return rc;
  return lamb_launch_apply(p, stage, n, table, ntensors, nblocks, partials, ratios, lr, img, st);
}

// The dense entry: `stage` already holds the fp32 gradient sum (q8 / top-k payloads decoded into
// it, or an accumulated round) and is overwritten with u; then the same apply.
int psx_lamb_apply(float* p, float* stage, float* m, float* v, long n, const void* table, int ntensors, int nblocks,
                   double* partials, float* ratios, float lr, float gscale, float wd, double beta1, double beta2,
                   double eps, long t, void* img, hipStream_t st) {
  if (!lamb_args_ok(p, stage, m, v, n, table, ntensors, nblocks, partials, ratios, t)) return (int)hipErrorInvalidValue;
  AdamwScalars c;
  if (lamb_scalars(beta1, beta2, eps, t, c)) return (int)hipErrorInvalidValue;
  const WireSrcs sl{};
  const LarsSeg* tb = (const LarsSeg*)table;
  if (al16(p) && al16(stage) && al16(m) && al16(v))
    hipLaunchKernelGGL((lamb_moments_kernel<float, true, true>), dim3(nblocks), dim3(256), 0, st, (const float*)p, sl,
                       stage, m, v, n, tb, ntensors, nblocks, partials, gscale, wd, c);
  else
    hipLaunchKernelGGL((lamb_moments_kernel<float, true, false>), dim3(nblocks), dim3(256), 0, st, (const float*)p, sl,
                       stage, m, v, n, tb, ntensors, nblocks, partials, gscale, wd, c);
  const int rc = (int)hipGetLastError();
  if (rc) return rc;
  return lamb_launch_apply(p, stage, n, table, ntensors, nblocks, partials, ratios, lr, img, st);
}

}  // extern "C"
