// AdamW server update (Loshchilov & Hutter 2019, torch.optim.AdamW's form), --optimizer adamw.
//
// One streaming pass over a range of n contiguous elements:
//   s = sum_k decode(src_k) in fp32 in source order k = 0..W-1 (exactly the sum of
//   sgd_apply_multi), then the shared tail of adamw_tail.hpp on (s, p, m, v); img (optional)
//   receives the bf16 image of p' in the same pass.
// Element-wise: no norm of the gradient, no reduction, no atomics, so any range [lo, hi) of the
// arena is a legal update (gradient buckets of an overlapped round, a shard of the sharded server)
// and the result is bit-reproducible by construction.
//
// Ranges start at arbitrary tensor offsets, so the host picks a scalar head of h < 8 elements after
// which every pointer is 16-byte aligned (possible whenever all buffers share their element phase
// mod 8, as slices [lo:hi] of aligned buffers do). The body then moves 8 elements per lane: one
// 16-byte load per fp16 source (two per fp32 source), two 16-byte accesses each for p, m, v and
// one 16-byte store of the image; the tail is scalar again. Without such an h the element-wise
// form runs. Which element a lane owns never changes the arithmetic: all forms give the same bits.
#include <math.h>

#include "adamw_tail.hpp"
#include "wire.hpp"

namespace psx {

// The two source loops below spell out wire_sum1 / wire_sum8 (wire.hpp): through the helpers both
// kernels allocate two more VGPRs for the same arithmetic.
template <typename GT>
PSX_DEV void adamw_one(float* __restrict__ p, const WireSrcs& srcs, float* __restrict__ m, float* __restrict__ v,
                       size_t i, float gscale, const AdamwScalars& c, uint16_t* __restrict__ img) {
  float s = 0.f;
  for (int k = 0; k < srcs.n; ++k) s += ld_wire(reinterpret_cast<const GT*>(srcs.p[k]), i);
  float mv = m[i], vv = v[i];
  const float nv = adamw_tail(s, p[i], mv, vv, gscale, c);
  p[i] = nv;
  m[i] = mv;
  v[i] = vv;
  if (img) img[i] = f2bf(nv);
}

// element-wise form: any alignment
template <typename GT>
__global__ __launch_bounds__(256) void adamw_apply_kernel(float* __restrict__ p, WireSrcs srcs,
                                                          float* __restrict__ m, float* __restrict__ v, size_t n,
                                                          float gscale, AdamwScalars c, uint16_t* __restrict__ img) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    adamw_one<GT>(p, srcs, m, v, i, gscale, c, img);
}

// vector form: scalar head [0, h), 8-element groups [h, h + 8 * ng), scalar tail up to n; every
// pointer + h is 16-byte aligned (the host's choice of h)
template <typename GT>
__global__ __launch_bounds__(256) void adamw_apply_v8_kernel(float* __restrict__ p, WireSrcs srcs,
                                                             float* __restrict__ m, float* __restrict__ v, size_t n,
                                                             int h, float gscale, AdamwScalars c,
                                                             uint16_t* __restrict__ img) {
  const size_t ng = (n - h) >> 3;
  const size_t tb = h + (ng << 3);
  if (blockIdx.x == 0) {  // head and tail: fewer than 8 elements each, on two different waves
    const int tid = threadIdx.x;
    if (tid < h) adamw_one<GT>(p, srcs, m, v, tid, gscale, c, img);
    if (tid >= 64 && tb + (tid - 64) < n) adamw_one<GT>(p, srcs, m, v, tb + (tid - 64), gscale, c, img);
  }
  for (size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x; q < ng; q += (size_t)gridDim.x * blockDim.x) {
    const size_t i = h + (q << 3);
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
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
    float pv[8], mv[8], vv[8];
    ld8(p + i, pv);
    ld8(m + i, mv);
    ld8(v + i, vv);
#pragma unroll
    for (int j = 0; j < 8; ++j) pv[j] = adamw_tail(s[j], pv[j], mv[j], vv[j], gscale, c);
    st8(p + i, pv);
    st8(m + i, mv);
    st8(v + i, vv);
    if (img) st_bf8(img + i, pv);
  }
}

}  // namespace psx

using namespace psx;

// the eight fp32 scalars of one update, each computed in double and rounded once
static void adamw_scalars(double lr, double beta1, double beta2, double eps, double wd, long t, float out[8]) {
  out[0] = (float)(lr / (1.0 - pow(beta1, (double)t)));
  out[1] = (float)beta1;
  out[2] = (float)(1.0 - beta1);
  out[3] = (float)beta2;
  out[4] = (float)(1.0 - beta2);
  out[5] = (float)(1.0 / sqrt(1.0 - pow(beta2, (double)t)));
  out[6] = (float)eps;
  out[7] = (float)(1.0 - lr * wd);
}

extern "C" {

// out: step_size, beta1, 1 - beta1, beta2, 1 - beta2, rsqrt_bc2, eps, decay — exactly the values
// psx_adamw_apply_multi hands its kernel for the same arguments.
int psx_adamw_scalars(double lr, double beta1, double beta2, double eps, double wd, long t, float* out) {
  if (!out || t < 1) return (int)hipErrorInvalidValue;
  adamw_scalars(lr, beta1, beta2, eps, wd, t, out);
  return 0;
}

// The AdamW update of n contiguous elements from nsrc gradient wires (host array of 1..32 device
// pointers, all fp16 or all fp32, >= n elements each), update number t >= 1:
//   m, v : fp32 [n] first and second moment, read and replaced
//   img  : optional bf16 [n] image of the updated parameters
// One fp32 source is the dense entry (decoded q8 / top-k payloads, an accumulated round).
// One launch on `st`, no host synchronisation.
int psx_adamw_apply_multi(float* p, const void* const* srcs, int nsrc, int grad_fp16, float* m, float* v, long n,
                          double lr, float gscale, double beta1, double beta2, double eps, double wd, long t,
                          void* img, hipStream_t st) {
  if (!p || !m || !v || n <= 0 || t < 1) return (int)hipErrorInvalidValue;
  const size_t esz = grad_fp16 ? 2 : 4, nb = (size_t)n * 4;
  if (ranges_overlap(p, nb, m, nb) || ranges_overlap(p, nb, v, nb) || ranges_overlap(m, nb, v, nb))
    return (int)hipErrorInvalidValue;
  WireSrcs sl{};
  bool al = true;  // unused: the head search below decides the vector form
  if (!fill_srcs(srcs, nsrc, esz, n, sl, al, nullptr, {p, m, v})) return (int)hipErrorInvalidValue;
  float sc[8];
  adamw_scalars(lr, beta1, beta2, eps, wd, t, sc);
  const AdamwScalars c{sc[0], sc[1], sc[2], sc[3], sc[4], sc[5], sc[6], sc[7]};
  uint16_t* im = (uint16_t*)img;
  // head h < 8 after which every pointer is 16-byte aligned (-1: none)
  int head = -1;
  for (int h = 0; h < 8 && head < 0; ++h) {
    bool ok = ((uintptr_t)(p + h) | (uintptr_t)(m + h) | (uintptr_t)(v + h) | (uintptr_t)(im ? im + h : nullptr)) % 16 == 0;
    for (int k = 0; k < nsrc && ok; ++k) ok = ((uintptr_t)srcs[k] + h * esz) % 16 == 0;
    if (ok) head = h;
  }
  if (head >= 0 && n - head >= 8) {
    const int grid = stream_grid((size_t)(n - head) >> 3);
    if (grad_fp16)
      hipLaunchKernelGGL(adamw_apply_v8_kernel<uint16_t>, dim3(grid), dim3(256), 0, st, p, sl, m, v, (size_t)n, head,
                         gscale, c, im);
    else
      hipLaunchKernelGGL(adamw_apply_v8_kernel<float>, dim3(grid), dim3(256), 0, st, p, sl, m, v, (size_t)n, head,
                         gscale, c, im);
    return (int)hipGetLastError();
  }
  const int grid = stream_grid((size_t)n);
  if (grad_fp16)
    hipLaunchKernelGGL(adamw_apply_kernel<uint16_t>, dim3(grid), dim3(256), 0, st, p, sl, m, v, (size_t)n, gscale, c,
                       im);
  else
    hipLaunchKernelGGL(adamw_apply_kernel<float>, dim3(grid), dim3(256), 0, st, p, sl, m, v, (size_t)n, gscale, c, im);
  return (int)hipGetLastError();
}

}  // extern "C"
