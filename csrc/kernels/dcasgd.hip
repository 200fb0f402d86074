// Delay-compensated asynchronous SGD (DC-ASGD: Zheng et al., ICML 2017), --dc-lambda.
//
// An async push arrives with a gradient g taken at the parameters the worker last fetched
// (bak), while the server has moved on to w. DC-ASGD corrects g to first order with the diagonal
// outer-product approximation of the Hessian:
//
//   constant:  lam = dc_lambda
//   adaptive:  ms  = decay * ms + (1 - decay) * g*g          (one fp32 per parameter, zero at start)
//              lam = dc_lambda / sqrt(ms + eps)
//   g~ = g + lam * g * g * (w - bak)
//   w, momentum buffer, bf16 image <- sgd_tail<MOM>(g~, w, ..., lr, gscale = weight, ...)
//
// Two kernels:
//   dc_apply      : the whole update in one pass over the arena: reads g (2 or 4 B), w, bak
//                   [, ms][, buf], writes w [, ms][, buf][, bf16 image]. 8 elements per lane with
//                   16-byte accesses on every stream when every base pointer is 16-byte aligned
//                   (scalar accesses otherwise), n arbitrary: the n % 8 tail is taken by the first
//                   lanes of workgroup 0, as sgd_apply_h8_kernel does. bak == nullptr: the push of
//                   a worker without a backup, g~ = g (adaptive: ms is still updated).
//   dc_fetch_copy : the fetch that leaves the backup: dst[0:n_arena] = src and
//                   bak[0:n_params] = src[0:n_params] from one read of the arena (12 B per
//                   parameter where two device copies move 16). dst == nullptr: backup only.
//
// No atomics, no LDS, no host synchronisation: both are plain stream work (graph-capturable).
// The compensation is one device function (dc_grad) shared by every instantiation and by the
// vector and scalar forms, so every path rounds the same way.
#include "wire.hpp"

namespace psx {

// The compensated gradient of one element, fp32, in the order of the header. msp: this element's
// mean-square slot (read, then written; ADAPT only). comp = false: no backup, g~ = g.
template <bool ADAPT>
PSX_DEV float dc_grad(float g, float w, float bak, bool comp, float lam, float decay, float eps, float* msp) {
  if (ADAPT) {
    // the fma spelled out: left to contraction, the 8-per-lane form fused decay * ms into the add
    // and the scalar form (a misaligned slice, the n % 8 tail) added two rounded products
    const float m = __builtin_fmaf(decay, *msp, (1.f - decay) * g * g);
    *msp = m;
    lam = lam / sqrtf(m + eps);
  }
  return comp ? g + lam * g * g * (w - bak) : g;
}

template <typename GT, bool MOM, bool ADAPT>
__global__ __launch_bounds__(256) void dc_apply_kernel(float* __restrict__ p, const GT* __restrict__ g,
                                                       const float* __restrict__ bak, float* __restrict__ ms,
                                                       float* __restrict__ buf, size_t n, float lr, float gscale,
                                                       float momentum, float wd, float lam, float decay, float eps,
                                                       int first, uint16_t* __restrict__ img, int vec) {
  const bool comp = bak != nullptr;
  auto one = [&](size_t i) {
    const float pv = p[i];
    const float gc = dc_grad<ADAPT>(ld_wire(g, i), pv, comp ? bak[i] : pv, comp, lam, decay, eps, ms + i);
    const float nv = sgd_tail<MOM>(gc, pv, buf + i, lr, gscale, momentum, wd, first);
    p[i] = nv;
    if (img) img[i] = f2bf(nv);
  };
  const size_t tid = blockIdx.x * (size_t)blockDim.x + threadIdx.x, nthr = (size_t)gridDim.x * blockDim.x;
  if (!vec) {  // a base pointer off the 16-byte grid: element by element
    for (size_t i = tid; i < n; i += nthr) one(i);
    return;
  }
  const size_t n8 = n >> 3;
  if (blockIdx.x == 0 && threadIdx.x < (n & 7)) one((n8 << 3) + threadIdx.x);  // tail (n % 8 elements)
  for (size_t q = tid; q < n8; q += nthr) {
    const size_t i = q << 3;
    float gv[8], pv[8], bk[8], mv[8], bv[8];
    ld_wire8(g + i, gv);
    ld8(p + i, pv);
    if (comp) ld8(bak + i, bk);
    if (ADAPT) ld8(ms + i, mv);
    if (MOM && !first) ld8(buf + i, bv);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float gc = dc_grad<ADAPT>(gv[j], pv[j], comp ? bk[j] : pv[j], comp, lam, decay, eps, &mv[j]);
      pv[j] = sgd_tail<MOM>(gc, pv[j], &bv[j], lr, gscale, momentum, wd, first);
    }
    st8(p + i, pv);
    if (ADAPT) st8(ms + i, mv);
    if (MOM) st8(buf + i, bv);
    if (img) st_bf8(img + i, pv);
  }
}

// dst[0:n] = src (dst nullable), bak[0:nb] = src[0:nb], nb <= n: 4 elements per lane when aligned
__global__ __launch_bounds__(256) void dc_fetch_copy_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                            float* __restrict__ bak, size_t n, size_t nb, int vec) {
  const size_t tid = blockIdx.x * (size_t)blockDim.x + threadIdx.x, nthr = (size_t)gridDim.x * blockDim.x;
  auto one = [&](size_t i) {
    const float v = src[i];
    if (dst) dst[i] = v;
    if (i < nb) bak[i] = v;
  };
  if (!vec) {
    for (size_t i = tid; i < n; i += nthr) one(i);
    return;
  }
  const size_t n4 = n >> 2;
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) one((n4 << 2) + threadIdx.x);  // tail (n % 4 elements)
  for (size_t q = tid; q < n4; q += nthr) {
    const size_t i = q << 2;
    const f32x4 v = *reinterpret_cast<const f32x4*>(src + i);
    if (dst) *reinterpret_cast<f32x4*>(dst + i) = v;
    if (i + 4 <= nb) {
      *reinterpret_cast<f32x4*>(bak + i) = v;
    } else {  // the group that straddles the end of the backup
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (i + j < nb) bak[i + j] = v[j];
    }
  }
}

}  // namespace psx

using namespace psx;

// memory-bound: at most 2048 workgroups, grid-stride the rest
static int dc_grid(size_t work) { return stream_grid(work, 2048); }

extern "C" {

// The DC-ASGD server update of one push (see the header). g: fp16 (grad_fp16) or fp32, n
// elements; bak: the pushing worker's backup (nullptr: none, uncompensated); ms: the mean-square
// buffer (nullptr: the constant form, lam used as is; else lam / sqrt(ms + eps), ms updated);
// buf / first / img as psx_sgd_apply.
int psx_dc_apply(float* p, const void* g, const float* bak, float* ms, float* buf, long n, float lr, float gscale,
                 float momentum, float wd, float lam, float decay, float eps, int first, int grad_fp16, void* img,
                 hipStream_t st) {
  if (!p || !g || n <= 0) return (int)hipErrorInvalidValue;
  const bool mom = buf != nullptr && momentum != 0.f;
  const bool adapt = ms != nullptr;
  const int vec = al16(p) && al16(g) && al16(bak) && al16(ms) && (!mom || al16(buf)) && al16(img);
  const int grid = dc_grid(vec ? ((size_t)n + 7) / 8 : (size_t)n);
  uint16_t* im = (uint16_t*)img;
#define PSX_DC(G, M, A)                                                                                          \
  hipLaunchKernelGGL((dc_apply_kernel<G, M, A>), dim3(grid), dim3(256), 0, st, p, (const G*)g, bak, ms, buf,     \
                     (size_t)n, lr, gscale, momentum, wd, lam, decay, eps, first, im, vec)
  if (grad_fp16) {
    if (mom && adapt) PSX_DC(uint16_t, true, true);
    else if (mom) PSX_DC(uint16_t, true, false);
    else if (adapt) PSX_DC(uint16_t, false, true);
    else PSX_DC(uint16_t, false, false);
  } else {
    if (mom && adapt) PSX_DC(float, true, true);
    else if (mom) PSX_DC(float, true, false);
    else if (adapt) PSX_DC(float, false, true);
    else PSX_DC(float, false, false);
  }
#undef PSX_DC
  return (int)hipGetLastError();
}

// dst[0:n_arena] = src (dst == nullptr: skipped) and bak[0:n_params] = src[0:n_params].
int psx_dc_fetch_copy(const float* src, float* dst, float* bak, long n_arena, long n_params, hipStream_t st) {
  if (!src || !bak || n_params < 0 || n_params > n_arena) return (int)hipErrorInvalidValue;
  const size_t n = dst ? (size_t)n_arena : (size_t)n_params;  // backup only: nothing to read past it
  if (!n) return 0;
  const int vec = al16(src) && al16(dst) && al16(bak);
  hipLaunchKernelGGL(dc_fetch_copy_kernel, dim3(dc_grid(vec ? (n + 3) / 4 : n)), dim3(256), 0, st, src, dst, bak, n,
                     (size_t)n_params, vec);
  return (int)hipGetLastError();
}

}  // extern "C"
