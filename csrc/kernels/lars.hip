// Layer-wise adaptive server update (LARS: You, Gitman, Ginsburg 2017), --optimizer lars.
//
// The SGD kernels (optim.hip, q8.hip) see the trainable prefix of the arena as one anonymous run
// of floats. LARS scales every tensor's update by a trust ratio of two norms, so this file carries
// the tensor boundaries of models/layout.py to the device (LarsSeg, one record per trainable
// tensor; lars_seg.hpp, shared with lamb.hip) and reduces per tensor, in two launches over one
// flat grid of (tensor, chunk of kChunk elements) workgroups:
//
//   lars_norms : s = sum_k decode(g_k) in fp32 in source order k = 0..W-1 (exactly the sum of
//                sgd_apply_multi), written as fp32 to the staging buffer; one {sum s^2, sum w^2}
//                partial per workgroup. The dense entry takes s already in the staging buffer
//                (q8 / top-k payloads decoded by their own kernels) and only reduces.
//   lars_apply : every workgroup re-derives its tensor's ratio from the tensor's partials,
//                  lambda = trust * |w| / (gscale * |s| + wd * |w| + eps)   (1 if |w| or |s| is 0,
//                  and for 1-D tensors, which also take no weight decay),
//                and applies the shared update tail (sgd_tail.hpp) with gscale and wd scaled by
//                lambda: d = lambda * (gscale * s + wd * w); momentum; p -= lr * v; bf16 image.
//
// Determinism (the project's default mode): no atomics. A lane accumulates its elements serially
// with explicit fma in a fixed element order, partials are double from the cross-lane step on
// (xor shuffle tree over the wave, the four waves summed in order through LDS), and the
// partials of a tensor are summed with a fixed lane assignment and the same trees. Which element
// a lane owns depends only on the chunk's position in the arena, never on pointer alignment, so
// the multi-source and the dense entry end in the same bits for the same s.
//
// Tensor offsets are arbitrary (a 100-element bias, a 1728-element stem), so a chunk starts at any
// element: its head up to the next multiple of 8 arena elements and its tail are scalar accesses,
// the body is 8 elements per lane (one 16-byte fp16 load per source, two 16-byte fp32 accesses) when
// every base pointer is 16-byte aligned, and the same 8 elements with scalar accesses otherwise.
#include "lars_seg.hpp"

namespace psx {

// GT: wire element (fp16 bits or fp32). DENSE: s is already in `stage` (no sources, no rewrite).
// VEC: 16-byte accesses in the body (every base pointer 16-byte aligned).
template <typename GT, bool DENSE, bool VEC>
__global__ __launch_bounds__(256) void lars_norms_kernel(const float* __restrict__ p, WireSrcs srcs,
                                                         float* __restrict__ stage, long n,
                                                         const LarsSeg* __restrict__ table, int ntensors, int nblocks,
                                                         double* __restrict__ partials) {
  __shared__ int sh_t;
  __shared__ double red[2][4];
  const int t = lars_find(table, ntensors, nblocks, &sh_t);
  if (t < 0) return;  // block-uniform
  const LarsSeg seg = table[t];
  const ChunkRange r = chunk_range(seg.offset, seg.numel, blockIdx.x - seg.first_block, n);
  const int tid = threadIdx.x;
  float ss = 0.f, ww = 0.f;
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
        const float w = p[i];
        ss = __builtin_fmaf(s, s, ss);
        ww = __builtin_fmaf(w, w, ww);
      },
      [&](long i) {
        float s[8], w[8];
        if constexpr (DENSE) {
          ld8(stage + i, s);
        } else {
          wire_sum8<GT>(srcs, i, s);
          st8(stage + i, s);
        }
        ld8(p + i, w);
#pragma unroll
        for (int j = 0; j < 8; ++j) {  // the scalar form's order: element by element
          ss = __builtin_fmaf(s[j], s[j], ss);
          ww = __builtin_fmaf(w[j], w[j], ww);
        }
      });
  double dss = (double)ss, dww = (double)ww;
  block_sum2_f64(dss, dww, red);
  if (tid == 0) {
    partials[2 * (long)blockIdx.x] = dss;
    partials[2 * (long)blockIdx.x + 1] = dww;
  }
}

template <bool MOM, bool VEC>
__global__ __launch_bounds__(256) void lars_apply_kernel(float* __restrict__ p, const float* __restrict__ stage,
                                                         float* __restrict__ buf, long n,
                                                         const LarsSeg* __restrict__ table, int ntensors, int nblocks,
                                                         const double* __restrict__ partials,
                                                         float* __restrict__ ratios, float lr, float gscale,
                                                         float momentum, float wd, float trust, float eps, int first,
                                                         uint16_t* __restrict__ img) {
  __shared__ int sh_t;
  __shared__ double red[2][4];
  const int t = lars_find(table, ntensors, nblocks, &sh_t);
  if (t < 0) return;  // block-uniform
  const LarsSeg seg = table[t];
  const int chunk = blockIdx.x - seg.first_block;
  const ChunkRange r = chunk_range(seg.offset, seg.numel, chunk, n);
  const int tid = threadIdx.x;
  float lam = 1.f, gs = gscale, wdl = 0.f;
  if (seg.adapt) {  // block-uniform
    double ss, ww;  // the tensor's partials through the fixed trees (lars_seg.hpp)
    lars_tensor_sum2(seg, partials, ss, ww, red);
    const double gn = (double)gscale * sqrt(ss), wn = sqrt(ww);
    if (wn > 0.0 && gn > 0.0) lam = (float)((double)trust * wn / (gn + (double)wd * wn + (double)eps));
    gs = lam * gscale;
    wdl = lam * wd;
  }
  if (chunk == 0 && tid == 0) ratios[t] = lam;
  sgd_stage_chunk<MOM, VEC>(r, p, stage, buf, lr, gs, momentum, wdl, first, img);
}

}  // namespace psx

using namespace psx;

static int lars_launch_apply(float* p, float* stage, float* buf, long n, const void* table, int ntensors, int nblocks,
                             double* partials, float* ratios, float lr, float gscale, float momentum, float wd,
                             float trust, float eps, int first, void* img, hipStream_t st) {
  const bool mom = buf != nullptr && momentum != 0.f;
  const bool vec = al16(p) && al16(stage) && (!mom || al16(buf)) && al16(img);
  const LarsSeg* tb = (const LarsSeg*)table;
  uint16_t* im = (uint16_t*)img;
  dispatch2(mom, vec, [&](auto M, auto V) {
    hipLaunchKernelGGL((lars_apply_kernel<decltype(M)::value, decltype(V)::value>), dim3(nblocks), dim3(256), 0, st, p,
                       (const float*)stage, buf, n, tb, ntensors, nblocks, (const double*)partials, ratios, lr, gscale,
                       momentum, wd, trust, eps, first, im);
  });
  return (int)hipGetLastError();
}

static bool lars_args_ok(const void* p, const void* stage, long n, const void* table, int ntensors, int nblocks,
                         const void* partials, const void* ratios) {
  return p && stage && table && partials && ratios && n > 0 && ntensors > 0 && nblocks > 0;
}

extern "C" {

int psx_lars_table_size() { return (int)sizeof(LarsSeg); }
int psx_lars_chunk() { return kChunk; }

// The LARS update from nsrc gathered gradient wires (host array of nsrc <= 32 device pointers, all
// fp16 or all fp32, >= n elements each): two launches on `st`, no host synchronisation.
//   stage    : fp32 [n], receives the fp32 sum of the sources (must not alias a source)
//   table    : device array of ntensors LarsSeg covering [0, n), first_block ascending;
//              nblocks = sum of ceil(numel / psx_lars_chunk())
//   partials : double [2 * nblocks] scratch;  ratios: float [ntensors], lambda of every tensor
//   buf / first / img: as psx_sgd_apply_multi
int psx_lars_apply_multi(float* p, const void* const* srcs, int nsrc, int grad_fp16, float* stage, float* buf, long n,
                         const void* table, int ntensors, int nblocks, double* partials, float* ratios, float lr,
                         float gscale, float momentum, float wd, float trust, float eps, int first, void* img,
                         hipStream_t st) {
  if (!lars_args_ok(p, stage, n, table, ntensors, nblocks, partials, ratios)) return (int)hipErrorInvalidValue;
  WireSrcs sl{};
  bool vec = al16(p) && al16(stage);
  if (!fill_srcs(srcs, nsrc, grad_fp16 ? 2 : 4, n, sl, vec, stage)) return (int)hipErrorInvalidValue;
  const LarsSeg* tb = (const LarsSeg*)table;
  dispatch2(grad_fp16 != 0, vec, [&](auto H, auto V) {
    hipLaunchKernelGGL((lars_norms_kernel<wire_t<decltype(H)>, false, decltype(V)::value>), dim3(nblocks), dim3(256), 0,
                       st, (const float*)p, sl, stage, n, tb, ntensors, nblocks, partials);
  });
  const int rc = (int)hipGetLastError();
  if (rc) return rc;
  return lars_launch_apply(p, stage, buf, n, table, ntensors, nblocks, partials, ratios, lr, gscale, momentum, wd,
                           trust, eps, first, img, st);
}

// The dense entry: `stage` already holds the fp32 gradient sum (q8 / top-k payloads decoded into
// it, or an accumulated round); norms only, no rewrite, then the same apply.
int psx_lars_apply(float* p, float* stage, float* buf, long n, const void* table, int ntensors, int nblocks,
                   double* partials, float* ratios, float lr, float gscale, float momentum, float wd, float trust,
                   float eps, int first, void* img, hipStream_t st) {
  if (!lars_args_ok(p, stage, n, table, ntensors, nblocks, partials, ratios)) return (int)hipErrorInvalidValue;
  const WireSrcs sl{};
  const LarsSeg* tb = (const LarsSeg*)table;
  if (al16(p) && al16(stage))
    hipLaunchKernelGGL((lars_norms_kernel<float, true, true>), dim3(nblocks), dim3(256), 0, st, (const float*)p, sl,
                       stage, n, tb, ntensors, nblocks, partials);
  else
    hipLaunchKernelGGL((lars_norms_kernel<float, true, false>), dim3(nblocks), dim3(256), 0, st, (const float*)p, sl,
                       stage, n, tb, ntensors, nblocks, partials);
  const int rc = (int)hipGetLastError();
  if (rc) return rc;
  return lars_launch_apply(p, stage, buf, n, table, ntensors, nblocks, partials, ratios, lr, gscale, momentum, wd,
                           trust, eps, first, img, st);
}

}  // extern "C"
