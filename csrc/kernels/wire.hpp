// What the server update kernels share (optim.hip, lars.hip, adamw.hip, lamb.hip, gguard.hip,
// dcasgd.hip): the list of gradient wires and its fp32 sum, the walk over one chunk of the arena,
// the double block reductions, the bf16 image store, and the host side's pointer checks and
// launch dispatch. Everything here inlines into its caller; the arithmetic of an update stays in
// the tail headers (sgd_tail.hpp, adamw_tail.hpp, lamb_tail.hpp).
//
// The sum of a round: every wire decoded to fp32 and added in fp32, starting from 0, in list
// order k = 0..W-1 (what the reference's numpy loop does; an RCCL fp16 reduce would round the
// running sum to fp16 at every hop). The scalar and the 8-wide form add the same values in the
// same order, so which one a lane takes never changes the bits.
//
// A chunk is kChunk arena elements of one workgroup of 256 threads. It starts at any element: its
// head up to the next multiple of 8 arena elements and its tail are scalar accesses, the body is
// 8 elements per lane. Which element a lane owns depends only on the chunk's position in the
// arena, never on pointer alignment.
//
// Reductions: no atomics. Partials are double from the cross-lane step on: xor shuffle tree over
// the wave, then the four waves summed in order through LDS, ((r0 + r1) + r2) + r3.
#pragma once
#include <initializer_list>
#include <type_traits>

#include "common.hpp"
#include "sgd_tail.hpp"

namespace psx {

constexpr int kMaxSrc = 32;   // reference server.py:424-426 caps the job at 32 workers
constexpr int kChunk = 8192;  // elements per workgroup of the chunked kernels: 32 body elements per lane

struct WireSrcs {
  const void* p[kMaxSrc];
  int n;
};

// wire element i as fp32 (fp16 bits or fp32)
template <typename I>
PSX_DEV float ld_wire(const uint16_t* g, I i) {
  return (float)__builtin_bit_cast(_Float16, g[i]);
}
template <typename I>
PSX_DEV float ld_wire(const float* g, I i) {
  return g[i];
}

// 8 consecutive wire elements (one 16-byte fp16 load, or two fp32 ones; g 16-byte aligned)
PSX_DEV void ld_wire8(const uint16_t* g, float (&v)[8]) {
  const u32x4 w = *reinterpret_cast<const u32x4*>(g);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v[2 * j] = (float)__builtin_bit_cast(_Float16, (uint16_t)(w[j] & 0xffff));
    v[2 * j + 1] = (float)__builtin_bit_cast(_Float16, (uint16_t)(w[j] >> 16));
  }
}
PSX_DEV void ld_wire8(const float* g, float (&v)[8]) { ld8(g, v); }

// s = sum_k decode(src_k[i]) in source order
template <typename GT, typename I>
PSX_DEV float wire_sum1(const WireSrcs& srcs, I i) {
  float s = 0.f;
  for (int k = 0; k < srcs.n; ++k) s += ld_wire(reinterpret_cast<const GT*>(srcs.p[k]), i);
  return s;
}

// the 8 sums s[j] = sum_k decode(src_k[i + j]) in source order, 16-byte loads (every source + i
// 16-byte aligned)
template <typename GT, typename I>
PSX_DEV void wire_sum8(const WireSrcs& srcs, I i, float (&s)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) s[j] = 0.f;
  for (int k = 0; k < srcs.n; ++k) {
    float g[8];
    ld_wire8(reinterpret_cast<const GT*>(srcs.p[k]) + i, g);
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] += g[j];
  }
}

// the bf16 image of 8 consecutive parameters, one 16-byte store
PSX_DEV void st_bf8(uint16_t* img, const float (&v)[8]) {
  const u32x4 o = {pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]), pack_bf2(v[4], v[5]), pack_bf2(v[6], v[7])};
  *reinterpret_cast<u32x4*>(img) = o;
}

PSX_DEV double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// block-wide sum in double for 256 threads: wave trees, then the four waves in order (every
// thread gets it)
PSX_DEV double block_sum_f64(double a, double* red) {
  a = wave_sum_f64(a);
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  if (l == 0) red[w] = a;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// the same for a pair {a, b}
PSX_DEV void block_sum2_f64(double& a, double& b, double (*red)[4]) {
  a = wave_sum_f64(a);
  b = wave_sum_f64(b);
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  if (l == 0) {
    red[0][w] = a;
    red[1][w] = b;
  }
  __syncthreads();
  a = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
  b = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
}

// arena range [a0, a1) of one chunk: scalar head [a0, ha), 8-element groups [ha, tb), tail [tb, a1)
struct ChunkRange {
  long a0, ha, tb, a1;
};
// chunk number `chunk` of the segment [offset, offset + numel) of an arena of n elements; a chunk
// past the segment's end is empty (a1 <= a0 = ha = tb: no head, no group, no tail)
PSX_DEV ChunkRange chunk_range(long offset, long numel, int chunk, long n) {
  ChunkRange r;
  const long end = min(offset + numel, n);
  r.a0 = offset + (long)chunk * kChunk;
  r.a1 = min(r.a0 + kChunk, end);
  r.ha = min(r.a1, (r.a0 + 7) & ~7L);
  r.tb = r.ha + ((r.a1 - r.ha) & ~7L);
  return r;
}

// The walk of one workgroup over its chunk: one(i) for every head and tail element, and for
// every group of 8 at i eight(i) when VEC (16-byte accesses: every base pointer 16-byte aligned),
// else one(i), ..., one(i + 7).
template <bool VEC, typename One, typename Eight>
PSX_DEV void for_chunk(const ChunkRange& r, One one, Eight eight) {
  const int tid = threadIdx.x;
  if (tid < r.ha - r.a0) one(r.a0 + tid);
  const long ng = (r.tb - r.ha) >> 3;
  for (long q = tid; q < ng; q += 256) {
    const long i = r.ha + 8 * q;
    if constexpr (VEC) {
      eight(i);
    } else {
      for (int j = 0; j < 8; ++j) one(i + j);
    }
  }
  if (tid < r.a1 - r.tb) one(r.tb + tid);
}

// The update tail (sgd_tail.hpp) over one chunk of a staged fp32 gradient sum: p, buf and the
// optional bf16 image from stage, with the caller's gs and wd (lars_apply, guard_apply).
template <bool MOM, bool VEC>
PSX_DEV void sgd_stage_chunk(const ChunkRange& r, float* __restrict__ p, const float* __restrict__ stage,
                             float* __restrict__ buf, float lr, float gs, float momentum, float wd, int first,
                             uint16_t* __restrict__ img) {
  for_chunk<VEC>(
      r,
      [&](long i) {
        const float pv = p[i];
        const float nv = sgd_tail<MOM>(stage[i], pv, buf + i, lr, gs, momentum, wd, first);
        p[i] = nv;
        if (img) img[i] = f2bf(nv);
      },
      [&](long i) {
        float s[8], pv[8], bv[8];
        ld8(stage + i, s);
        ld8(p + i, pv);
        if (MOM && !first) ld8(buf + i, bv);
#pragma unroll
        for (int j = 0; j < 8; ++j) pv[j] = sgd_tail<MOM>(s[j], pv[j], &bv[j], lr, gs, momentum, wd, first);
        st8(p + i, pv);
        if (MOM) st8(buf + i, bv);
        if (img) st_bf8(img + i, pv);
      });
}

// ---- host side ----

static inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// [a, a + na) and [b, b + nb) share a byte
static inline bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + nb && y < x + na;
}

// grid of a grid-stride kernel over `work` threads: memory-bound, so a capped number of workgroups
static inline int stream_grid(size_t work, size_t cap = 4096) {
  size_t g = (work + 255) / 256;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}

// The device's source list from the host's array of nsrc wires of n elements of esz bytes; every
// source's alignment is folded into vec. False (nothing launched) for a bad count, a null source,
// a source that is `stage`, or one that shares a byte with one of the fp32 [n] buffers in `state`.
static inline bool fill_srcs(const void* const* srcs, int nsrc, size_t esz, long n, WireSrcs& sl, bool& vec,
                             const void* stage, std::initializer_list<const void*> state = {}) {
  if (!srcs || nsrc < 1 || nsrc > kMaxSrc) return false;
  sl.n = nsrc;
  for (int k = 0; k < nsrc; ++k) {
    const void* s = srcs[k];
    if (!s || s == stage) return false;
    for (const void* b : state)
      if (ranges_overlap(s, (size_t)n * esz, b, (size_t)n * 4)) return false;
    sl.p[k] = s;
    vec = vec && al16(s);
  }
  return true;
}

// f(A, B) with the two run-time switches as std::bool_constant arguments: one launch site for the
// four instantiations of a kernel templated on both
template <typename F>
static inline void dispatch2(bool a, bool b, F f) {
  if (a && b) f(std::true_type{}, std::true_type{});
  else if (a) f(std::true_type{}, std::false_type{});
  else if (b) f(std::false_type{}, std::true_type{});
  else f(std::false_type{}, std::false_type{});
}
// the wire element type of a dispatch2 switch on grad_fp16
template <typename FP16>
using wire_t = std::conditional_t<FP16::value, uint16_t, float>;

}  // namespace psx
