// What the block-scaled gradient wires share (q8.hip, sign1.hip; parallel/blockwire.py is the
// Python side): a payload is one uint8 buffer of fixed size for a given n,
//   [ header: 4 x int32 = {magic, n, block = 256, nblk = ceil(n / 256)}      16 bytes
//   | scales: fp32[nblk], section padded to a multiple of 16 bytes
//   | body:   the codec's own bytes ]
// Blocks are runs of 256 consecutive elements of the flat parameter arena and are independent:
// every entry point takes a 256-aligned element sub-range [off, off + cnt).
//
// Here: layout and range check, the encoders' gradient loaders and header write, the source list
// with its host checks, and the two forms of the server update straight from the payloads as
// function templates over a codec policy W (the codec's arithmetic stays in its own file):
//   W::deq1(payload, body_off, i)    element i of one payload, decoded
//   W::unit_base(e0, u)              first element of 1024-element unit u of a range from e0
//   W::Unit, W::kAhead               a lane's part of one source's unit; sources loaded ahead of use
//   W::load(payload, body_off, ub, lane, unit), W::add(unit, s)   load it; add it into s[16]
#pragma once
#include <float.h>

#include "wire.hpp"

// Everything below keeps its multiplies and adds apart (hipcc contracts by default); the shared
// update tail (sgd_tail.hpp, included above) was parsed with the library default, as in optim.hip.
#pragma clang fp contract(off)

namespace psx {

constexpr int kBlock = 256;

struct BlockLayout {
  long nblk, scales_off, body_off, bytes;
};
static inline long block_count(long n) { return (n + kBlock - 1) / kBlock; }
// the layout for n elements and a body of body_bytes
static inline BlockLayout block_layout(long n, long body_bytes) {
  BlockLayout l;
  l.nblk = block_count(n);
  l.scales_off = 16;
  l.body_off = l.scales_off + ((4 * l.nblk + 15) & ~15L);
  l.bytes = l.body_off + body_bytes;
  return l;
}

// [off, off + cnt) must start on a block and end on a block or at n
static inline bool block_range_ok(long n, long off, long cnt) {
  return n > 0 && n <= 0x7fffffffL && off >= 0 && cnt >= 0 && off % kBlock == 0 && off + cnt <= n &&
         ((off + cnt) % kBlock == 0 || off + cnt == n);
}

// gradient elements as fp32 (fp32, or fp16 bits), one and four (g + i 16-byte, fp16: 8-byte aligned)
PSX_DEV float h2f(uint32_t bits) { return (float)__builtin_bit_cast(_Float16, (uint16_t)bits); }
PSX_DEV float ld_g1(const float* g, long i) { return g[i]; }
PSX_DEV float ld_g1(const uint16_t* g, long i) { return h2f(g[i]); }
PSX_DEV void ld_g4(const float* g, long i, float (&v)[4]) {
  const f32x4 t = *reinterpret_cast<const f32x4*>(g + i);
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = t[j];
}
PSX_DEV void ld_g4(const uint16_t* g, long i, float (&v)[4]) {
  const u32x2 t = *reinterpret_cast<const u32x2*>(g + i);
  v[0] = h2f(t[0] & 0xffff);
  v[1] = h2f(t[0] >> 16);
  v[2] = h2f(t[1] & 0xffff);
  v[3] = h2f(t[1] >> 16);
}

// the header, by the first four threads of workgroup 0 of the encode that covers block 0
PSX_DEV void block_write_header(int* hdr, int magic, long n) {
  if (hdr != nullptr && blockIdx.x == 0 && threadIdx.x < 4) {
    const long nblk = (n + kBlock - 1) / kBlock;
    hdr[threadIdx.x] = threadIdx.x == 0 ? magic : threadIdx.x == 1 ? (int)n : threadIdx.x == 2 ? kBlock : (int)nblk;
  }
}

struct BlockSrcs {
  const uint8_t* p[kMaxSrc];
  int n;
};

// one element's decoded sum over the sources, in source order
template <typename W>
PSX_DEV float block_sum1(const BlockSrcs& srcs, long body_off, long i) {
  float s = 0.f;
  for (int k = 0; k < srcs.n; ++k) s = s + W::deq1(srcs.p[k], body_off, i);
  return s;
}

// The update of element i alone: any alignment.
template <bool MOM, typename W>
PSX_DEV void block_apply1(float* __restrict__ p, const BlockSrcs& srcs, long body_off, float* __restrict__ buf, long i,
                          float lr, float gscale, float momentum, float wd, int first, uint16_t* __restrict__ img,
                          bool write_img) {
  const float pv = p[i];
  const float nv = sgd_tail<MOM>(block_sum1<W>(srcs, body_off, i), pv, buf + i, lr, gscale, momentum, wd, first);
  p[i] = nv;
  if (write_img) img[i] = f2bf(nv);
}

// Elements i0, i0 + stride, ... below e1, one at a time: any alignment. (blockDim is read by the
// kernels themselves and handed down: only there does the compiler know the workgroups uniform.)
template <bool MOM, typename W>
PSX_DEV void block_apply_elems(float* __restrict__ p, const BlockSrcs& srcs, long body_off, float* __restrict__ buf,
                               long i0, long stride, long e1, float lr, float gscale, float momentum, float wd,
                               int first, uint16_t* __restrict__ img, bool write_img) {
  for (long i = i0; i < e1; i += stride)
    block_apply1<MOM, W>(p, srcs, body_off, buf, i, lr, gscale, momentum, wd, first, img, write_img);
}

// Elements [e0, e1) (e0 a multiple of 256), a wave per 1024 elements as 4 rows of 256 (one block
// each); lane l owns elements 4 l .. 4 l + 3 of every row, so every p / buf / img access is 16
// bytes per lane and contiguous across the wave, and a lane's p and buf loads are issued ahead of
// the sources'. p, buf, img 16-byte aligned; what is left of the range after the whole units goes
// element by element in workgroup 0 (nthreads: its blockDim.x).
template <bool MOM, bool IMG, typename W>
PSX_DEV void block_apply_rows(float* __restrict__ p, const BlockSrcs& srcs, long body_off, float* __restrict__ buf,
                              long e0, long e1, float lr, float gscale, float momentum, float wd, int first,
                              uint16_t* __restrict__ img, unsigned nthreads) {
  const long nu = (e1 - e0) >> 10;  // whole 1024-element units
  const long t0 = e0 + (nu << 10);
  if (blockIdx.x == 0)
    block_apply_elems<MOM, W>(p, srcs, body_off, buf, t0 + threadIdx.x, nthreads, e1, lr, gscale, momentum, wd, first,
                              img, IMG);
  const int lane = threadIdx.x & 63;
  const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long)gridDim.x * 4;
  for (long u = wave; u < nu; u += nwaves) {
    const long ub = W::unit_base(e0, u);
    const long e = ub + lane * 4;  // row v: e + 256 v
    f32x4 pv[4];
    float bv[16] = {};
#pragma unroll
    for (int v = 0; v < 4; ++v) pv[v] = *reinterpret_cast<const f32x4*>(p + e + 256 * v);
    if (MOM && !first) {
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(buf + e + 256 * v);
#pragma unroll
        for (int j = 0; j < 4; ++j) bv[4 * v + j] = t[j];
      }
    }
    float s[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) s[j] = 0.f;
    for (int k0 = 0; k0 < srcs.n; k0 += W::kAhead) {
      typename W::Unit un[W::kAhead];
#pragma unroll
      for (int m = 0; m < W::kAhead; ++m)
        if (k0 + m < srcs.n) W::load(srcs.p[k0 + m], body_off, ub, lane, un[m]);
#pragma unroll
      for (int m = 0; m < W::kAhead; ++m)
        if (k0 + m < srcs.n) W::add(un[m], s);
    }
#pragma unroll
    for (int v = 0; v < 4; ++v)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        pv[v][j] = sgd_tail<MOM>(s[4 * v + j], pv[v][j], &bv[4 * v + j], lr, gscale, momentum, wd, first);
#pragma unroll
    for (int v = 0; v < 4; ++v) *reinterpret_cast<f32x4*>(p + e + 256 * v) = pv[v];
    if (MOM) {
#pragma unroll
      for (int v = 0; v < 4; ++v)
        *reinterpret_cast<f32x4*>(buf + e + 256 * v) = (f32x4){bv[4 * v], bv[4 * v + 1], bv[4 * v + 2], bv[4 * v + 3]};
    }
    if (IMG) {
#pragma unroll
      for (int v = 0; v < 4; ++v)
        *reinterpret_cast<u32x2*>(img + e + 256 * v) = (u32x2){pack_bf2(pv[v][0], pv[v][1]), pack_bf2(pv[v][2], pv[v][3])};
    }
  }
}

// The host prologue of apply_multi: the checks, and the device's source list from the host's
// array of nsrc payloads of `bytes` bytes each. hipErrorInvalidValue (nothing may be launched) for
// a bad count or range, a null or misaligned payload, or one that shares a byte with p, buf
// (fp32 [n]) or img (bf16 [n]); 0 with sl.n == 0 for an empty range (nothing to launch).
static inline int block_apply_prologue(const void* const* payloads, int nsrc, long bytes, long n, long off, long cnt,
                                       const void* p, const void* buf, const void* img, BlockSrcs& sl) {
  sl.n = 0;
  if (!payloads || nsrc < 1 || nsrc > kMaxSrc || !block_range_ok(n, off, cnt)) return (int)hipErrorInvalidValue;
  if (cnt == 0) return 0;
  for (int k = 0; k < nsrc; ++k) {
    const void* s = payloads[k];
    if (!s || !al16(s)) return (int)hipErrorInvalidValue;
    if (ranges_overlap(s, (size_t)bytes, p, (size_t)n * 4) ||
        (buf && ranges_overlap(s, (size_t)bytes, buf, (size_t)n * 4)) ||
        (img && ranges_overlap(s, (size_t)bytes, img, (size_t)n * 2)))
      return (int)hipErrorInvalidValue;
    sl.p[k] = (const uint8_t*)s;
  }
  sl.n = nsrc;
  return 0;
}

}  // namespace psx
