// The per-tensor segment table and the deterministic per-tensor reduction shared by the layer-wise
// server updates (lars.hip, lamb.hip).
//
// The trainable prefix of the arena is covered by one LarsSeg record per tensor (models/layout.py
// order); the kernels run over one flat grid of (tensor, chunk of kLarsChunk elements) workgroups
// of 256 threads. A chunk starts at any element: its head up to the next multiple of 8 arena
// elements and its tail are scalar accesses, the body is 8 elements per lane. Which element a lane
// owns depends only on the chunk's position in the arena, never on pointer alignment.
//
// Reductions: no atomics. A lane accumulates serially in fp32 with explicit fma, partials are
// double from the cross-lane step on (xor shuffle tree over the wave, the four waves summed in
// order through LDS); a tensor's per-workgroup partials are summed with a fixed lane assignment
// and the same trees (lars_tensor_sum2).
#pragma once
#include "common.hpp"

namespace psx {

constexpr int kLarsChunk = 8192;  // elements per workgroup: 32 body elements per lane
constexpr int kLarsMaxSrc = 32;   // reference server.py:424-426 caps the job at 32 workers

struct LarsSeg {
  long offset;      // first arena element of the tensor
  long numel;
  int adapt;        // 1: trust ratio + weight decay (ndim > 1); 0: ratio 1, no weight decay
  int first_block;  // first workgroup of the tensor in the flat grid
};

struct LarsSrcs {
  const void* p[kLarsMaxSrc];
  int n;
};

// which tensor owns this workgroup: every record's block range tested in parallel (-1: none)
PSX_DEV int lars_find(const LarsSeg* __restrict__ table, int ntensors, int nblocks, int* sh) {
  if (threadIdx.x == 0) *sh = -1;
  __syncthreads();
  const int bid = blockIdx.x;
  for (int k = threadIdx.x; k < ntensors; k += blockDim.x) {
    const int lo = table[k].first_block;
    const int hi = k + 1 < ntensors ? table[k + 1].first_block : nblocks;
    if (lo <= bid && bid < hi) *sh = k;
  }
  __syncthreads();
  return *sh;
}

// arena range [a0, a1) of one chunk: scalar head [a0, ha), 8-element groups [ha, tb), tail [tb, a1)
struct LarsRange {
  long a0, ha, tb, a1;
};
PSX_DEV LarsRange lars_range(const LarsSeg& s, int chunk, long n) {
  LarsRange r;
  const long end = min(s.offset + s.numel, n);
  r.a0 = min(s.offset + (long)chunk * kLarsChunk, end);
  r.a1 = min(r.a0 + kLarsChunk, end);
  r.ha = min(r.a1, (r.a0 + 7) & ~7L);
  r.tb = r.ha + ((r.a1 - r.ha) & ~7L);
  return r;
}

PSX_DEV float lars_ld(const uint16_t* g, long i) { return (float)__builtin_bit_cast(_Float16, g[i]); }
PSX_DEV float lars_ld(const float* g, long i) { return g[i]; }

PSX_DEV double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// block-wide {a, b} in double: wave trees, then the four waves in order (every thread gets both)
PSX_DEV void lars_block_sum2(double& a, double& b, double (*red)[4]) {
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

// the two sums of a tensor's partials: partial j on lane (j - first) % 256, lane-serial, then the
// fixed trees (every thread gets both)
PSX_DEV void lars_tensor_sum2(const LarsSeg& seg, const double* __restrict__ partials, double& a, double& b,
                              double (*red)[4]) {
  const long b0 = seg.first_block, b1 = b0 + (seg.numel + kLarsChunk - 1) / kLarsChunk;
  a = 0.0;
  b = 0.0;
  for (long j = b0 + threadIdx.x; j < b1; j += 256) {
    a += partials[2 * j];
    b += partials[2 * j + 1];
  }
  lars_block_sum2(a, b, red);
}

// the 8 fp32 sums s[j] = sum_k decode(src_k[i + j]) in source order, 16-byte loads (i and every
// source 16-byte aligned)
template <typename GT>
PSX_DEV void lars_sum8(const LarsSrcs& srcs, long i, float (&s)[8]) {
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
      const float* g = reinterpret_cast<const float*>(srcs.p[k]) + i;
      const f32x4 a = *reinterpret_cast<const f32x4*>(g);
      const f32x4 b = *reinterpret_cast<const f32x4*>(g + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        s[j] += a[j];
        s[4 + j] += b[j];
      }
    }
  }
}

}  // namespace psx
