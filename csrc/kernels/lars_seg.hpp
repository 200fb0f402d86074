// The per-tensor segment table and the deterministic per-tensor reduction shared by the layer-wise
// server updates (lars.hip, lamb.hip).
//
// The trainable prefix of the arena is covered by one LarsSeg record per tensor (models/layout.py
// order); the kernels run over one flat grid of (tensor, chunk of kChunk elements) workgroups
// of 256 threads. The chunk's range and walk, the wire sum and the double block sums are wire.hpp's;
// a tensor's per-workgroup partials are summed here with a fixed lane assignment and the same
// trees (lars_tensor_sum2).
#pragma once
#include "wire.hpp"

namespace psx {

struct LarsSeg {
  long offset;      // first arena element of the tensor
  long numel;
  int adapt;        // 1: trust ratio + weight decay (ndim > 1); 0: ratio 1, no weight decay
  int first_block;  // first workgroup of the tensor in the flat grid
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

// the two sums of a tensor's partials: partial j on lane (j - first) % 256, lane-serial, then the
// fixed trees (every thread gets both)
PSX_DEV void lars_tensor_sum2(const LarsSeg& seg, const double* __restrict__ partials, double& a, double& b,
                              double (*red)[4]) {
  const long b0 = seg.first_block, b1 = b0 + (seg.numel + kChunk - 1) / kChunk;
  a = 0.0;
  b = 0.0;
  for (long j = b0 + threadIdx.x; j < b1; j += 256) {
    a += partials[2 * j];
    b += partials[2 * j + 1];
  }
  block_sum2_f64(a, b, red);
}

}  // namespace psx
