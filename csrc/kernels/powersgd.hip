// Rank-r PowerSGD gradient codec (Vogels et al. 2019), --codec powersgd: one round trip, so it fits
// a parameter server. Every worker compresses on its own; the server sums the decoded products.
// Per worker: an fp32 residual e [n] and one cols x r matrix Q per compressed tensor (warm start).
// For every tensor with ndim > 1 that gains from rank r (the host table decides, ops/kernels.py
// PowerSGDTable), read as the row-major rows x cols matrix it is in the arena:
//   M  = g + e
//   P  = M Q                                   rows x r
//   P^ = the columns of P orthonormalised by modified Gram-Schmidt in column order, fp32
//   Q' = M^T P^                                cols x r, the next push's Q
//   e  = M - P^ Q'^T
//   wire: P^ and Q', fp32
// A column of P whose squared norm after its projections is 0, or at most kPgDrop (1e-8) of its
// squared norm before them, is stored as zeros, and so is its Q' column on the wire: no 0 / 0, and
// no rounding noise blown up to a unit vector that is not orthogonal to the others. The worker's own
// Q keeps its previous column in that case (an all-zero gradient would otherwise leave Q = 0, whose
// P is 0 for ever). Every other tensor travels as fp16 of g in a dense tail and has no residual.
//
// Payload (bytes): [16-byte frame the host writes | fp32 factors | fp16 tail], padded to 16. A
// compressed tensor's factors are P^ [rows][r] then Q' [cols][r], both row-major; the worker's Q
// buffer has the factor section's layout (only the Q' places are used).
//
// The encode is four launches on the caller's stream, no host synchronisation, each one flat grid
// over all compressed tensors through a precomputed tile map (PsgdPlan), as muon.hip's:
//   psgd_project     : workgroup = 64 rows x one slab of the columns. Reads g and e 32 columns at a
//                      time, writes M back into e, stages M (MFMA row operand) and the slab's rows
//                      of Q (column operand, r zero-padded to 16) in LDS; each of the four waves
//                      owns 16 rows x 16 and keeps two accumulators for the two 16-deep halves of a
//                      step, added once at the end. The slab's partial P goes to the workspace.
//                      rows / 64 tiles alone are far too few (512 x 4608: 8), so the columns are
//                      cut into slabs of 256. The grid's last workgroups write the fp16 tail.
//   psgd_orth        : one workgroup per tensor. Slabs summed in slab order into LDS (rows x r
//                      fp32, at most kPgLdsFloats = 128 KB of the 160 KB), then Gram-Schmidt: a
//                      thread owns rows tid, tid + 256, ... of every column, so only the dot
//                      products cross threads (fp32 fma in row order per thread, then wire.hpp's
//                      double trees). P^ goes straight into the payload, the dropped columns' mask
//                      into the workspace.
//   psgd_backproject : Q' = M^T P^, workgroup = 64 columns, K = rows in steps of 32; the M tile is
//                      K-strided and read from LDS as four scalars per fragment (muon.hip's NN
//                      form), P^ is staged transposed. K is not split: the output tiles number
//                      sum(cols) / 64, about 450 on ResNet-18. Into the payload and the worker's Q.
//   psgd_residual    : e = M - P^ Q'^T, workgroup = 64 x 64, wave = 16 rows x 64 columns, K = r: one
//                      v_mfma_f32_16x16x4_f32 per 16 x 16 tile per 4 ranks, operands straight from
//                      the payload (a lane needs one float of each per MFMA). The product is taken
//                      transposed (Q' is the row operand), so a lane ends with four consecutive
//                      columns of one row: 16-byte accesses of e. Store-bound.
// psgd_decode is the server's one launch for W payloads: psgd_residual's tile with the workers'
// products chained through the accumulator in list order, overwrite or add, then the fp16 tails
// summed in fp32 in list order. With W = 1 the product has the bits the worker subtracted: the same
// function (psgd_outer), the same K order, the same MFMA.
//
// Accesses are 16 bytes wide where a tensor's offset and cols are multiples of 4 (every ResNet conv
// but the stem), element-wise otherwise. Determinism: one owner per output element, fixed K order,
// slabs summed in slab order, no float atomics.
#include <math.h>

#include "lars_seg.hpp"

namespace psx {

constexpr int kPgTile = 64;            // rows (project, residual) or columns (backproject, residual) per workgroup
constexpr int kPgKT = 32;              // K elements staged per main-loop step
constexpr int kPgLd = kPgKT + 4;       // LDS row stride of a K-contiguous operand tile
constexpr int kPgLdX = kPgTile + 4;    // LDS row stride of backproject's [32][64] M tile
constexpr int kPgLdsFloats = 32768;    // psgd_orth's LDS budget: rows * r floats
constexpr int kPgHeader = 16;          // bytes of the payload's frame
constexpr float kPgDrop = 1e-8f;       // the dropped-column fraction of the header comment

// one trainable tensor of the model, compressed or tail (ops/kernels.py PowerSGDTable builds the records)
struct PsgdSeg {
  long offset;       // first arena element
  long numel;
  long foff;         // compressed: P^ in the factor section (floats), Q' follows at foff + rows * r; tail: its place in the tail (halfs)
  long woff;         // its `slabs` partial P in the workspace (floats)
  int rows, cols;
  int slabs, kslab;  // the columns in `slabs` slabs of kslab (a multiple of kPgKT; the last may be short)
  int comp;          // 1: compressed, 0: tail
  int vec;           // offset and cols are multiples of 4
};

struct PsgdPlan {
  const PsgdSeg* segs;
  const int4* map_p;  // {tensor, row tile, slab, 0}
  const int4* map_q;  // {tensor, column tile, compressed index, 0}
  const int4* map_r;  // {tensor, row tile, column tile, 0}
  const int4* map_t;  // {tensor, chunk of kChunk, 0, 0} over the tail tensors
  const int* comp;    // compressed index -> tensor
  long factors;       // floats of the factor section
  long tails;         // halfs of the tail
  long wsfloats;      // floats of the partial-P workspace; the dropped-column masks (int [ncomp]) follow
  int nseg, ncomp, ntp, ntq, ntr, ntt;
  int orth_floats;    // max rows * r over the compressed tensors
};

struct PsgdSrcs {
  const uint8_t* p[kMaxSrc];
  int n;
};

PSX_DEV f32x4 ld_wire4(const float* g, long i) { return *reinterpret_cast<const f32x4*>(g + i); }
PSX_DEV f32x4 ld_wire4(const uint16_t* g, long i) {
  const u32x2 w = *reinterpret_cast<const u32x2*>(g + i);
  return (f32x4){(float)__builtin_bit_cast(_Float16, (uint16_t)(w[0] & 0xffff)),
                 (float)__builtin_bit_cast(_Float16, (uint16_t)(w[0] >> 16)),
                 (float)__builtin_bit_cast(_Float16, (uint16_t)(w[1] & 0xffff)),
                 (float)__builtin_bit_cast(_Float16, (uint16_t)(w[1] >> 16))};
}
PSX_DEV uint16_t to_half(float v) { return __builtin_bit_cast(uint16_t, (_Float16)v); }
PSX_DEV uint16_t to_half(uint16_t v) { return v; }
template <typename GT>
PSX_DEV GT ld_raw(const GT* g, long i) {
  return g[i];
}

PSX_DEV f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// the range of one chunk of a tail tensor
PSX_DEV void psgd_tail_range(const PsgdSeg& g, int chunk, long& i0, long& i1) {
  i0 = (long)chunk * kChunk;
  i1 = min(i0 + kChunk, g.numel);
}

template <typename GT>
__global__ __launch_bounds__(256) void psgd_project_kernel(const GT* __restrict__ gr, float* __restrict__ e,
                                                           const float* __restrict__ q, float* __restrict__ ws,
                                                           uint16_t* __restrict__ tail, PsgdPlan pl, int r, int vecok) {
  __shared__ __attribute__((aligned(16))) float sa[kPgTile * kPgLd];
  __shared__ __attribute__((aligned(16))) float sq[16 * kPgLd];
  const int tid = threadIdx.x;
  if ((int)blockIdx.x >= pl.ntp) {  // the fp16 tail: block-uniform
    const int4 t = pl.map_t[blockIdx.x - pl.ntp];
    const PsgdSeg g = pl.segs[t.x];
    long i0, i1;
    psgd_tail_range(g, t.y, i0, i1);
    for (long i = i0 + tid; i < i1; i += 256) tail[g.foff + i] = to_half(ld_raw(gr, g.offset + i));
    return;
  }
  const int4 tile = pl.map_p[blockIdx.x];
  const PsgdSeg g = pl.segs[tile.x];
  const int rows = g.rows, cols = g.cols, row0 = tile.y * kPgTile;
  const int k0 = tile.z * g.kslab, k1 = min(cols, k0 + g.kslab);
  const bool vec = vecok && g.vec;
  const GT* __restrict__ gp = gr + g.offset;
  float* __restrict__ ep = e + g.offset;
  const float* __restrict__ qp = q + g.foff + (long)rows * r;

  const int lane = tid & 63, wave = tid >> 6, l16 = lane & 15, kg = lane >> 4;
  f32x4 acc[2] = {};
  f32x4 ra[2];
  float rq[2];
  // M = g + e of this step's 64 x 32, written back; zeros outside the matrix and the slab
  auto fetch = [&](int k) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = tid + 256 * i, rr = row0 + (c >> 3), kk = k + 4 * (c & 7);
      f32x4 m = {0.f, 0.f, 0.f, 0.f};
      if (rr < rows && kk < k1) {
        const long at = (long)rr * cols + kk;
        if (vec) {  // cols and the slab's end are multiples of 4: kk < k1 covers kk + 3
          m = ld_wire4(gp, at) + *reinterpret_cast<const f32x4*>(ep + at);
          *reinterpret_cast<f32x4*>(ep + at) = m;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (kk + j < k1) {
              m[j] = ld_wire(gp, at + j) + ep[at + j];
              ep[at + j] = m[j];
            }
        }
      }
      ra[i] = m;
      const int kq = k + (c >> 4), jq = c & 15;
      rq[i] = jq < r && kq < k1 ? qp[(long)kq * r + jq] : 0.f;
    }
  };
  fetch(k0);
  for (int k = k0; k < k1; k += kPgKT) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = tid + 256 * i;
      *reinterpret_cast<f32x4*>(&sa[(c >> 3) * kPgLd + 4 * (c & 7)]) = ra[i];
      sq[(c & 15) * kPgLd + (c >> 4)] = rq[i];
    }
    __syncthreads();
    if (k + kPgKT < k1) fetch(k + kPgKT);  // in flight under the MFMAs below
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const f32x4 fa = *reinterpret_cast<const f32x4*>(&sa[(wave * 16 + l16) * kPgLd + 16 * h + 4 * kg]);
      const f32x4 fb = *reinterpret_cast<const f32x4*>(&sq[l16 * kPgLd + 16 * h + 4 * kg]);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[h] = mfma4(fa[j], fb[j], acc[h]);
    }
    __syncthreads();
  }
  // lane holds rows 4 kg .. 4 kg + 3 of column l16 of its wave's 16 x 16
  float* __restrict__ out = ws + g.woff + (long)tile.z * rows * r;
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const int row = row0 + wave * 16 + 4 * kg + v;
    if (row < rows && l16 < r) out[(long)row * r + l16] = acc[0][v] + acc[1][v];
  }
}

// block-wide sum in double, every thread gets it; consecutive calls alternate between the two
// rows of `red`, so a call never overwrites what a slower wave still reads
PSX_DEV double psgd_bsum(double v, double (*red)[4], int& par) {
  v = wave_sum_f64(v);
  double* rd = red[par];
  par ^= 1;
  if ((threadIdx.x & 63) == 0) rd[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((rd[0] + rd[1]) + rd[2]) + rd[3];
}

__global__ __launch_bounds__(256) void psgd_orth_kernel(const float* __restrict__ ws, int* __restrict__ drop,
                                                        float* __restrict__ fac, PsgdPlan pl, int r) {
  extern __shared__ __attribute__((aligned(16))) float sp[];  // [rows][r]
  __shared__ double red[2][4];
  const PsgdSeg g = pl.segs[pl.comp[blockIdx.x]];
  const int tid = threadIdx.x, rows = g.rows;
  const int total = rows * r;
  const float* __restrict__ w = ws + g.woff;
  for (int i = tid; i < total; i += 256) {
    float s = w[i];
    for (int sl = 1; sl < g.slabs; ++sl) s += w[(long)sl * total + i];
    sp[i] = s;
  }
  __syncthreads();  // from here on a thread touches its own rows only
  int par = 0, mask = 0;
  auto dot = [&](int a, int b) {
    float s = 0.f;
    for (int row = tid; row < rows; row += 256) s = __builtin_fmaf(sp[row * r + a], sp[row * r + b], s);
    return psgd_bsum((double)s, red, par);
  };
  for (int j = 0; j < r; ++j) {
    const double n0 = dot(j, j);
    for (int i = 0; i < j; ++i) {
      if (mask >> i & 1) continue;  // block-uniform
      const float d = (float)dot(i, j);
      for (int row = tid; row < rows; row += 256) sp[row * r + j] = __builtin_fmaf(-d, sp[row * r + i], sp[row * r + j]);
    }
    const double n1 = dot(j, j);
    const bool dropped = n1 == 0.0 || n1 <= (double)kPgDrop * n0;  // a NaN norm is kept: it travels, as on every wire
    if (dropped) mask |= 1 << j;
    const float inv = dropped ? 0.f : (float)(1.0 / sqrt(n1));
    for (int row = tid; row < rows; row += 256) sp[row * r + j] = dropped ? 0.f : sp[row * r + j] * inv;
  }
  float* __restrict__ out = fac + g.foff;
  for (int row = tid; row < rows; row += 256)
    for (int j = 0; j < r; ++j) out[(long)row * r + j] = sp[row * r + j];
  if (tid == 0) drop[blockIdx.x] = mask;
}

__global__ __launch_bounds__(256) void psgd_backproject_kernel(const float* __restrict__ e,
                                                               const int* __restrict__ drop, float* __restrict__ fac,
                                                               float* __restrict__ q, PsgdPlan pl, int r, int vecok) {
  __shared__ __attribute__((aligned(16))) float sx[kPgKT * kPgLdX];
  __shared__ __attribute__((aligned(16))) float sp[16 * kPgLd];
  const int4 tile = pl.map_q[blockIdx.x];
  const PsgdSeg g = pl.segs[tile.x];
  const int rows = g.rows, cols = g.cols, col0 = tile.y * kPgTile;
  const bool vec = vecok && g.vec;
  const float* __restrict__ ep = e + g.offset;
  const float* __restrict__ pp = fac + g.foff;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, kg = lane >> 4;
  f32x4 acc[2] = {};
  f32x4 ra[2];
  float rp[2];
  auto fetch = [&](int k) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = tid + 256 * i, kr = k + (c >> 4), cc = col0 + 4 * (c & 15);
      f32x4 m = {0.f, 0.f, 0.f, 0.f};
      if (kr < rows && cc < cols) {
        const long at = (long)kr * cols + cc;
        if (vec) {  // cols is a multiple of 4: cc < cols covers cc + 3
          m = *reinterpret_cast<const f32x4*>(ep + at);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (cc + j < cols) m[j] = ep[at + j];
        }
      }
      ra[i] = m;
      const int jq = c & 15;
      rp[i] = jq < r && kr < rows ? pp[(long)kr * r + jq] : 0.f;
    }
  };
  fetch(0);
  for (int k = 0; k < rows; k += kPgKT) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = tid + 256 * i;
      *reinterpret_cast<f32x4*>(&sx[(c >> 4) * kPgLdX + 4 * (c & 15)]) = ra[i];
      sp[(c & 15) * kPgLd + (c >> 4)] = rp[i];
    }
    __syncthreads();
    if (k + kPgKT < rows) fetch(k + kPgKT);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const f32x4 fb = *reinterpret_cast<const f32x4*>(&sp[l16 * kPgLd + 16 * h + 4 * kg]);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[h] = mfma4(sx[(16 * h + 4 * kg + j) * kPgLdX + wave * 16 + l16], fb[j], acc[h]);
    }
    __syncthreads();
  }
  const int mask = drop[tile.z];
  const long qoff = g.foff + (long)rows * r;
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const int oc = col0 + wave * 16 + 4 * kg + v;
    if (oc < cols && l16 < r) {
      const float val = acc[0][v] + acc[1][v];
      fac[qoff + (long)oc * r + l16] = val;
      if (!(mask >> l16 & 1)) q[qoff + (long)oc * r + l16] = val;
    }
  }
}

// acc[c] += (P^ Q'^T)^T of the wave's 16 rows (from mrow) x columns colbase + 16 c .. + 15, K = r in
// steps of 4: afterwards a lane holds columns colbase + 16 c + 4 kg .. + 3 of row mrow + l16
PSX_DEV void psgd_outer(f32x4 (&acc)[4], const float* __restrict__ pp, const float* __restrict__ qq, int rows,
                        int cols, int r, int mrow, int colbase, int l16, int kg) {
  for (int s = 0; s < r; s += 4) {
    const float b = mrow + l16 < rows ? pp[(long)(mrow + l16) * r + s + kg] : 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int col = colbase + 16 * c + l16;
      const float a = col < cols ? qq[(long)col * r + s + kg] : 0.f;
      acc[c] = mfma4(a, b, acc[c]);
    }
  }
}

// DECODE: out = [out +] the sum of the W products and tails; else e = M - the payload's own product
template <bool DECODE>
__global__ __launch_bounds__(256) void psgd_outer_kernel(float* __restrict__ dst, PsgdSrcs srcs, PsgdPlan pl, int r,
                                                         int add, int vecok) {
  const int tid = threadIdx.x;
  if constexpr (DECODE) {
    if ((int)blockIdx.x >= pl.ntr) {  // the tails: block-uniform
      const int4 t = pl.map_t[blockIdx.x - pl.ntr];
      const PsgdSeg g = pl.segs[t.x];
      long i0, i1;
      psgd_tail_range(g, t.y, i0, i1);
      const long tb = kPgHeader + 4 * pl.factors;
      for (long i = i0 + tid; i < i1; i += 256) {
        float s = 0.f;
        for (int k = 0; k < srcs.n; ++k) s += ld_wire(reinterpret_cast<const uint16_t*>(srcs.p[k] + tb), g.foff + i);
        dst[g.offset + i] = add ? dst[g.offset + i] + s : s;
      }
      return;
    }
  }
  const int4 tile = pl.map_r[blockIdx.x];
  const PsgdSeg g = pl.segs[tile.x];
  const int rows = g.rows, cols = g.cols;
  const bool vec = vecok && g.vec;
  const int lane = tid & 63, wave = tid >> 6, l16 = lane & 15, kg = lane >> 4;
  const int mrow = tile.y * kPgTile + wave * 16, colbase = tile.z * kPgTile;
  f32x4 acc[4] = {};
  for (int k = 0; k < srcs.n; ++k) {
    const float* __restrict__ pp = reinterpret_cast<const float*>(srcs.p[k] + kPgHeader) + g.foff;
    psgd_outer(acc, pp, pp + (long)rows * r, rows, cols, r, mrow, colbase, l16, kg);
  }
  const int row = mrow + l16;
  if (row >= rows) return;
  float* __restrict__ dp = dst + g.offset + (long)row * cols;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int col = colbase + 16 * c + 4 * kg;
    if (col >= cols) continue;
    if (vec) {  // cols is a multiple of 4: col < cols covers col + 3
      f32x4 o = acc[c];
      if (!DECODE) o = *reinterpret_cast<const f32x4*>(dp + col) - o;
      else if (add) o = *reinterpret_cast<const f32x4*>(dp + col) + o;
      *reinterpret_cast<f32x4*>(dp + col) = o;
    } else {
#pragma unroll
      for (int v = 0; v < 4; ++v)
        if (col + v < cols) {
          float o = acc[c][v];
          if (!DECODE) o = dp[col + v] - o;
          else if (add) o = dp[col + v] + o;
          dp[col + v] = o;
        }
    }
  }
}

}  // namespace psx

using namespace psx;

static size_t psgd_payload_bytes(const PsgdPlan& pl) {
  return ((size_t)kPgHeader + 4 * (size_t)pl.factors + 2 * (size_t)pl.tails + 15) & ~(size_t)15;
}

// what both entries check of the table and the plan
static bool psgd_plan_ok(const PsgdPlan* pl, const void* table, int nseg, long n, int rank, long payload_bytes) {
  if (!pl || !table || n <= 0 || nseg <= 0) return false;
  if (rank != 4 && rank != 8 && rank != 12 && rank != 16) return false;
  if (pl->segs != table || pl->nseg != nseg || pl->ncomp < 0 || pl->ncomp > nseg) return false;
  if (pl->factors < 0 || pl->tails < 0 || pl->factors + pl->tails <= 0 || pl->wsfloats < 0) return false;
  if (pl->ncomp > 0 && (!pl->map_p || !pl->map_q || !pl->map_r || !pl->comp || pl->ntp <= 0 || pl->ntq <= 0 ||
                        pl->ntr <= 0 || pl->orth_floats <= 0 || pl->orth_floats > kPgLdsFloats))
    return false;
  if (pl->ncomp == 0 && (pl->ntp || pl->ntq || pl->ntr)) return false;
  if ((pl->ntt > 0) != (pl->tails > 0) || (pl->ntt > 0 && !pl->map_t)) return false;
  return payload_bytes == (long)psgd_payload_bytes(*pl);
}

extern "C" {

int psx_powersgd_seg_size() { return (int)sizeof(PsgdSeg); }
int psx_powersgd_plan_size() { return (int)sizeof(PsgdPlan); }
int psx_powersgd_lds_floats() { return kPgLdsFloats; }
int psx_powersgd_header_bytes() { return kPgHeader; }

// The encode of one push (the header comment): four launches on `st`, no host synchronisation.
//   g        : the gradient, fp16 or fp32 [n]
//   e        : fp32 [n] residual, read and replaced (tail tensors' elements are never touched)
//   table, nseg, plan : the PowerSGDTable of the layout for this rank
//   q        : fp32 [plan->factors], the worker's Q in the factor section's layout, read and replaced
//   payload  : payload_bytes bytes, 16-byte aligned; the 16-byte frame is the host's and is left alone
//   ws       : fp32 [plan->wsfloats + plan->ncomp] workspace
int psx_powersgd_encode(const void* g, int grad_fp16, float* e, long n, const void* table, int nseg,
                        const PsgdPlan* plan, int rank, float* q, uint8_t* payload, long payload_bytes, float* ws,
                        hipStream_t st) {
  if (!g || !e || !q || !payload || !ws || !psgd_plan_ok(plan, table, nseg, n, rank, payload_bytes))
    return (int)hipErrorInvalidValue;
  if (!al16(payload) || !al16(q) || !al16(ws)) return (int)hipErrorInvalidValue;
  const size_t esz = grad_fp16 ? 2 : 4;
  if (ranges_overlap(g, (size_t)n * esz, e, (size_t)n * 4) ||
      ranges_overlap(payload, (size_t)payload_bytes, e, (size_t)n * 4) ||
      ranges_overlap(payload, (size_t)payload_bytes, g, (size_t)n * esz))
    return (int)hipErrorInvalidValue;
  const PsgdPlan pl = *plan;
  const int vecok = al16(g) && al16(e);
  float* fac = reinterpret_cast<float*>(payload + kPgHeader);
  uint16_t* tail = reinterpret_cast<uint16_t*>(payload + kPgHeader + 4 * pl.factors);
  int* drop = reinterpret_cast<int*>(ws + pl.wsfloats);
  if (pl.ntp + pl.ntt > 0) {
    if (grad_fp16)
      hipLaunchKernelGGL((psgd_project_kernel<uint16_t>), dim3(pl.ntp + pl.ntt), dim3(256), 0, st, (const uint16_t*)g,
                         e, q, ws, tail, pl, rank, vecok);
    else
      hipLaunchKernelGGL((psgd_project_kernel<float>), dim3(pl.ntp + pl.ntt), dim3(256), 0, st, (const float*)g, e, q,
                         ws, tail, pl, rank, vecok);
  }
  int rc = (int)hipGetLastError();
  if (rc || pl.ncomp == 0) return rc;
  if (pl.orth_floats * 4 > 64 * 1024) {  // past the default limit of dynamic LDS (ResNet-50's 2048-row layers)
    rc = (int)hipFuncSetAttribute(reinterpret_cast<const void*>(psgd_orth_kernel),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, kPgLdsFloats * 4);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(psgd_orth_kernel, dim3(pl.ncomp), dim3(256), (size_t)pl.orth_floats * 4, st, ws, drop, fac, pl,
                     rank);
  hipLaunchKernelGGL(psgd_backproject_kernel, dim3(pl.ntq), dim3(256), 0, st, e, drop, fac, q, pl, rank, vecok);
  PsgdSrcs own{};
  own.p[0] = payload;
  own.n = 1;
  hipLaunchKernelGGL((psgd_outer_kernel<false>), dim3(pl.ntr), dim3(256), 0, st, e, own, pl, rank, 0, vecok);
  return (int)hipGetLastError();
}

// out = [out +] sum_w decode(payload_w) over nsrc payloads (host array of 1..32 device pointers,
// payload_bytes bytes each, 16-byte aligned) in list order: one launch on `st`. out: fp32 [n].
int psx_powersgd_decode(const void* const* payloads, int nsrc, long payload_bytes, float* out, long n,
                        const void* table, int nseg, const PsgdPlan* plan, int rank, int add, hipStream_t st) {
  if (!payloads || !out || nsrc < 1 || nsrc > kMaxSrc || !psgd_plan_ok(plan, table, nseg, n, rank, payload_bytes))
    return (int)hipErrorInvalidValue;
  PsgdSrcs sl{};
  sl.n = nsrc;
  for (int k = 0; k < nsrc; ++k) {
    const void* s = payloads[k];
    if (!s || !al16(s) || ranges_overlap(s, (size_t)payload_bytes, out, (size_t)n * 4)) return (int)hipErrorInvalidValue;
    sl.p[k] = (const uint8_t*)s;
  }
  const PsgdPlan pl = *plan;
  hipLaunchKernelGGL((psgd_outer_kernel<true>), dim3(pl.ntr + pl.ntt), dim3(256), 0, st, out, sl, pl, rank, add,
                     (int)al16(out));
  return (int)hipGetLastError();
}

}  // extern "C"
