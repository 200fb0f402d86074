// Muon server update (Jordan et al. 2024), --optimizer muon: Nesterov momentum, orthogonalised per
// weight matrix by a fixed Newton-Schulz polynomial on the exact-fp32 MFMA. For update number t,
// with s the fp32 sum of the W wires in list order (wire.hpp) and g = gscale * s:
//   b' = mu b + g;  u = g + mu b'                                   every element (mu = 0: u = g)
//   tensors with ndim > 1, read as the row-major rows x cols matrix U they are in the arena:
//     X = U / (|U|_F + 1e-7), transposed when rows > cols, so X is m x n with m <= n
//     `steps` times:  A = X X^T;  B = cb A + cc A A;  X = ca X + B X
//     w' = w (1 - lr wd) - lr sqrt(max(1, rows / cols)) O,  O = X in the tensor's orientation
//   1-D tensors:  w' = w - lr_aux u
//
// 1 + 3 * steps + 1 launches on the caller's stream, no host synchronisation:
//
//   muon_stage : the LARS grid of (tensor, chunk of kChunk) workgroups (lars_seg.hpp). Wire sum (or
//                the staged sum of the dense entry), momentum, u. A matrix tensor's u goes into the
//                X workspace in m x n orientation (tall tensors transposed on the way in) with one
//                sum u^2 double partial per workgroup; a 1-D tensor is stepped here, image included.
//   muon_gemm  : three launches per iteration, each one flat grid over every matrix tensor of the
//                model through a precomputed tile map {matrix, ti, tj, slab} (MuonPlan):
//                  SyrkA  A_slab = X[:, slab] X[:, slab]^T   K = n split into `slabs` slabs (two
//                         for a 512 x 4608 layer, whose 36 output tiles alone leave CUs idle);
//                  SyrkB  B = cb A + cc A A, A = the slabs summed in slab order while they are
//                         staged (and again in the epilogue): the split costs no launch;
//                  NN     X' = ca X + B X into the other X buffer.
//                Both SYRK forms compute the tiles with tj >= ti only and write the mirror (A is
//                symmetric bit for bit: the products of (i, j) and (j, i) are the same, in the
//                same order). 1 / (|U|_F + 1e-7) costs no pass: the first SyrkA scales its output
//                by its square and the first NN its output by it, every workgroup deriving it
//                from the tensor's partials (lars_tensor_sum2).
//   muon_apply : LARS grid; the matrix tensors' step from O, the bf16 image, |U|_F into ratios[t].
//
// One workgroup of 256 threads owns one 64 x 64 output tile: four waves of 32 x 32, each 2 x 2
// MFMA tiles issued through mma_tiles<2, 2, float> (v_mfma_f32_16x16x4_f32, no accumulator
// chains). Operands go global -> registers -> LDS 32 K at a time, the next step's loads in flight
// under this step's MFMAs. Both SYRK operands are K-contiguous rows, read from LDS as 16-byte
// fragments; the NN form's X tile is K-strided and read as four scalars per fragment.
//
// Padding: every workspace matrix is padded with zeros to 64 in both dimensions, so no main loop
// has a tail predicate. Zero rows and columns are a fixed point of the iteration, and every
// epilogue stores 0 outside m x m (m x n), so a non-finite gradient cannot poison the pads; the
// pads of X buffer 0 are stored by muon_stage itself, shared among the tensor's workgroups.
// Determinism: one owner per output element, fixed K order, slabs summed in slab order, no float
// atomics; reductions as lars.hip.
#include <math.h>

#include "lars_seg.hpp"

namespace psx {

constexpr int kMuTile = 64;           // output tile edge; workspace matrices are padded to it
constexpr int kMuKT = 32;             // K elements staged per main-loop step
constexpr int kMuLd = kMuKT + 4;      // LDS row stride of a [64][32] operand tile (16-byte rows, banks spread)
constexpr int kMuLdX = kMuTile + 4;   // LDS row stride of the NN form's [32][64] X tile
enum { kMuSyrkA = 0, kMuSyrkB = 1, kMuNN = 2 };

// one matrix tensor of the model (ops/kernels.py MuonTable builds the records)
struct MuonSeg {
  long offset;       // first arena element
  long xoff;         // its mp x np matrix in either X buffer (floats)
  long aoff;         // its `slabs` mp x mp slabs in the A workspace
  long boff;         // its mp x mp matrix in the B workspace
  int rows, cols;    // the tensor's own shape
  int m, n;          // working orientation, m <= n
  int mp, np;        // m, n padded to kMuTile
  int slabs, kslab;  // K = np of A = X X^T in `slabs` slabs of kslab (a multiple of kMuKT; the last may be short)
  int lars;          // its record in the LarsSeg table
  int tall;          // rows > cols: the workspace holds the transpose
};

struct MuonPlan {
  const MuonSeg* segs;
  const int* mat_of;  // LarsSeg index -> MuonSeg index, -1 for a 1-D tensor
  const int4* map_a;  // tile maps {matrix, ti, tj, slab} of the three forms
  const int4* map_b;
  const int4* map_n;
  float* x[2];        // X ping-pong
  float* a;
  float* b;
  int nmat, nta, ntb, ntn;
};

// where element (r, c) of the tensor sits in its workspace matrix
PSX_DEV long muon_at(const MuonSeg& g, unsigned r, unsigned c) {
  return g.tall ? (long)c * g.np + r : (long)r * g.np + c;
}

// 1 / (|U|_F + 1e-7) of a tensor from its partials (every thread gets it)
PSX_DEV float muon_scale(const LarsSeg& seg, const double* __restrict__ partials, double (*red)[4]) {
  double uu, z;
  lars_tensor_sum2(seg, partials, uu, z, red);
  return (float)(1.0 / (sqrt(uu) + 1e-7));
}

// GT: wire element. DENSE: s is already in `stage`. MOM: mu != 0 (buf given). VEC: 16-byte accesses.
// p null: the chain alone (psx_muon_orthogonalize), nothing is stepped.
template <typename GT, bool DENSE, bool MOM, bool VEC>
__global__ __launch_bounds__(256) void muon_stage_kernel(float* __restrict__ p, WireSrcs srcs,
                                                         float* __restrict__ stage, float* __restrict__ buf, long n,
                                                         const LarsSeg* __restrict__ table, int ntensors, int nblocks,
                                                         double* __restrict__ partials, MuonPlan pl, float gscale,
                                                         float mu, float lr_aux, uint16_t* __restrict__ img) {
  __shared__ int sh_t;
  __shared__ double red[2][4];
  const int t = lars_find(table, ntensors, nblocks, &sh_t);
  if (t < 0) return;  // block-uniform
  const LarsSeg seg = table[t];
  const ChunkRange r = chunk_range(seg.offset, seg.numel, blockIdx.x - seg.first_block, n);
  const int k = pl.mat_of[t];  // block-uniform
  MuonSeg g{};
  if (k >= 0) g = pl.segs[k];
  float* __restrict__ x = pl.x[0] + g.xoff;
  const unsigned cols = (unsigned)g.cols;
  if (k >= 0) {
    // the zero pads of X0: columns n .. np of the m live rows, then rows m .. mp whole; pad
    // element j belongs to workgroup (j / 256) % nchunks of the tensor
    const int nch = (int)((seg.numel + kChunk - 1) / kChunk), pc = g.np - g.n;
    const long side = (long)g.m * pc, pads = side + (long)(g.mp - g.m) * g.np;
    for (long j = (long)(blockIdx.x - seg.first_block) * 256 + threadIdx.x; j < pads; j += (long)nch * 256)
      x[j < side ? (j / pc) * g.np + g.n + j % pc : (long)g.m * g.np + (j - side)] = 0.f;
  }
  float uu = 0.f;
  // one element: the buffer advanced, u returned, its square summed
  auto tail = [&](float s, float& bv) {
    const float gr = gscale * s;
    float u = gr;
    if constexpr (MOM) {
      bv = __builtin_fmaf(mu, bv, gr);
      u = __builtin_fmaf(mu, bv, gr);
    }
    uu = __builtin_fmaf(u, u, uu);
    return u;
  };
  for_chunk<VEC>(
      r,
      [&](long i) {
        float s;
        if constexpr (DENSE) s = stage[i];
        else stage[i] = s = wire_sum1<GT>(srcs, i);
        float bv = 0.f;
        if constexpr (MOM) bv = buf[i];
        const float u = tail(s, bv);
        if constexpr (MOM) buf[i] = bv;
        if (k >= 0) {
          const unsigned e = (unsigned)(i - seg.offset), rr = e / cols;
          x[muon_at(g, rr, e - rr * cols)] = u;
        } else if (p) {
          const float nv = __builtin_fmaf(-lr_aux, u, p[i]);
          p[i] = nv;
          if (img) img[i] = f2bf(nv);
        }
      },
      [&](long i) {
        float s[8], bv[8], pv[8];
        if constexpr (DENSE) {
          ld8(stage + i, s);
        } else {
          wire_sum8<GT>(srcs, i, s);
          st8(stage + i, s);
        }
        if constexpr (MOM) ld8(buf + i, bv);
#pragma unroll
        for (int j = 0; j < 8; ++j) s[j] = tail(s[j], bv[j]);  // the scalar form's order
        if constexpr (MOM) st8(buf + i, bv);
        if (k >= 0) {
          const unsigned e = (unsigned)(i - seg.offset);
          unsigned rr = e / cols, cc = e - rr * cols;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            x[muon_at(g, rr, cc)] = s[j];
            if (++cc == cols) {
              cc = 0;
              ++rr;
            }
          }
        } else if (p) {
          ld8(p + i, pv);
#pragma unroll
          for (int j = 0; j < 8; ++j) pv[j] = __builtin_fmaf(-lr_aux, s[j], pv[j]);
          st8(p + i, pv);
          if (img) st_bf8(img + i, pv);
        }
      });
  double duu = (double)uu, z = 0.0;
  block_sum2_f64(duu, z, red);
  if (threadIdx.x == 0) {
    partials[2 * (long)blockIdx.x] = duu;
    partials[2 * (long)blockIdx.x + 1] = 0.0;
  }
}

// One 64 x 64 output tile of one matrix tensor (the header comment). alpha, beta: SyrkA stores
// beta sc^2 P P^T, SyrkB alpha P + beta P P^T, NN sc (alpha X + B X); sc = 1 unless `norm`.
template <int FORM>
__global__ __launch_bounds__(256) void muon_gemm_kernel(MuonPlan pl, const int4* __restrict__ map,
                                                        const float* __restrict__ xin, float* __restrict__ xout,
                                                        float alpha, float beta, int norm,
                                                        const LarsSeg* __restrict__ table,
                                                        const double* __restrict__ partials) {
  constexpr bool NN = FORM == kMuNN;
  __shared__ __attribute__((aligned(16))) float sa[kMuTile * kMuLd];
  __shared__ __attribute__((aligned(16))) float sb[NN ? kMuKT * kMuLdX : kMuTile * kMuLd];
  __shared__ double red[2][4];
  const int4 tile = map[blockIdx.x];
  const MuonSeg g = pl.segs[tile.x];
  const int ti = tile.y, tj = tile.z;
  float sc = 1.f;
  if (norm) sc = muon_scale(table[g.lars], partials, red);  // block-uniform

  const long mm = (long)g.mp * g.mp;  // one slab of A
  const float *pa, *pb;
  int ld, k0 = 0, k1 = g.mp;
  if constexpr (FORM == kMuSyrkA) {
    ld = g.np;
    pa = xin + g.xoff + (long)ti * kMuTile * ld;
    pb = xin + g.xoff + (long)tj * kMuTile * ld;
    k0 = tile.w * g.kslab;
    k1 = min(g.np, k0 + g.kslab);
  } else if constexpr (FORM == kMuSyrkB) {
    ld = g.mp;
    pa = pl.a + g.aoff + (long)ti * kMuTile * ld;
    pb = pl.a + g.aoff + (long)tj * kMuTile * ld;
  } else {
    ld = g.mp;
    pa = pl.b + g.boff + (long)ti * kMuTile * ld;
    pb = xin + g.xoff + (long)tj * kMuTile;  // rows are K here, stride np
  }
  // 16 bytes of a row operand; SyrkB's is the sum of A's slabs in slab order
  auto ldc = [&](const float* q) {
    f32x4 v = *reinterpret_cast<const f32x4*>(q);
    if constexpr (FORM == kMuSyrkB)
      for (int s = 1; s < g.slabs; ++s) v += *reinterpret_cast<const f32x4*>(q + s * mm);
    return v;
  };

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  const int l16 = lane & 15, kg = lane >> 4;
  f32x4 acc[2][2] = {};
  f32x4 ra[2], rb[2];
  auto fetch = [&](int k) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = tid + 256 * i;
      ra[i] = ldc(pa + (long)(c >> 3) * ld + k + 4 * (c & 7));
      if constexpr (NN) rb[i] = *reinterpret_cast<const f32x4*>(pb + (long)(k + (c >> 4)) * g.np + 4 * (c & 15));
      else rb[i] = ldc(pb + (long)(c >> 3) * ld + k + 4 * (c & 7));
    }
  };
  fetch(k0);
  for (int k = k0; k < k1; k += kMuKT) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = tid + 256 * i;
      *reinterpret_cast<f32x4*>(&sa[(c >> 3) * kMuLd + 4 * (c & 7)]) = ra[i];
      if constexpr (NN) *reinterpret_cast<f32x4*>(&sb[(c >> 4) * kMuLdX + 4 * (c & 15)]) = rb[i];
      else *reinterpret_cast<f32x4*>(&sb[(c >> 3) * kMuLd + 4 * (c & 7)]) = rb[i];
    }
    __syncthreads();
    if (k + kMuKT < k1) fetch(k + kMuKT);  // in flight under the MFMAs below
#pragma unroll
    for (int ks = 0; ks < kMuKT; ks += 16) {
      u32x4 fa[2], fb[2];
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        fa[q] = *reinterpret_cast<const u32x4*>(&sa[(wm * 32 + q * 16 + l16) * kMuLd + ks + 4 * kg]);
        if constexpr (NN) {
#pragma unroll
          for (int j = 0; j < 4; ++j) fb[q][j] = __float_as_uint(sb[(ks + 4 * kg + j) * kMuLdX + wn * 32 + q * 16 + l16]);
        } else {
          fb[q] = *reinterpret_cast<const u32x4*>(&sb[(wn * 32 + q * 16 + l16) * kMuLd + ks + 4 * kg]);
        }
      }
      mma_tiles<2, 2, float>(acc, fa, fb);
    }
    __syncthreads();
  }

  // epilogue: lane holds rows row0 .. row0 + 3 of column col of each 16 x 16 tile
  const int ldo = NN ? g.np : g.mp, nlim = NN ? g.n : g.m;
  float* out;
  if constexpr (FORM == kMuSyrkA) out = pl.a + g.aoff + tile.w * mm;
  else if constexpr (FORM == kMuSyrkB) out = pl.b + g.boff;
  else out = xout + g.xoff;
  const float s2 = beta * (sc * sc);
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int w = 0; w < 2; ++w) {
      const int row0 = ti * kMuTile + wm * 32 + q * 16 + 4 * kg, col = tj * kMuTile + wn * 32 + w * 16 + l16;
      f32x4 o;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const long at = (long)(row0 + v) * ldo + col;
        float val;
        if constexpr (FORM == kMuSyrkA) {
          val = s2 * acc[q][w][v];
        } else if constexpr (FORM == kMuSyrkB) {
          float pv = pl.a[g.aoff + at];
          for (int s = 1; s < g.slabs; ++s) pv += pl.a[g.aoff + s * mm + at];
          val = alpha * pv + beta * acc[q][w][v];
        } else {
          val = sc * (alpha * xin[g.xoff + at] + acc[q][w][v]);
        }
        o[v] = row0 + v < g.m && col < nlim ? val : 0.f;
        out[at] = o[v];
      }
      if constexpr (!NN)
        if (ti != tj) *reinterpret_cast<f32x4*>(&out[(long)col * ldo + row0]) = o;  // the mirror tile
    }
}

// raw: p receives O itself (psx_muon_orthogonalize)
template <bool VEC>
__global__ __launch_bounds__(256) void muon_apply_kernel(float* __restrict__ p, long n,
                                                         const LarsSeg* __restrict__ table, int ntensors, int nblocks,
                                                         const double* __restrict__ partials,
                                                         float* __restrict__ ratios, MuonPlan pl,
                                                         const float* __restrict__ xfin, float lr, float decay, int raw,
                                                         uint16_t* __restrict__ img) {
  __shared__ int sh_t;
  __shared__ double red[2][4];
  const int t = lars_find(table, ntensors, nblocks, &sh_t);
  if (t < 0) return;  // block-uniform
  const int k = pl.mat_of[t];
  if (k < 0) return;  // a 1-D tensor: muon_stage stepped it
  const LarsSeg seg = table[t];
  const MuonSeg g = pl.segs[k];
  const int chunk = blockIdx.x - seg.first_block;
  const ChunkRange r = chunk_range(seg.offset, seg.numel, chunk, n);
  if (chunk == 0) {  // block-uniform
    double uu, z;
    lars_tensor_sum2(seg, partials, uu, z, red);
    if (threadIdx.x == 0) ratios[t] = (float)sqrt(uu);
  }
  const float* __restrict__ x = xfin + g.xoff;
  const unsigned cols = (unsigned)g.cols;
  const float step = lr * sqrtf(fmaxf(1.f, (float)g.rows / (float)g.cols));
  auto upd = [&](float w, float o) { return __builtin_fmaf(-step, o, decay * w); };
  for_chunk<VEC>(
      r,
      [&](long i) {
        const unsigned e = (unsigned)(i - seg.offset), rr = e / cols;
        const float o = x[muon_at(g, rr, e - rr * cols)];
        const float nv = raw ? o : upd(p[i], o);
        p[i] = nv;
        if (img) img[i] = f2bf(nv);
      },
      [&](long i) {
        float pv[8] = {};
        if (!raw) ld8(p + i, pv);
        const unsigned e = (unsigned)(i - seg.offset);
        unsigned rr = e / cols, cc = e - rr * cols;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float o = x[muon_at(g, rr, cc)];
          pv[j] = raw ? o : upd(pv[j], o);
          if (++cc == cols) {
            cc = 0;
            ++rr;
          }
        }
        st8(p + i, pv);
        if (img) st_bf8(img + i, pv);
      });
}

}  // namespace psx

using namespace psx;

// the arguments every entry shares: the LARS table and scratch, the plan, the chain's length
static bool muon_args_ok(const void* p, const void* stage, long n, const void* table, int ntensors, int nblocks,
                         const void* partials, const void* ratios, const MuonPlan* pl, int steps) {
  if (!p || !stage || !table || !partials || !ratios || !pl || n <= 0 || ntensors <= 0 || nblocks <= 0 || steps < 1)
    return false;
  if (!pl->segs || !pl->mat_of || !pl->map_a || !pl->map_b || !pl->map_n || !pl->x[0] || !pl->x[1] || !pl->a || !pl->b)
    return false;
  if (pl->nmat <= 0 || pl->nmat > ntensors || pl->nta <= 0 || pl->ntb <= 0 || pl->ntn <= 0) return false;
  if (!al16(pl->x[0]) || !al16(pl->x[1]) || !al16(pl->a) || !al16(pl->b)) return false;
  return !ranges_overlap(p, (size_t)n * 4, stage, (size_t)n * 4);
}

// the momentum buffer: given exactly when mu != 0, disjoint from p and stage
static bool muon_buf_ok(const void* p, const void* stage, const void* buf, long n, float mu) {
  if ((mu != 0.f) != (buf != nullptr)) return false;
  const size_t nb = (size_t)n * 4;
  return !buf || (!ranges_overlap(buf, nb, p, nb) && !ranges_overlap(buf, nb, stage, nb));
}

// the 3 * steps launches of the chain; O ends in x[steps & 1]
static int muon_chain(const MuonPlan& pl, const LarsSeg* tb, const double* partials, int steps, float ca, float cb,
                      float cc, int normalize, hipStream_t st) {
  for (int it = 0; it < steps; ++it) {
    const float* xin = pl.x[it & 1];
    float* xout = pl.x[(it + 1) & 1];
    const int norm = normalize && it == 0;
    hipLaunchKernelGGL((muon_gemm_kernel<kMuSyrkA>), dim3(pl.nta), dim3(256), 0, st, pl, pl.map_a, xin, xout, 0.f, 1.f,
                       norm, tb, partials);
    hipLaunchKernelGGL((muon_gemm_kernel<kMuSyrkB>), dim3(pl.ntb), dim3(256), 0, st, pl, pl.map_b, xin, xout, cb, cc, 0,
                       tb, partials);
    hipLaunchKernelGGL((muon_gemm_kernel<kMuNN>), dim3(pl.ntn), dim3(256), 0, st, pl, pl.map_n, xin, xout, ca, 1.f,
                       norm, tb, partials);
    const int rc = (int)hipGetLastError();
    if (rc) return rc;
  }
  return 0;
}

static int muon_launch_apply(float* p, long n, const LarsSeg* tb, int ntensors, int nblocks, const double* partials,
                             float* ratios, const MuonPlan& pl, int steps, float lr, float wd, int raw, void* img,
                             hipStream_t st) {
  const float decay = 1.f - lr * wd;
  const float* xfin = pl.x[steps & 1];
  uint16_t* im = (uint16_t*)img;
  if (al16(p) && al16(img))
    hipLaunchKernelGGL((muon_apply_kernel<true>), dim3(nblocks), dim3(256), 0, st, p, n, tb, ntensors, nblocks, partials,
                       ratios, pl, xfin, lr, decay, raw, im);
  else
    hipLaunchKernelGGL((muon_apply_kernel<false>), dim3(nblocks), dim3(256), 0, st, p, n, tb, ntensors, nblocks,
                       partials, ratios, pl, xfin, lr, decay, raw, im);
  return (int)hipGetLastError();
}

extern "C" {

int psx_muon_seg_size() { return (int)sizeof(MuonSeg); }
int psx_muon_tile() { return kMuTile; }
int psx_muon_ktile() { return kMuKT; }

// The Muon update from nsrc gathered gradient wires (host array of 1..32 device pointers, all
// fp16 or all fp32, >= n elements each): 1 + 3 * steps + 1 launches on `st`, no host
// synchronisation.
//   stage    : fp32 [n], receives the wire sum s (must not alias a source)
//   buf      : fp32 [n] momentum buffer, read and replaced; null exactly when mu == 0
//   table, ntensors, nblocks, partials, ratios : as psx_lars_apply_multi; partials receives the
//              per-workgroup sum u^2, ratios |U|_F of the matrix tensors
//   plan     : the MuonPlan of the same layout (table, tile maps, workspaces)
//   lr_aux   : the 1-D tensors' learning rate
//   ca, cb, cc, steps : the Newton-Schulz polynomial and its number of iterations
//   normalize: 0 leaves X0 = U (scale 1)
//   img      : optional bf16 [n] image of the updated parameters
int psx_muon_apply_multi(float* p, const void* const* srcs, int nsrc, int grad_fp16, float* stage, float* buf, long n,
                         const void* table, int ntensors, int nblocks, double* partials, float* ratios,
                         const MuonPlan* plan, float lr, float lr_aux, float gscale, float mu, float wd, int steps,
                         float ca, float cb, float cc, int normalize, void* img, hipStream_t st) {
  if (!muon_args_ok(p, stage, n, table, ntensors, nblocks, partials, ratios, plan, steps) ||
      !muon_buf_ok(p, stage, buf, n, mu))
    return (int)hipErrorInvalidValue;
  WireSrcs sl{};
  bool vec = al16(p) && al16(stage) && al16(buf) && al16(img);
  if (!fill_srcs(srcs, nsrc, grad_fp16 ? 2 : 4, n, sl, vec, stage, {p, buf ? buf : p})) return (int)hipErrorInvalidValue;
  const LarsSeg* tb = (const LarsSeg*)table;
  const MuonPlan pl = *plan;
  uint16_t* im = (uint16_t*)img;
  dispatch2(grad_fp16 != 0, vec, [&](auto H, auto V) {
    using GT = wire_t<decltype(H)>;
    constexpr bool VE = decltype(V)::value;
    if (buf)
      hipLaunchKernelGGL((muon_stage_kernel<GT, false, true, VE>), dim3(nblocks), dim3(256), 0, st, p, sl, stage, buf, n,
                         tb, ntensors, nblocks, partials, pl, gscale, mu, lr_aux, im);
    else
      hipLaunchKernelGGL((muon_stage_kernel<GT, false, false, VE>), dim3(nblocks), dim3(256), 0, st, p, sl, stage, buf,
                         n, tb, ntensors, nblocks, partials, pl, gscale, mu, lr_aux, im);
  });
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  rc = muon_chain(pl, tb, partials, steps, ca, cb, cc, normalize, st);
  if (rc) return rc;
  return muon_launch_apply(p, n, tb, ntensors, nblocks, partials, ratios, pl, steps, lr, wd, 0, img, st);
}

// The dense entry: `stage` already holds the fp32 gradient sum (q8 / sign1 / top-k payloads
// decoded into it, or an accumulated round) and is left as it is; then the same launches.
int psx_muon_apply(float* p, float* stage, float* buf, long n, const void* table, int ntensors, int nblocks,
                   double* partials, float* ratios, const MuonPlan* plan, float lr, float lr_aux, float gscale,
                   float mu, float wd, int steps, float ca, float cb, float cc, int normalize, void* img,
                   hipStream_t st) {
  if (!muon_args_ok(p, stage, n, table, ntensors, nblocks, partials, ratios, plan, steps) ||
      !muon_buf_ok(p, stage, buf, n, mu))
    return (int)hipErrorInvalidValue;
  const WireSrcs sl{};
  const LarsSeg* tb = (const LarsSeg*)table;
  const MuonPlan pl = *plan;
  uint16_t* im = (uint16_t*)img;
  dispatch2(buf != nullptr, al16(p) && al16(stage) && al16(buf) && al16(img), [&](auto M, auto V) {
    hipLaunchKernelGGL((muon_stage_kernel<float, true, decltype(M)::value, decltype(V)::value>), dim3(nblocks),
                       dim3(256), 0, st, p, sl, stage, buf, n, tb, ntensors, nblocks, partials, pl, gscale, mu, lr_aux,
                       im);
  });
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  rc = muon_chain(pl, tb, partials, steps, ca, cb, cc, normalize, st);
  if (rc) return rc;
  return muon_launch_apply(p, n, tb, ntensors, nblocks, partials, ratios, pl, steps, lr, wd, 0, img, st);
}

// The chain alone: `in` holds the matrices of the table back to back (every tensor of the table a
// matrix), `out` receives O in the same places. The same 1 + 3 * steps + 1 launches.
int psx_muon_orthogonalize(float* in, float* out, long n, const void* table, int ntensors, int nblocks,
                           double* partials, float* ratios, const MuonPlan* plan, int steps, float ca, float cb,
                           float cc, int normalize, hipStream_t st) {
  if (!muon_args_ok(out, in, n, table, ntensors, nblocks, partials, ratios, plan, steps) || plan->nmat != ntensors)
    return (int)hipErrorInvalidValue;
  const WireSrcs sl{};
  const LarsSeg* tb = (const LarsSeg*)table;
  const MuonPlan pl = *plan;
  if (al16(in))
    hipLaunchKernelGGL((muon_stage_kernel<float, true, false, true>), dim3(nblocks), dim3(256), 0, st, (float*)nullptr,
                       sl, in, (float*)nullptr, n, tb, ntensors, nblocks, partials, pl, 1.f, 0.f, 0.f,
                       (uint16_t*)nullptr);
  else
    hipLaunchKernelGGL((muon_stage_kernel<float, true, false, false>), dim3(nblocks), dim3(256), 0, st, (float*)nullptr,
                       sl, in, (float*)nullptr, n, tb, ntensors, nblocks, partials, pl, 1.f, 0.f, 0.f,
                       (uint16_t*)nullptr);
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  rc = muon_chain(pl, tb, partials, steps, ca, cb, cc, normalize, st);
  if (rc) return rc;
  return muon_launch_apply(out, n, tb, ntensors, nblocks, partials, ratios, pl, steps, 1.f, 0.f, 1, nullptr, st);
}

}  // extern "C"
