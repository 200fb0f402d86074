// Weight-gradient implicit GEMM v2: dW[oc][k] = sum_pix dY[pix][oc] * im2col(X)[pix][k]
// (reduction over N*P*Q pixels, split-K over pixel ranges), LDS-DMA staged, 3-stage ring.
//
// Both operands are pixel-major in HBM, so the LDS tiles are pixel-major and the MFMA
// (v_mfma_f32_16x16x32_bf16) fragments along the pixel (reduction) axis are fetched with the
// gfx950 transposing LDS read ds_read_b64_tr_b16: im2col columns k are the MFMA's M rows, output
// channels its N columns, so a lane of a 16x16 tile holds 4 consecutive k of one oc.
//   * tiles up to 128 (k) x 128 (oc),
//   * global->LDS by global_load_lds with a per-lane im2col source address (padding = zero
//     page) and the transposed-read swizzle folded into the source address,
//   * pixel -> (n, oh, ow) and tap -> (r, s) by multiply-high division (no integer divide in
//     the main loop), 3 LDS stages with counted vmcnt waits and one barrier per 64 pixels.
// Partial sums go to fp32 slabs [split][OC][Kg] reduced by wgrad_reduce (wgrad_reduce.hip),
// which also permutes to OIHW and emits the fp16 wire codec.
#include <stdlib.h>

#include "pipeline.hpp"

namespace psx {

struct Wgrad2Args {
  const void* x;         // NHWC [Nb][IH][IW][IC] (bf16 bits, or fp32 for wgrad2f_kernel)
  const void* dy;        // NHWC [Nb][OH][OW][OC]
  float* part;           // [splits][OC][Kg]
  const void* zero;      // 16-byte zero page
  int IH, IW, IC, OC, R, S, pad, stride, Kg, log2_icc, npix;
  FastDiv div_ohw, div_ow, div_s;
  int n_k_tiles, n_oc_tiles, splits, steps_per_split;  // steps of 64 pixels
};

// pixel-major tile swizzle for the transposed reads: 128 B rows share a bank row in pairs, so the
// chunk index takes two bits of the row pair; 256 B rows put each row on its own bank row, so 8
// rows x 2 chunks need (r&7)<<1.
template <int ROWB>
PSX_DEV int pm2(int r, int c) {
  if constexpr (ROWB == 128) return r * 128 + ((c ^ (((r >> 1) & 3) << 1)) << 4);
  return r * 256 + ((c ^ ((r & 7) << 1)) << 4);
}

PSX_DEV s16x4 tr_read2(const unsigned char* base, int off) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base + off));
}

// wait until at most `ahead` later stage groups (PER DMA ops each) are still in flight
template <int PER, int MAXA>
PSX_DEV void wait_ahead(int ahead) {
  if constexpr (MAXA <= 0) {
    wait_vmcnt<0>();
  } else {
    if (ahead >= MAXA)
      wait_vmcnt<MAXA * PER>();
    else
      wait_ahead<PER, MAXA - 1>(ahead);
  }
}

template <int BR, int BC, int NS>
__global__ __launch_bounds__(256) void wgrad2_kernel(Wgrad2Args a) {
  constexpr int XROWB = BR * 2, DROWB = BC * 2;           // bytes per pixel row
  constexpr int XCPR = XROWB / 16, DCPR = DROWB / 16;     // 16-byte chunks per row
  constexpr int XRPI = 64 / XCPR, DRPI = 64 / DCPR;       // rows per DMA instruction
  constexpr int LX = 64 / XRPI / 4, LD = 64 / DRPI / 4;   // DMA instructions per wave per stage
  constexpr int XT = 64 * XROWB, DT = 64 * DROWB, STAGE = XT + DT;
  constexpr int MT = BR / 32, NT = BC / 32;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid >> 1, wn = wid & 1;
  const int ntile = a.n_k_tiles * a.n_oc_tiles;
  const int bid = xcd_remap(blockIdx.x, ntile * a.splits);
  const int split = bid / ntile, t = bid - split * ntile;
  const int oc_t = t % a.n_oc_tiles, k_t = t / a.n_oc_tiles;
  const int k0 = k_t * BR, oc0 = oc_t * BC;
  const int pbeg = split * a.steps_per_split * 64;
  const int nsteps = min(a.steps_per_split, (a.npix - pbeg + 63) / 64);

  // ---- per-lane DMA state ----
  // X: this lane's row within each instruction and its (logical) k-chunk -> tap / channel
  int xrow[LX], xtap_r[LX], xtap_s[LX], xc0[LX];
  bool xtap_ok[LX];
#pragma unroll
  for (int i = 0; i < LX; ++i) {
    const int row = (i * 4 + wid) * XRPI + lane / XCPR;
    const int pos = lane % XCPR;
    const int c = (XROWB == 128) ? (pos ^ (((row >> 1) & 3) << 1)) : (pos ^ ((row & 7) << 1));
    xrow[i] = row;
    const int gk = (k0 >> 3) + c;
    const int tap = gk >> a.log2_icc;
    xc0[i] = (gk & ((1 << a.log2_icc) - 1)) << 3;
    xtap_ok[i] = tap < a.R * a.S;
    const int r = fdiv(tap, a.div_s);
    xtap_r[i] = r;
    xtap_s[i] = tap - r * a.S;
  }
  int drow[LD], dchunk[LD];
#pragma unroll
  for (int i = 0; i < LD; ++i) {
    const int row = (i * 4 + wid) * DRPI + lane / DCPR;
    const int pos = lane % DCPR;
    drow[i] = row;
    dchunk[i] = (DROWB == 128) ? (pos ^ (((row >> 1) & 3) << 1)) : (pos ^ ((row & 7) << 1));
  }
  const int OW = a.div_ow.d;

  const uint16_t* const xg = (const uint16_t*)a.x;
  const uint16_t* const dyg = (const uint16_t*)a.dy;
  const uint16_t* const zero = (const uint16_t*)a.zero;
  // 1x1 / stride 1 / pad 0 (most of ResNet-50's weight gradients): output pixel == input pixel,
  // no (n, oh, ow) decomposition per staged row
  const bool ident = a.R == 1 && a.S == 1 && a.stride == 1 && a.pad == 0;
  auto issue = [&](int st, int stage) {
    unsigned char* base = smem + stage * STAGE;
    const int p0 = pbeg + st * 64;
#pragma unroll
    for (int i = 0; i < LX; ++i) {
      const int pix = p0 + xrow[i];
      const uint16_t* src = zero;
      if (ident) {
        if (pix < a.npix && xtap_ok[i]) src = xg + (size_t)pix * a.IC + xc0[i];
      } else if (pix < a.npix && xtap_ok[i]) {
        const int n = fdiv(pix, a.div_ohw);
        const int rem = pix - n * a.div_ohw.d;
        const int oh = fdiv(rem, a.div_ow);
        const int ow = rem - oh * OW;
        const int ih = oh * a.stride - a.pad + xtap_r[i], iw = ow * a.stride - a.pad + xtap_s[i];
        if ((unsigned)ih < (unsigned)a.IH && (unsigned)iw < (unsigned)a.IW)
          src = xg + ((size_t)(n * a.IH + ih) * a.IW + iw) * a.IC + xc0[i];
      }
      glds16(src, base + (i * 4 + wid) * 1024);
    }
#pragma unroll
    for (int i = 0; i < LD; ++i) {
      const int pix = p0 + drow[i];
      const uint16_t* src = pix < a.npix ? dyg + (size_t)pix * a.OC + oc0 + dchunk[i] * 8 : zero;
      glds16(src, base + XT + (i * 4 + wid) * 1024);
    }
  };

  f32x4 acc[MT][NT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[m][n] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // NS-stage ring: steps st+1 .. st+NS-2 may still be in flight while step st is consumed
#pragma unroll
  for (int i = 0; i < NS - 1; ++i)
    if (i < nsteps) issue(i, i);
  const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
  // unrolled by NS: compile-time stage offsets (see wgrad3_kernel)
  auto step = [&](const int st, auto sc) {
    constexpr int stage = decltype(sc)::value;
    wait_ahead<LX + LD, NS - 2>(min(NS - 2, nsteps - 1 - st));  // groups issued after step st's
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (st + NS - 1 < nsteps) issue(st + NS - 1, stage == 0 ? NS - 1 : stage - 1);
    const unsigned char* X = smem + stage * STAGE;
    const unsigned char* D = X + XT;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int row0 = kk * 32 + 4 * g + q, row1 = row0 + 16;
      bf16x8 fa[MT], fb[NT];
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        const int col = wm * (BR / 2) + m * 16 + 4 * p;
        const s16x4 lo = tr_read2(X, pm2<XROWB>(row0, col >> 3) + ((col & 7) << 1));
        const s16x4 hi = tr_read2(X, pm2<XROWB>(row1, col >> 3) + ((col & 7) << 1));
        fa[m] = __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
      }
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const int col = wn * (BC / 2) + n * 16 + 4 * p;
        const s16x4 lo = tr_read2(D, pm2<DROWB>(row0, col >> 3) + ((col & 7) << 1));
        const s16x4 hi = tr_read2(D, pm2<DROWB>(row1, col >> 3) + ((col & 7) << 1));
        fb[n] = __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
      }
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n)
          acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[m], fb[n], acc[m][n], 0, 0, 0);
    }
  };
  for (int st0 = 0; st0 < nsteps; st0 += NS)
    static_for<0, NS>([&](auto sc) {
      const int st = st0 + decltype(sc)::value;
      if (st < nsteps) step(st, sc);
    });

  float* part = a.part + (size_t)split * a.OC * a.Kg;
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const int k = k0 + wm * (BR / 2) + m * 16 + 4 * (lane >> 4);
      const int oc = oc0 + wn * (BC / 2) + n * 16 + (lane & 15);
      *reinterpret_cast<f32x4*>(part + (size_t)oc * a.Kg + k) = acc[m][n];
    }
}

// ---------------------------------------------------------------------------------------
// wgrad2f: the fp32 weight gradient (the reference's training precision). Same GEMM, grid and
// LDS-DMA ring as wgrad2_kernel, fp32 operands: a stage holds 32 pixels x (BR + BC) fp32 columns
// and the reduction runs on v_mfma_f32_16x16x4_f32 (exact f32). Its A/B fragments hold ONE
// element per lane (lane l: column l & 15 of pixel 4s + (l >> 4)), so the pixel-major tiles need
// no transposed read: one ds_read_b32 per operand per MFMA. Rows are 256/512 B (a multiple of
// the 32 banks), so the 16-byte chunk index is XOR-ed with bit 2 on odd rows (applied to the DMA
// source address, the LDS destination stays lane-linear): the two rows a 32-lane read group
// touches then sit 16 banks apart, conflict-free.
template <int BR, int BC, int NS>
__global__ __launch_bounds__(256) void wgrad2f_kernel(Wgrad2Args a) {
  constexpr int PS = 32;                                  // pixels per stage
  constexpr int XROWB = BR * 4, DROWB = BC * 4;           // bytes per pixel row
  constexpr int XCPR = XROWB / 16, DCPR = DROWB / 16;     // 16-byte chunks per row
  constexpr int XRPI = 64 / XCPR, DRPI = 64 / DCPR;       // rows per DMA instruction
  constexpr int LX = PS / XRPI / 4, LD = PS / DRPI / 4;   // DMA instructions per wave per stage
  constexpr int XT = PS * XROWB, DT = PS * DROWB, STAGE = XT + DT;
  constexpr int MT = BR / 32, NT = BC / 32;
  static_assert(LX >= 1 && LD >= 1, "tile too narrow for the 32-pixel stage");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid >> 1, wn = wid & 1;
  const int ntile = a.n_k_tiles * a.n_oc_tiles;
  const int bid = xcd_remap(blockIdx.x, ntile * a.splits);
  const int split = bid / ntile, t = bid - split * ntile;
  const int oc_t = t % a.n_oc_tiles, k_t = t / a.n_oc_tiles;
  const int k0 = k_t * BR, oc0 = oc_t * BC;
  const int pbeg = split * a.steps_per_split * PS;
  const int nsteps = min(a.steps_per_split, (a.npix - pbeg + PS - 1) / PS);
  const float* const xg = (const float*)a.x;
  const float* const dyg = (const float*)a.dy;
  const float* const zero = (const float*)a.zero;

  int xrow[LX], xtap_r[LX], xtap_s[LX], xc0[LX];
  bool xtap_ok[LX];
#pragma unroll
  for (int i = 0; i < LX; ++i) {
    const int row = (i * 4 + wid) * XRPI + lane / XCPR;
    const int c = (lane % XCPR) ^ ((row & 1) << 2);  // logical chunk of this lane's slot
    xrow[i] = row;
    const int gk = (k0 >> 2) + c;
    const int tap = gk >> a.log2_icc;
    xc0[i] = (gk & ((1 << a.log2_icc) - 1)) << 2;
    xtap_ok[i] = tap < a.R * a.S;
    const int r = fdiv(tap, a.div_s);
    xtap_r[i] = r;
    xtap_s[i] = tap - r * a.S;
  }
  int drow[LD], dchunk[LD];
#pragma unroll
  for (int i = 0; i < LD; ++i) {
    const int row = (i * 4 + wid) * DRPI + lane / DCPR;
    drow[i] = row;
    dchunk[i] = (lane % DCPR) ^ ((row & 1) << 2);
  }
  const int OW = a.div_ow.d;
  const bool ident = a.R == 1 && a.S == 1 && a.stride == 1 && a.pad == 0;  // (see wgrad2_kernel)

  auto issue = [&](int st, int stage) {
    unsigned char* base = smem + stage * STAGE;
    const int p0 = pbeg + st * PS;
#pragma unroll
    for (int i = 0; i < LX; ++i) {
      const int pix = p0 + xrow[i];
      const float* src = zero;
      if (ident) {
        if (pix < a.npix && xtap_ok[i]) src = xg + (size_t)pix * a.IC + xc0[i];
      } else if (pix < a.npix && xtap_ok[i]) {
        const int n = fdiv(pix, a.div_ohw);
        const int rem = pix - n * a.div_ohw.d;
        const int oh = fdiv(rem, a.div_ow);
        const int ow = rem - oh * OW;
        const int ih = oh * a.stride - a.pad + xtap_r[i], iw = ow * a.stride - a.pad + xtap_s[i];
        if ((unsigned)ih < (unsigned)a.IH && (unsigned)iw < (unsigned)a.IW)
          src = xg + ((size_t)(n * a.IH + ih) * a.IW + iw) * a.IC + xc0[i];
      }
      glds16(src, base + (i * 4 + wid) * 1024);
    }
#pragma unroll
    for (int i = 0; i < LD; ++i) {
      const int pix = p0 + drow[i];
      const float* src = pix < a.npix ? dyg + (size_t)pix * a.OC + oc0 + dchunk[i] * 4 : zero;
      glds16(src, base + XT + (i * 4 + wid) * 1024);
    }
  };

  f32x4 acc[MT][NT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[m][n] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // per-lane fragment byte offsets within a row (odd rows: chunk bit 2 flipped)
  const int kq = lane >> 4, col = lane & 15;
  int aoff[MT], boff[NT];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int c = wm * (BR / 2) + m * 16 + col;
    aoff[m] = (((c >> 2) ^ ((kq & 1) << 2)) << 4) + ((c & 3) << 2);
  }
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const int c = wn * (BC / 2) + n * 16 + col;
    boff[n] = (((c >> 2) ^ ((kq & 1) << 2)) << 4) + ((c & 3) << 2);
  }

#pragma unroll
  for (int i = 0; i < NS - 1; ++i)
    if (i < nsteps) issue(i, i);
  // unrolled by NS: compile-time stage offsets (see wgrad3_kernel)
  auto step = [&](const int st, auto sc) {
    constexpr int stage = decltype(sc)::value;
    wait_ahead<LX + LD, NS - 2>(min(NS - 2, nsteps - 1 - st));
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (st + NS - 1 < nsteps) issue(st + NS - 1, stage == 0 ? NS - 1 : stage - 1);
    const unsigned char* X = smem + stage * STAGE;
    const unsigned char* D = X + XT;
#pragma unroll
    for (int s4 = 0; s4 < PS / 4; ++s4) {
      const int row = 4 * s4 + kq;
      float fa[MT], fb[NT];
#pragma unroll
      for (int m = 0; m < MT; ++m) fa[m] = *reinterpret_cast<const float*>(X + row * XROWB + aoff[m]);
#pragma unroll
      for (int n = 0; n < NT; ++n) fb[n] = *reinterpret_cast<const float*>(D + row * DROWB + boff[n]);
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n)
          acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[m], fb[n], acc[m][n], 0, 0, 0);
    }
  };
  for (int st0 = 0; st0 < nsteps; st0 += NS)
    static_for<0, NS>([&](auto sc) {
      const int st = st0 + decltype(sc)::value;
      if (st < nsteps) step(st, sc);
    });

  float* part = a.part + (size_t)split * a.OC * a.Kg;
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const int k = k0 + wm * (BR / 2) + m * 16 + 4 * (lane >> 4);
      const int oc = oc0 + wn * (BC / 2) + n * 16 + (lane & 15);
      *reinterpret_cast<f32x4*>(part + (size_t)oc * a.Kg + k) = acc[m][n];
    }
}

// ---------------------------------------------------------------------------------------
// wgrad3: 3x3 / stride 1 / pad 1 with tap reuse. For one kernel row r, the three taps s=0,1,2
// read the same input row shifted by -1/0/+1 pixels, so one LDS window of 64 input pixels
// x(n, oh+r-1, ow) (plus one zero row for the row edges) feeds a 192-row output tile
// (3 taps x 64 channels) instead of three 64-row tiles each gathering its own copy. Each lane's
// transposed-read address picks slot (pixel + s - 1), or the zero row when ow + s - 1 leaves
// the image row; 64-pixel steps hold whole rows because W is a power of two <= 64. Staged
// bytes per step stay ~16 KB while the MFMA work per step triples (wgrad2 is LDS-DMA bound).
// G (general widths, e.g. ResNet-50's 56 / 28 / 14 / 7): a step takes PIX = 56 pixels — whole
// rows of any W dividing 56 — in the 64-row tiles; rows 56..63 are zero on both operands (1/8 of
// the MFMA work idle), pixel -> (oh, ow) by multiply-high division.
struct Wgrad3Args {
  const void* x;         // NHWC [Nb][H][W][IC] (bf16 bits, or fp32 for wgrad3f_kernel)
  const void* dy;        // NHWC [Nb][H][W][OC]
  float* part;           // [splits][OC][Kg]
  const void* zero;      // 16-byte zero page
  int H, W, log2w, IC, OC, Kg, npix;
  int n_c_tiles, n_oc_tiles, splits, steps_per_split;
  int pix;               // pixels per step (G: 56)
  FastDiv div_w, div_h;  // (G)
};

template <int BC, int NS, bool G>
__global__ __launch_bounds__(256) void wgrad3_kernel(Wgrad3Args a) {
  constexpr int DROWB = BC * 2, DCPR = DROWB / 16, DRPI = 64 / DCPR, LD = 64 / DRPI / 4;
  constexpr int XT = 65 * 128, DT = 64 * DROWB, STAGE = XT + DT;
  constexpr int NT = BC / 32;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid >> 1, wn = wid & 1;
  const int ntile = 3 * a.n_c_tiles * a.n_oc_tiles;
  const int bid = xcd_remap(blockIdx.x, ntile * a.splits);
  const int split = bid / ntile, t = bid - split * ntile;
  const int oc_t = t % a.n_oc_tiles, rest = t / a.n_oc_tiles;
  const int c_t = rest % a.n_c_tiles, r = rest / a.n_c_tiles;
  const int c0 = c_t * 64, oc0 = oc_t * BC;
  const int PIX = G ? a.pix : 64;
  const int pbeg = split * a.steps_per_split * PIX;
  const int nsteps = min(a.steps_per_split, (a.npix - pbeg + PIX - 1) / PIX);
  const int W = a.W;
  const uint16_t* const xg = (const uint16_t*)a.x;
  const uint16_t* const dyg = (const uint16_t*)a.dy;
  const uint16_t* const zero = (const uint16_t*)a.zero;

  // zero row (slot 64) of every stage; the DMA never writes it
  if (tid < NS * 8) *reinterpret_cast<uint4*>(smem + (tid >> 3) * STAGE + 64 * 128 + (tid & 7) * 16) = uint4{0, 0, 0, 0};

  // ---- per-lane DMA state ----
  int xrow[2], xcol[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = (i * 4 + wid) * 8 + (lane >> 3);
    xrow[i] = row;
    xcol[i] = c0 + (((lane & 7) ^ (((row >> 1) & 3) << 1)) << 3);
  }
  int drow[LD], dchunk[LD];
#pragma unroll
  for (int i = 0; i < LD; ++i) {
    const int row = (i * 4 + wid) * DRPI + lane / DCPR;
    const int pos = lane % DCPR;
    drow[i] = row;
    dchunk[i] = (DROWB == 128) ? (pos ^ (((row >> 1) & 3) << 1)) : (pos ^ ((row & 7) << 1));
  }
  const long xshift = (long)(r - 1) * W;

  auto issue = [&](int st, int stage) {
    unsigned char* base = smem + stage * STAGE;
    const int p0 = pbeg + st * PIX;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int pix = p0 + xrow[i];
      int ih;
      if constexpr (G) {
        const int q = fdiv(pix, a.div_w);
        ih = q - fdiv(q, a.div_h) * a.H + r - 1;
      } else {
        ih = ((pix >> a.log2w) & (a.H - 1)) + r - 1;
      }
      const uint16_t* src = zero;
      if ((!G || xrow[i] < PIX) && pix < a.npix && (unsigned)ih < (unsigned)a.H)
        src = xg + ((long)pix + xshift) * a.IC + xcol[i];
      glds16(src, base + (i * 4 + wid) * 1024);
    }
#pragma unroll
    for (int i = 0; i < LD; ++i) {
      const int pix = p0 + drow[i];
      const bool ok = (!G || drow[i] < PIX) && pix < a.npix;
      const uint16_t* src = ok ? dyg + (size_t)pix * a.OC + oc0 + dchunk[i] * 8 : zero;
      glds16(src, base + XT + (i * 4 + wid) * 1024);
    }
  };

  // per-lane window slots: logical K row (pixel) -> physical LDS row for tap s
  const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
  int soff[2][2][3], sxr[2][2][3];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int row = kk * 32 + h * 16 + 4 * g + q;
      const int ow = G ? row - fdiv(row, a.div_w) * W : row & (W - 1);
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        const int iw = ow + s - 1;
        const int slot = ((!G || row < PIX) && (unsigned)iw < (unsigned)W) ? row + s - 1 : 64;
        soff[kk][h][s] = slot * 128 + ((4 * p & 7) << 1);
        sxr[kk][h][s] = ((slot >> 1) & 3) << 1;
      }
    }

  f32x4 acc[6][NT];
#pragma unroll
  for (int m = 0; m < 6; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[m][n] = (f32x4){0.f, 0.f, 0.f, 0.f};

  __syncthreads();
#pragma unroll
  for (int i = 0; i < NS - 1; ++i)
    if (i < nsteps) issue(i, i);
  // The step loop is unrolled by NS so that every step's stage is a compile-time constant: the
  // fragment reads then address LDS as per-lane offsets hoisted out of the loop + an immediate
  // (a runtime stage base cost one v_add per read, ~2 of wgrad3's 5.3 VALU per MFMA).
  auto step = [&](const int st, auto sc) {
    constexpr int stage = decltype(sc)::value;
    wait_ahead<2 + LD, NS - 2>(min(NS - 2, nsteps - 1 - st));
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (st + NS - 1 < nsteps) issue(st + NS - 1, stage == 0 ? NS - 1 : stage - 1);
    const unsigned char* X = smem + stage * STAGE;
    const unsigned char* D = X + XT;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int row0 = kk * 32 + 4 * g + q, row1 = row0 + 16;
      bf16x8 fa[6], fb[NT];
#pragma unroll
      for (int m = 0; m < 6; ++m) {
        const int s = m >> 1;
        const int cc = ((wm * 32 + (m & 1) * 16) >> 3) + (p >> 1);  // 16-byte chunk of the channel
        const s16x4 lo = tr_read2(X, soff[kk][0][s] + ((cc ^ sxr[kk][0][s]) << 4));
        const s16x4 hi = tr_read2(X, soff[kk][1][s] + ((cc ^ sxr[kk][1][s]) << 4));
        fa[m] = __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
      }
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const int col = wn * (BC / 2) + n * 16 + 4 * p;
        const s16x4 lo = tr_read2(D, pm2<DROWB>(row0, col >> 3) + ((col & 7) << 1));
        const s16x4 hi = tr_read2(D, pm2<DROWB>(row1, col >> 3) + ((col & 7) << 1));
        fb[n] = __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
      }
#pragma unroll
      for (int m = 0; m < 6; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n)
          acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[m], fb[n], acc[m][n], 0, 0, 0);
    }
  };
  for (int st0 = 0; st0 < nsteps; st0 += NS)
    static_for<0, NS>([&](auto sc) {
      const int st = st0 + decltype(sc)::value;
      if (st < nsteps) step(st, sc);
    });

  float* part = a.part + (size_t)split * a.OC * a.Kg;
#pragma unroll
  for (int m = 0; m < 6; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const int k = (r * 3 + (m >> 1)) * a.IC + c0 + wm * 32 + (m & 1) * 16 + 4 * (lane >> 4);
      const int oc = oc0 + wn * (BC / 2) + n * 16 + (lane & 15);
      *reinterpret_cast<f32x4*>(part + (size_t)oc * a.Kg + k) = acc[m][n];
    }
}

// ---------------------------------------------------------------------------------------
// wgrad3f: the fp32 tap-reuse weight gradient (3x3 / stride 1 / pad 1, power-of-two W <= 32).
// Same decomposition as wgrad3 — one workgroup = kernel row r x 64 input channels x BC output
// channels x a pixel range, its 192-row tile covering the taps s = 0, 1, 2 — on the exact-f32
// v_mfma_f32_16x16x4_f32. A stage holds 32 pixels (whole image rows: W divides 32) of x shifted
// by r - 1 rows and of dy; the A fragment of tap s is the x window read one slot left / in place /
// one slot right (lane l: channel l & 15 of pixel 4k + (l >> 4) + s - 1). Slots that leave the
// image row (ow + s - 1 outside [0, W)) are zeroed in registers from a per-lane bit mask over the
// 8 k-steps, computed once. Compared with wgrad2f (64x64 tiles, one tap per row) the MFMA work
// per staged byte triples: x is staged once per kernel row instead of once per tap. Rows are
// 256 B (x) / 256-512 B (dy); the 16-byte chunk index is XOR-ed with bit 2 on odd slots (in the
// DMA source address), so the two slots a 32-lane read group touches sit 16 banks apart. A
// 256-byte guard row in front of every stage's x tile absorbs the masked slot -1 read.
template <int BC, int NS>
__global__ __launch_bounds__(256) void wgrad3f_kernel(Wgrad3Args a) {
  constexpr int PS = 32;
  constexpr int DROWB = BC * 4, DCPR = DROWB / 16, DRPI = 64 / DCPR;
  constexpr int LX = PS / 4 / 4, LD = PS / DRPI / 4;  // DMA instructions per wave per stage
  constexpr int GUARD = 256, XT = PS * 256, DT = PS * DROWB, STAGE = GUARD + XT + DT;
  constexpr int NT = BC / 32;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid >> 1, wn = wid & 1;
  const int ntile = 3 * a.n_c_tiles * a.n_oc_tiles;
  const int bid = xcd_remap(blockIdx.x, ntile * a.splits);
  const int split = bid / ntile, t = bid - split * ntile;
  const int oc_t = t % a.n_oc_tiles, rest = t / a.n_oc_tiles;
  const int c_t = rest % a.n_c_tiles, r = rest / a.n_c_tiles;
  const int c0 = c_t * 64, oc0 = oc_t * BC;
  const int pbeg = split * a.steps_per_split * PS;
  const int nsteps = min(a.steps_per_split, (a.npix - pbeg) / PS);
  const int W = a.W;
  const float* const xg = (const float*)a.x;
  const float* const dyg = (const float*)a.dy;
  const float* const zero = (const float*)a.zero;

  // ---- per-lane DMA state ----
  int xrow[LX], xcol[LX];
#pragma unroll
  for (int i = 0; i < LX; ++i) {
    const int row = (i * 4 + wid) * 4 + (lane >> 4);
    xrow[i] = row;
    xcol[i] = c0 + (((lane & 15) ^ ((row & 1) << 2)) << 2);
  }
  int drow[LD], dcol[LD];
#pragma unroll
  for (int i = 0; i < LD; ++i) {
    const int row = (i * 4 + wid) * DRPI + lane / DCPR;
    drow[i] = row;
    dcol[i] = oc0 + (((lane % DCPR) ^ ((row & 1) << 2)) << 2);
  }
  const long xshift = (long)(r - 1) * W;

  auto issue = [&](int st, int stage) {
    unsigned char* base = smem + stage * STAGE + GUARD;
    const int p0 = pbeg + st * PS;
#pragma unroll
    for (int i = 0; i < LX; ++i) {
      const int pix = p0 + xrow[i];
      const int ih = ((pix >> a.log2w) & (a.H - 1)) + r - 1;
      const float* src = (unsigned)ih < (unsigned)a.H ? xg + ((long)pix + xshift) * a.IC + xcol[i] : zero;
      glds16(src, base + (i * 4 + wid) * 1024);
    }
#pragma unroll
    for (int i = 0; i < LD; ++i) glds16(dyg + (size_t)(p0 + drow[i]) * a.OC + dcol[i], base + XT + (i * 4 + wid) * 1024);
  };

  // per-lane fragment offsets (relative to the k-step's first slot row) and tap masks
  const int kq = lane >> 4, col = lane & 15;
  int aoff[3][2], boff[NT];
#pragma unroll
  for (int s = 0; s < 3; ++s)
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int c = wm * 32 + m * 16 + col;
      aoff[s][m] = (kq + s - 1) * 256 + ((((c >> 2) ^ (((kq + s + 1) & 1) << 2)) << 4) + ((c & 3) << 2));
    }
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const int c = wn * (BC / 2) + n * 16 + col;
    boff[n] = kq * DROWB + ((((c >> 2) ^ ((kq & 1) << 2)) << 4) + ((c & 3) << 2));
  }
  unsigned lmask = 0, rmask = 0;  // bit k: slot of tap 0 / tap 2 inside the image row at k-step k
#pragma unroll
  for (int k = 0; k < PS / 4; ++k) {
    const int ow = (4 * k + kq) & (W - 1);
    lmask |= (ow != 0 ? 1u : 0u) << k;
    rmask |= (ow != W - 1 ? 1u : 0u) << k;
  }

  f32x4 acc[3][2][NT];
#pragma unroll
  for (int s = 0; s < 3; ++s)
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < NT; ++n) acc[s][m][n] = (f32x4){0.f, 0.f, 0.f, 0.f};

#pragma unroll
  for (int i = 0; i < NS - 1; ++i)
    if (i < nsteps) issue(i, i);
  int stage = 0;
  for (int st = 0; st < nsteps; ++st) {
    wait_ahead<LX + LD, NS - 2>(min(NS - 2, nsteps - 1 - st));
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (st + NS - 1 < nsteps) issue(st + NS - 1, stage == 0 ? NS - 1 : stage - 1);
    const unsigned char* X = smem + stage * STAGE + GUARD;
    const unsigned char* D = X + XT;
#pragma unroll
    for (int k = 0; k < PS / 4; ++k) {
      float fa[3][2], fb[NT];
#pragma unroll
      for (int s = 0; s < 3; ++s)
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          const float v = *reinterpret_cast<const float*>(X + k * 1024 + aoff[s][m]);
          fa[s][m] = s == 1 ? v : (((s == 0 ? lmask : rmask) >> k) & 1u) ? v : 0.f;
        }
#pragma unroll
      for (int n = 0; n < NT; ++n) fb[n] = *reinterpret_cast<const float*>(D + k * 4 * DROWB + boff[n]);
#pragma unroll
      for (int s = 0; s < 3; ++s)
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
          for (int n = 0; n < NT; ++n)
            acc[s][m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[s][m], fb[n], acc[s][m][n], 0, 0, 0);
    }
    stage = stage == NS - 1 ? 0 : stage + 1;
  }

  float* part = a.part + (size_t)split * a.OC * a.Kg;
#pragma unroll
  for (int s = 0; s < 3; ++s)
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const int k = (r * 3 + s) * a.IC + c0 + wm * 32 + m * 16 + 4 * (lane >> 4);
        const int oc = oc0 + wn * (BC / 2) + n * 16 + (lane & 15);
        *reinterpret_cast<f32x4*>(part + (size_t)oc * a.Kg + k) = acc[s][m][n];
      }
}

}  // namespace psx

using namespace psx;

extern "C" int psx_stem7_wgrad(const float* x, const float* dy, float* part, int Nb, int IH, int IW, int cin, int cp,
                               int OC, int Kg, hipStream_t st);

namespace {

struct WGeom {
  int Nb, H, W, IC, OC, R, S, stride, pad, Kg;
  int OH() const { return (H + 2 * pad - R) / stride + 1; }
  int OW() const { return (W + 2 * pad - S) / stride + 1; }
  int npix() const { return Nb * OH() * OW(); }
};

// The launch decision of one weight gradient: which kernel family (kind, f32), which instantiation
// (BR x BC tile, NS ring stages), how many splits of how many pixel-steps. Made once per call by
// route_wgrad from the geometry alone; psx_conv_wgrad2 launches what it says and
// psx_conv_wgrad2_path reports it, so the two cannot drift.
enum { kTile = 0, kTap = 1, kTapG = 2, kStem7 = 3 };
struct WRoute {
  int kind;         // kTile wgrad2[f]_kernel, kTap / kTapG wgrad3[f]_kernel (G: general widths), kStem7 stem.hip
  int f32;
  int BR, BC, NS;   // tap reuse: BR = 192 (3 taps x 64 channels); stem7: 0
  int splits, sps;  // sps: pixel-steps per split
  int pix;          // pixels per step
};

// Workgroup slots of the chip the weight gradient plans for (256 CUs x occupancy).
int wg_slots(int occ) { return 256 * occ; }

// LDS bytes per workgroup: an NS-stage BR x BC tile of 64 bf16 / 32 fp32 pixels per stage, and the
// tap-reuse tiles (x window of 64 channels + zero row / guard row, dy BC wide).
constexpr int wlds(int BR, int BC, int NS) { return NS * 64 * (BR + BC) * 2; }
constexpr int wldsf(int BR, int BC, int NS) { return NS * 32 * (BR + BC) * 4; }
constexpr int wlds3(int BC, int NS) { return NS * (65 * 128 + 64 * BC * 2); }
constexpr int wlds3f(int BC, int NS) { return NS * (256 + 32 * 256 + 32 * BC * 4); }

// Workgroups per CU that the LDS allows, at most 3.
int wocc(int lds) { return 163840 / lds > 3 ? 3 : 163840 / lds; }

// One tile shape that a planner weighs: occ workgroups of it share a CU, `tiles` of them cover
// dW, a pixel-step of one takes step_us. eff (fp32 model): MFMA efficiency at 1 / 2 / 3
// co-resident workgroups.
struct WCand {
  int BR, BC, NS, occ;
  long tiles;
  double step_us;
  const double* eff;
};
using WCost = double (*)(const WCand& c, int OC, int Kg, int spl, int sps);

// bf16 round model: tiles x splits workgroups fill whole rounds of the 256 CUs x (workgroups per
// CU that the LDS allows); +3 us prologue/epilogue per workgroup; split-K partials cost a write +
// a read at ~5 TB/s.
double wcost_bf16(const WCand& c, int OC, int Kg, int spl, int sps) {
  const int slots = wg_slots(c.occ);
  const long wgs = c.tiles * spl;
  const long rounds = (wgs + slots - 1) / slots;
  return rounds * (sps * c.step_us + 3.0) + (spl > 1 ? spl * (double)OC * Kg * 8.0 / 5e6 : 0.0);
}

// fp32 round model: workgroups run in rounds of 256 CUs x k co-resident workgroups (k <= the LDS
// occupancy); a round's length is its workgroups' stages x the f32 MFMA time of a stage x
// k / eff(k) — a lone wave per SIMD leaves every stage's DMA wait and barrier exposed — plus
// ~1.5 us of prologue / partial-tile store, and the split-K partial traffic (written here, read by
// the reduction) comes on top. Round quantisation dominates: the 64-channel 32x32 layer takes
// 100 us at 84 splits (756 workgroups: one round at k = 3) and 131 us at 86 (774: a second round
// for 6 workgroups).
double wcost_f32(const WCand& c, int OC, int Kg, int spl, int sps) {
  auto eff = [&](int k) { return c.eff[k <= 1 ? 0 : k == 2 ? 1 : 2]; };
  const long wgs = c.tiles * spl, full = wgs / (256L * c.occ), rest = wgs - full * 256L * c.occ;
  const int krest = (int)((rest + 255) / 256);
  double t = full * (sps * c.step_us * c.occ / eff(c.occ) + 1.5);
  if (rest) t += sps * c.step_us * krest / eff(krest) + 1.5;
  if (spl > 1) t += spl * (double)OC * Kg * 6.0 / 6e6;  // reduction read + extra store
  return t;
}

void wset(WRoute& r, int BR, int BC, int NS, int splits, int sps) {
  r.BR = BR; r.BC = BC; r.NS = NS; r.splits = splits; r.sps = sps;
}

// The split search of every planner: sp = 1 .. smax pixel ranges of one candidate, the first
// with the strictly lowest modelled time (over all candidates so far: best_t) goes into r.
// equal: only split counts that give equal ranges (sp ranges of sps steps leave none empty; the
// fp32 planners' filter).
void wsearch(WRoute& r, double& best_t, const WCand& c, WCost cost, bool equal, int OC, int Kg, int steps, int smax) {
  if (c.occ < 1) return;
  for (int sp = 1; sp <= smax; ++sp) {
    const int sps = (steps + sp - 1) / sp;
    const int spl = (steps + sps - 1) / sps;
    if (equal && sp > 1 && spl != sp) continue;
    const double t = cost(c, OC, Kg, spl, sps);
    if (t < best_t) {
      best_t = t;
      wset(r, c.BR, c.BC, c.NS, spl, sps);
    }
  }
}

// bf16 tile plan: >= 8 pixel-steps per split; among the tile shapes the one with the lowest
// modelled time wins (per-step costs measured on MI355X with rocprofv3: 128x128 ~1.2 us at
// 1 WG/CU, 64x64 ~0.7 us at 3 WG/CU). fbr / fbc (> 0): only that tile (its split count still from
// the model). Split cap 256 (64 until round 6: ResNet-50's 56x56 1x1 layers sat at it with ~98
// steps per workgroup; 256 measured -2 % on its bf16 step, profiles/r6_wgrad_split_cap_ab.jsonl).
void wplan(WRoute& r, int OC, int Kg, int npix, int fbr, int fbc) {
  wset(r, 64, 64, 3, 1, 0);
  double best_t = 1e30;
  const int steps = (npix + 63) / 64;
  const int smax = steps / 8 > 0 ? steps / 8 : 1;
  const int brs[2] = {128, 64}, bcs[2] = {128, 64};
  for (int ib = 0; ib < 2; ++ib)
    for (int ic = 0; ic < 2; ++ic) {
      const int BR = brs[ib], BC = bcs[ic];
      if ((fbr && BR != fbr) || (fbc && BC != fbc)) continue;
      if (Kg % BR || OC % BC || (BR == 128 && Kg < 256)) continue;
      const int NS = (BR == 128 && BC == 128) ? 4 : 3;
      const WCand c{BR, BC, NS, wocc(wlds(BR, BC, NS)), (long)(Kg / BR) * (OC / BC),
                    0.55 + 0.15 * (double)(BR * BC) / 4096.0, nullptr};
      wsearch(r, best_t, c, wcost_bf16, false, OC, Kg, steps, smax < 256 ? smax : 256);
    }
}

// bf16 tap-reuse plan: the same model with wgrad3's per-step costs, >= 4 pixel-steps per split.
// Split cap 128 (256 until round 6): fewer partial slabs to write and reduce; ResNet-18 bf16
// -9.5 us twice, ResNet-50 bf16 -24 us, 64 +30 us (profiles/r6_wgrad3_split_cap_ab.jsonl).
void wplan3(WRoute& r, int OC, int IC, int Kg, int npix, int pix) {
  wset(r, 192, 64, 3, 1, 0);
  double best_t = 1e30;
  const int steps = npix / pix;
  const int smax = steps / 4 > 0 ? steps / 4 : 1;
  for (int cfg = 0; cfg < 4; ++cfg) {
    const int BC = cfg & 1 ? 128 : 64, NS = cfg & 2 ? 6 : 3;
    if (OC % BC) continue;
    const WCand c{192, BC, NS, wocc(wlds3(BC, NS)), 3L * (IC / 64) * (OC / BC),
                  (BC == 64 ? 0.9 : 1.3) * (NS == 6 ? 0.8 : 1.0), nullptr};
    wsearch(r, best_t, c, wcost_bf16, false, OC, Kg, steps, smax < 128 ? smax : 128);
  }
}

// fp32 tile plan (wgrad2f_kernel): a stage at the full f32 MFMA rate is BR*BC/4 cycles per wave;
// eff as measured: 64x64 0.55 / 0.65 / 0.72 at k = 1 / 2 / 3 co-resident workgroups.
void wplanf(WRoute& r, int OC, int Kg, int npix) {
  static const double eff_sq[3] = {0.55, 0.65, 0.72}, eff_wide[3] = {0.60, 0.68, 0.68};
  wset(r, 64, 64, 3, 1, 0);
  double best_t = 1e30;
  const int steps = (npix + 31) / 32;
  const int brs[2] = {128, 64}, bcs[2] = {128, 64};
  for (int ib = 0; ib < 2; ++ib)
    for (int ic = 0; ic < 2; ++ic) {
      const int BR = brs[ib], BC = bcs[ic];
      if (Kg % BR || OC % BC) continue;
      const WCand c{BR, BC, 3, wocc(wldsf(BR, BC, 3)), (long)(Kg / BR) * (OC / BC),
                    (double)(BR * BC) / 4.0 / 2100.0, BR == 64 && BC == 64 ? eff_sq : eff_wide};
      wsearch(r, best_t, c, wcost_f32, true, OC, Kg, steps, steps < 256 ? steps : 256);
    }
}

// fp32 tap-reuse plan (wgrad3f_kernel): the fp32 round model with the tap-reuse tile (192 x BC
// per workgroup, 3 x 64 x BC x 32 MACs per stage). eff(k) as measured for the tap-reuse conv
// mainloops (64-66 % at 2-3 co-resident workgroups).
void wplan3f(WRoute& r, int OC, int IC, int Kg, int npix) {
  static const double eff[3] = {0.55, 0.66, 0.70};
  wset(r, 192, 64, 3, 1, 0);
  double best_t = 1e30;
  const int steps = npix / 32;
  for (int BC = 64; BC <= 128; BC *= 2) {
    if (OC % BC) continue;
    const WCand c{192, BC, 3, wocc(wlds3f(BC, 3)), 3L * (IC / 64) * (OC / BC), 3.0 * 64 * BC / 4.0 / 2100.0, eff};
    wsearch(r, best_t, c, wcost_f32, true, OC, Kg, steps, steps < 512 ? steps : 512);
  }
}

// Which kernel the weight gradient of this geometry takes and how it is split; 0, or the code
// psx_conv_wgrad2 refuses the geometry with (-2).
int route_wgrad(const WGeom& g, bool f32, WRoute& r) {
  const int H = g.H, W = g.W, IC = g.IC, OC = g.OC, Kg = g.Kg, npix = g.npix();
  r = WRoute{kTile, f32 ? 1 : 0, 0, 0, 0, 1, 0, 0};
  if (OC % 64 || Kg % 64) return -2;
  if (f32 && IC == 4 && g.R == 7 && g.S == 7 && g.stride == 2 && g.pad == 3 && OC == 64 && H == 224 && W == 224) {
    // the ImageNet stem: its own MFMA kernel with the input patch in LDS (stem.hip), its own split query
    const int e = psx_stem7_wgrad(nullptr, nullptr, nullptr, g.Nb, H, W, 3, 4, OC, Kg, nullptr);
    if (e != -11) {
      r.kind = kStem7;
      r.splits = e;
      return e < 0 ? e : 0;
    }
  }
  // 3x3 stride-1 layers, tap-reuse kernels: power-of-two rows (whole rows in 64-pixel steps, 32 in
  // fp32), or in bf16 widths dividing 56 (ResNet-50: 56-pixel steps of whole rows, G)
  const bool w3ok = g.R == 3 && g.S == 3 && g.stride == 1 && g.pad == 1 && IC % 64 == 0;
  const bool pow2hw = (W & (W - 1)) == 0 && (H & (H - 1)) == 0 && W >= 2;
  if (f32 && w3ok && pow2hw && W <= 32 && npix % 32 == 0 && Kg == 9 * IC) {
    r.kind = kTap;
    r.pix = 32;
    wplan3f(r, OC, IC, Kg, npix);
  } else if (f32) {
    if (IC % 4 || (IC & (IC - 1))) return -2;
    r.pix = 32;
    wplanf(r, OC, Kg, npix);
  } else {
    const bool pow2 = pow2hw && W <= 64 && npix % 64 == 0;
    const bool gen = !pow2 && W >= 2 && 56 % W == 0 && npix % 56 == 0;
    if (w3ok && (pow2 || gen)) {
      r.kind = pow2 ? kTap : kTapG;
      r.pix = pow2 ? 64 : 56;
      wplan3(r, OC, IC, Kg, npix, r.pix);
    } else {
      // Tile: the round-5 sweep (profiles/r5_r50_wgrad_tiles.jsonl, ResNet-50's 1x1 layers): 64 (k) x
      // 128 (oc) wins by 10-20 % on every layer up to 28x28 with OC % 128 == 0 (128x512x28 42.0 ->
      // 34.7 us, 1024x2048x14/s2 64.3 -> 55.4), 64x64 on the 56x56 ones (the model's choice there).
      const bool t128 = OC % 128 == 0 && Kg % 64 == 0 && npix <= 128 * 28 * 28;
      r.pix = 64;
      wplan(r, OC, Kg, npix, t128 ? 64 : 0, t128 ? 128 : 0);
    }
  }
  if ((r.kind == kTile && Kg % r.BR) || OC % r.BC) return -2;
  return 0;
}

int ilog2w(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return l;
}

// One launch table per kernel family: every instantiation, by the route fields that select it.
// (Listed in the order the file has always instantiated them: the compiler numbers its local
// labels by that order, so scripts/prof/isa_equal.py sees any reordering as a change.)
template <typename Args>
struct WKernel {
  int kind, BR, BC, NS;
  void (*fn)(Args);
  int lds;
};
#define PSX_W2F(BR, BC) {kTile, BR, BC, 3, wgrad2f_kernel<BR, BC, 3>, wldsf(BR, BC, 3)}
#define PSX_W3F(BC) {kTap, 192, BC, 3, wgrad3f_kernel<BC, 3>, wlds3f(BC, 3)}
#define PSX_W3(BC, NS, G) {G ? kTapG : kTap, 192, BC, NS, wgrad3_kernel<BC, NS, G>, wlds3(BC, NS)}
#define PSX_W2(BR, BC, NS) {kTile, BR, BC, NS, wgrad2_kernel<BR, BC, NS>, wlds(BR, BC, NS)}
const WKernel<Wgrad2Args> kW2fKernels[4] = {PSX_W2F(128, 128), PSX_W2F(128, 64), PSX_W2F(64, 128), PSX_W2F(64, 64)};
const WKernel<Wgrad3Args> kW3fKernels[2] = {PSX_W3F(128), PSX_W3F(64)};
const WKernel<Wgrad3Args> kW3Kernels[8] = {PSX_W3(128, 6, false), PSX_W3(128, 3, false), PSX_W3(64, 6, false),
                                           PSX_W3(64, 3, false),  PSX_W3(128, 6, true),  PSX_W3(128, 3, true),
                                           PSX_W3(64, 6, true),   PSX_W3(64, 3, true)};
const WKernel<Wgrad2Args> kW2Kernels[4] = {PSX_W2(128, 128, 4), PSX_W2(128, 64, 3), PSX_W2(64, 128, 3),
                                           PSX_W2(64, 64, 3)};
#undef PSX_W2F
#undef PSX_W3F
#undef PSX_W3
#undef PSX_W2

// Launches the route's kernel of an n-entry table over tiles x splits workgroups; returns the HIP error code.
template <typename Args>
int wlaunch(const WKernel<Args>* tab, int n, const WRoute& r, int tiles, const Args& a, hipStream_t st) {
  for (const WKernel<Args>* k = tab; k < tab + n; ++k)
    if (k->kind == r.kind && k->BR == r.BR && k->BC == r.BC && k->NS == r.NS) {
      hipLaunchKernelGGL(k->fn, dim3(tiles * r.splits), dim3(256), (size_t)k->lds, st, a);
      return (int)hipGetLastError();
    }
  return (int)hipErrorInvalidDeviceFunction;  // no such instantiation
}

int launch_tile(const WRoute& r, const WGeom& g, const void* x, const void* dy, float* part, const void* zero,
                hipStream_t st) {
  Wgrad2Args a{};
  a.x = x;
  a.dy = dy;
  a.part = part;
  a.zero = zero;
  a.IH = g.H; a.IW = g.W; a.IC = g.IC; a.OC = g.OC; a.R = g.R; a.S = g.S; a.pad = g.pad; a.stride = g.stride;
  a.Kg = g.Kg;
  a.log2_icc = ilog2w(g.IC / (r.f32 ? 4 : 8));
  a.npix = g.npix();
  a.div_ohw = make_fastdiv(g.OH() * g.OW());
  a.div_ow = make_fastdiv(g.OW());
  a.div_s = make_fastdiv(g.S);
  a.n_k_tiles = g.Kg / r.BR;
  a.n_oc_tiles = g.OC / r.BC;
  a.splits = r.splits;
  a.steps_per_split = r.sps;
  return wlaunch(r.f32 ? kW2fKernels : kW2Kernels, 4, r, a.n_k_tiles * a.n_oc_tiles, a, st);
}

int launch_tap(const WRoute& r, const WGeom& g, const void* x, const void* dy, float* part, const void* zero,
               hipStream_t st) {
  Wgrad3Args b{};
  b.x = x; b.dy = dy; b.part = part; b.zero = zero;
  b.H = g.H; b.W = g.W; b.log2w = ilog2w(g.W); b.IC = g.IC; b.OC = g.OC; b.Kg = g.Kg; b.npix = g.npix();
  b.n_c_tiles = g.IC / 64; b.n_oc_tiles = g.OC / r.BC; b.splits = r.splits; b.steps_per_split = r.sps;
  b.pix = r.pix;
  b.div_w = make_fastdiv(g.W);
  b.div_h = make_fastdiv(g.H);
  return r.f32 ? wlaunch(kW3fKernels, 2, r, 3 * b.n_c_tiles * b.n_oc_tiles, b, st)
               : wlaunch(kW3Kernels, 8, r, 3 * b.n_c_tiles * b.n_oc_tiles, b, st);
}

}  // namespace

extern "C" {

// Batched TN GEMMs part[b * q + j][K][C] = sum over tiles t in range j of D[b][t][:]^T . X[b][t][:]
// with X [nb][T][C], D [nb][T][K] (the Winograd weight gradient, wino.hip): wgrad2f_kernel as a
// 1x1 weight gradient over nb * T pixels whose split s = b * q + j covers T / q pixels of batch b.
// T % (32 q) == 0; BR | C, BC | K (64 or 128); C a power of two.
int psx_bgemm_tn_f32(const float* X, const float* D, float* part, const void* zero, int T, int C, int K, int nb, int q,
                     int BR, int BC, hipStream_t st) {
  if (q < 1 || T % (32 * q) || C % BR || K % BC || (C & (C - 1)) || (BR != 64 && BR != 128) || (BC != 64 && BC != 128))
    return -2;
  const WGeom g{nb * T, 1, 1, C, K, 1, 1, 1, 0, C};
  const WRoute r{kTile, 1, BR, BC, 3, nb * q, T / q / 32, 32};
  return launch_tile(r, g, X, D, part, zero, st);
}

// Which kernel psx_conv_wgrad2 launches for this geometry and how it splits the pixels, without
// launching anything: route_wgrad's decision. out[8]: kind (0 tile, 1 tap reuse, 2 tap reuse over
// general widths, 3 the ImageNet stem), f32, BR, BC, NS, splits, pixel-steps per split, pixels
// per step. Returns 0 or psx_conv_wgrad2's own refusal of the geometry (-2).
int psx_conv_wgrad2_path(int Nb, int H, int W, int IC, int OC, int R, int S, int stride, int pad, int Kg, int f32,
                         int* out) {
  WRoute r;
  if (const int e = route_wgrad(WGeom{Nb, H, W, IC, OC, R, S, stride, pad, Kg}, f32 != 0, r)) return e;
  const int v[8] = {r.kind, r.f32, r.BR, r.BC, r.NS, r.splits, r.sps, r.pix};
  for (int i = 0; i < 8; ++i) out[i] = v[i];
  return 0;
}

// Returns the split count (query with part == nullptr); partials need splits*OC*Kg floats.
// f32: x / dy are fp32 (wgrad2f_kernel) instead of bf16.
int psx_conv_wgrad2(const void* x, const void* dy, float* part, const void* zero, int Nb, int H, int W, int IC, int OC,
                    int R, int S, int stride, int pad, int Kg, int f32, hipStream_t st) {
  const WGeom g{Nb, H, W, IC, OC, R, S, stride, pad, Kg};
  WRoute r;
  if (const int e = route_wgrad(g, f32 != 0, r)) return e;
  if (!part) return r.splits;
  if (r.kind == kStem7) return psx_stem7_wgrad((const float*)x, (const float*)dy, part, Nb, H, W, 3, 4, OC, Kg, st);
  const int e = r.kind == kTile ? launch_tile(r, g, x, dy, part, zero, st) : launch_tap(r, g, x, dy, part, zero, st);
  return e ? -e : r.splits;
}

}  // extern "C"
