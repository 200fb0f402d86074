// Block-scaled int8 gradient wire with error feedback (push codec --codec q8, parallel/q8.py).
//
// Payload (one uint8 buffer of fixed size for a given n):
//   [ header: 4 x int32 = {magic 'Q8B1', n, block = 256, nblk = ceil(n / 256)}      16 bytes
//   | scales: fp32[nblk], section padded to a multiple of 16 bytes
//   | q:      int8[n],    section padded to a multiple of 16 bytes ]
// Blocks are runs of 256 consecutive elements of the flat parameter arena and are independent:
// every entry point takes a 256-aligned element sub-range [off, off + cnt).
//
// Arithmetic per block, acc = resid + float(g) (fixed: the torch CPU path of parallel/q8.py
// follows it literally and both agree bit for bit):
//   amax  = max |acc|            (tail block zero-filled)
//   scale = amax / 127.0f,  inv = amax > 0 ? 127.0f / amax : 0
//   q     = clamp(rintf(acc * inv), -127, 127)   (a NaN product, 0 * inf, counts as 0)
//   deq   = float(q) * scale,  resid = acc - deq  (a separate subtraction, never an FMA)
// A block holding a NaN or an Inf sends scale = NaN, q = 0 (and keeps resid = NaN): the server's
// parameters go NaN as they would with the fp16 wire, so a diverged run stays visible.
// Decode-and-sum over sources: s = 0; s = s + (float(q_k) * scale_k) in source order, the
// product rounded before the add.
//
//   * q8_encode      : one streaming pass, a wave owns a block (64 lanes x 4 elements; 16-byte
//                      loads of g and resid, wave-level shuffle reduction, no LDS, no barrier)
//   * fetchq8_encode : the same pass for the fetch wire (--fetch-codec q8delta): the block is
//                      d = arena - shadow and the server's shadow of the workers' copy becomes
//                      shadow + deq, what q8_decode(add) leaves on every worker
//   * q8_apply_multi : the server update straight from the gathered payloads, 16 int8 per lane
//                      per source (4 rows of a wave's 1024 elements), same update tail as
//                      sgd_apply_multi (sgd_tail.hpp)
//   * q8_decode      : dst = [dst +] scale * deq (in-process accumulation, reference semantics)
#include <float.h>

#include "wire.hpp"

// Everything below keeps its multiplies and adds apart (hipcc contracts by default); the shared
// update tail above was parsed with the library default, as in optim.hip.
#pragma clang fp contract(off)

namespace psx {

constexpr int kQ8Block = 256;
constexpr int kQ8Magic = 0x31423851;  // the bytes 'Q' '8' 'B' '1'

struct Q8Layout {
  long nblk, scales_off, q_off, bytes;
};
static inline Q8Layout q8_layout(long n) {
  Q8Layout l;
  l.nblk = (n + kQ8Block - 1) / kQ8Block;
  l.scales_off = 16;
  l.q_off = l.scales_off + ((4 * l.nblk + 15) & ~15L);
  l.bytes = l.q_off + ((n + 15) & ~15L);
  return l;
}

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

// int8 number j (0..3) of a packed word, as float
PSX_DEV float q8_f(uint32_t w, int j) { return (float)((int)(w << (24 - 8 * j)) >> 24); }

// A wave quantises one block: lane l holds elements 4 l .. 4 l + 3 of it in v. Gives the block's
// scale (wave-uniform), the lane's four int8 packed into w and their dequantised values
// deq[j] = float(q_j) * scale, by the arithmetic in the header.
PSX_DEV void q8_quant4(const float (&v)[4], float& scale, uint32_t& w, float (&deq)[4]) {
  float amax = 0.f;
  bool bad = false;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float a = fabsf(v[j]);
    bad = bad || !(a <= FLT_MAX);  // NaN or Inf (fmaxf below drops NaNs)
    amax = fmaxf(amax, a);
  }
  amax = wave_max(amax);
  const bool blk_bad = __ballot(bad) != 0ull;
  scale = blk_bad ? __builtin_nanf("") : amax / 127.0f;
  const float inv = (!blk_bad && amax > 0.f) ? 127.0f / amax : 0.f;
  w = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float r = rintf(v[j] * inv);
    r = r == r ? r : 0.f;
    r = fminf(fmaxf(r, -127.f), 127.f);
    deq[j] = r * scale;  // r is float(q) exactly
    w |= ((uint32_t)(int)r & 0xffu) << (8 * j);
  }
}

// Blocks [blk0, blk1) of the arena. VEC: g, resid 16-byte (fp16 g: 8-byte) aligned; the tail
// block (the one holding element n - 1 when n % 256 != 0) and the unaligned form go element by
// element and touch nothing at or past n in g or resid. q words past n within the padded section
// [0, qwords) are written as zeros.
template <typename GT, bool VEC>
__global__ __launch_bounds__(256) void q8_encode_kernel(const GT* __restrict__ g, float* __restrict__ resid, long n,
                                                        long blk0, long blk1, float* __restrict__ scales,
                                                        uint32_t* __restrict__ qw, long qwords,
                                                        int* __restrict__ hdr) {
  const int lane = threadIdx.x & 63;
  if (hdr != nullptr && blockIdx.x == 0 && threadIdx.x < 4) {
    const long nblk = (n + kQ8Block - 1) / kQ8Block;
    hdr[threadIdx.x] = threadIdx.x == 0 ? kQ8Magic : threadIdx.x == 1 ? (int)n : threadIdx.x == 2 ? kQ8Block : (int)nblk;
  }
  const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long)gridDim.x * 4;
  for (long b = blk0 + wave; b < blk1; b += nwaves) {
    const long e = b * kQ8Block + lane * 4;
    const bool full = (b + 1) * kQ8Block <= n;  // wave-uniform
    float acc[4];
    if (VEC && full) {
      float gv[4];
      ld_g4(g, e, gv);
      const f32x4 r = *reinterpret_cast<const f32x4*>(resid + e);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = r[j] + gv[j];
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = e + j < n ? resid[e + j] + ld_g1(g, e + j) : 0.f;
    }
    uint32_t w;
    float scale, deq[4], res[4];
    q8_quant4(acc, scale, w, deq);
#pragma unroll
    for (int j = 0; j < 4; ++j) res[j] = acc[j] - deq[j];
    if (VEC && full) {
      *reinterpret_cast<f32x4*>(resid + e) = (f32x4){res[0], res[1], res[2], res[3]};
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (e + j < n) resid[e + j] = res[j];
    }
    if ((e >> 2) < qwords) qw[e >> 2] = w;
    if (lane == 0) scales[b] = scale;
  }
}

// The fetch wire's encode (--fetch-codec q8delta, parallel/fetchq8.py): the same pass with
// d = arena - shadow in place of resid + g, and shadow = shadow + deq (the copy every worker
// holds) in place of the residual. Same forms, same bounds: nothing at or past n is touched in
// arena or shadow. 13 bytes per element: 8 read, 4 + 1 written.
template <bool VEC>
__global__ __launch_bounds__(256) void fetchq8_encode_kernel(const float* __restrict__ arena,
                                                             float* __restrict__ shadow, long n, long blk0, long blk1,
                                                             float* __restrict__ scales, uint32_t* __restrict__ qw,
                                                             long qwords, int* __restrict__ hdr) {
  const int lane = threadIdx.x & 63;
  if (hdr != nullptr && blockIdx.x == 0 && threadIdx.x < 4) {
    const long nblk = (n + kQ8Block - 1) / kQ8Block;
    hdr[threadIdx.x] = threadIdx.x == 0 ? kQ8Magic : threadIdx.x == 1 ? (int)n : threadIdx.x == 2 ? kQ8Block : (int)nblk;
  }
  const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long)gridDim.x * 4;
  for (long b = blk0 + wave; b < blk1; b += nwaves) {
    const long e = b * kQ8Block + lane * 4;
    const bool full = (b + 1) * kQ8Block <= n;  // wave-uniform
    float sh[4], d[4];
    if (VEC && full) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(arena + e);
      const f32x4 s = *reinterpret_cast<const f32x4*>(shadow + e);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        sh[j] = s[j];
        d[j] = a[j] - s[j];
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        sh[j] = e + j < n ? shadow[e + j] : 0.f;
        d[j] = e + j < n ? arena[e + j] - sh[j] : 0.f;
      }
    }
    uint32_t w;
    float scale, deq[4];
    q8_quant4(d, scale, w, deq);
#pragma unroll
    for (int j = 0; j < 4; ++j) sh[j] = sh[j] + deq[j];
    if (VEC && full) {
      *reinterpret_cast<f32x4*>(shadow + e) = (f32x4){sh[0], sh[1], sh[2], sh[3]};
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (e + j < n) shadow[e + j] = sh[j];
    }
    if ((e >> 2) < qwords) qw[e >> 2] = w;
    if (lane == 0) scales[b] = scale;
  }
}

struct Q8Srcs {
  const uint8_t* p[kMaxSrc];
  int n;
};

// one element's decoded sum over the sources, in source order
PSX_DEV float q8_sum1(const Q8Srcs& srcs, long q_off, long i) {
  float s = 0.f;
  for (int k = 0; k < srcs.n; ++k) {
    const float sc = reinterpret_cast<const float*>(srcs.p[k] + 16)[i / kQ8Block];
    const float qf = (float)reinterpret_cast<const int8_t*>(srcs.p[k] + q_off)[i];
    s = s + qf * sc;
  }
  return s;
}

// Elements [e0, e1) (e0 a multiple of 256). Element-wise form: any alignment.
template <bool MOM>
__global__ __launch_bounds__(256) void q8_apply_multi_kernel(float* __restrict__ p, Q8Srcs srcs, long q_off,
                                                             float* __restrict__ buf, long e0, long e1, float lr,
                                                             float gscale, float momentum, float wd, int first,
                                                             uint16_t* __restrict__ img) {
  for (long i = e0 + blockIdx.x * (long)blockDim.x + threadIdx.x; i < e1; i += (long)gridDim.x * blockDim.x) {
    const float pv = p[i];
    const float nv = sgd_tail<MOM>(q8_sum1(srcs, q_off, i), pv, buf + i, lr, gscale, momentum, wd, first);
    p[i] = nv;
    if (img) img[i] = f2bf(nv);
  }
}

// Vectorised form: a wave covers 1024 elements as 4 rows of 256 (one block each); lane l owns
// elements 4 l .. 4 l + 3 of every row, 16 int8 per lane per source. Every p / buf access is
// 16 bytes per lane and contiguous across the wave, q is one dword per row and source, the
// row's scale is wave-uniform, and a lane's loads are issued ahead of their first use (p and buf
// first, then the sources two at a time). The form with one 16-byte q load per lane (a lane
// owning 16 consecutive elements) makes each of its four p loads touch a quarter of 64 separate
// 64-byte segments; it measured 21.7 us against 16.2 us for this one (W = 1, n = 11.2 M; the
// fp16-wire kernel: 17.5 us). p, buf, img 16-byte aligned; what is left of the range after the
// whole 1024-element units goes element by element in workgroup 0.
template <bool MOM, bool IMG>
__global__ __launch_bounds__(256) void q8_apply_multi_rows_kernel(float* __restrict__ p, Q8Srcs srcs, long q_off,
                                                                  float* __restrict__ buf, long e0, long e1, float lr,
                                                                  float gscale, float momentum, float wd, int first,
                                                                  uint16_t* __restrict__ img) {
  const long nu = (e1 - e0) >> 10;  // whole 1024-element units
  const long t0 = e0 + (nu << 10);
  if (blockIdx.x == 0) {
    for (long i = t0 + threadIdx.x; i < e1; i += blockDim.x) {
      const float pv = p[i];
      const float nv = sgd_tail<MOM>(q8_sum1(srcs, q_off, i), pv, buf + i, lr, gscale, momentum, wd, first);
      p[i] = nv;
      if (IMG) img[i] = f2bf(nv);
    }
  }
  const int lane = threadIdx.x & 63;
  const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long)gridDim.x * 4;
  for (long u = wave; u < nu; u += nwaves) {
    const long e = e0 + (u << 10) + lane * 4;  // row v: e + 256 v
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
    for (int k0 = 0; k0 < srcs.n; k0 += 2) {
      uint32_t qv[2][4];
      float sc[2][4];
#pragma unroll
      for (int m = 0; m < 2; ++m)
        if (k0 + m < srcs.n) {
          const uint8_t* base = srcs.p[k0 + m];
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            qv[m][v] = *reinterpret_cast<const uint32_t*>(base + q_off + e + 256 * v);
            sc[m][v] = reinterpret_cast<const float*>(base + 16)[(e >> 8) + v];
          }
        }
#pragma unroll
      for (int m = 0; m < 2; ++m)
        if (k0 + m < srcs.n) {
#pragma unroll
          for (int j = 0; j < 16; ++j) s[j] = s[j] + q8_f(qv[m][j >> 2], j & 3) * sc[m][j >> 2];
        }
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

// dst[i] = [dst[i] +] scale * (float(q[i]) * scales[i / 256]) over [e0, e1); VEC: dst 16-byte
// aligned, 16 elements per lane, the e1 % 16 tail element by element in workgroup 0.
template <bool ADD>
PSX_DEV void q8_dec1(const float* scales, const int8_t* q, float* dst, long i, float scale) {
  const float v = scale * ((float)q[i] * scales[i / kQ8Block]);
  dst[i] = ADD ? dst[i] + v : v;
}

template <bool ADD, bool VEC>
__global__ __launch_bounds__(256) void q8_decode_kernel(const float* __restrict__ scales, const int8_t* __restrict__ q,
                                                        float* __restrict__ dst, long e0, long e1, float scale) {
  if (!VEC) {
    for (long i = e0 + blockIdx.x * (long)blockDim.x + threadIdx.x; i < e1; i += (long)gridDim.x * blockDim.x)
      q8_dec1<ADD>(scales, q, dst, i, scale);
    return;
  }
  const long c0 = e0 >> 4, c1 = e1 >> 4;
  if (blockIdx.x == 0 && (long)threadIdx.x < (e1 & 15)) q8_dec1<ADD>(scales, q, dst, (c1 << 4) + threadIdx.x, scale);
  for (long c = c0 + blockIdx.x * (long)blockDim.x + threadIdx.x; c < c1; c += (long)gridDim.x * blockDim.x) {
    const u32x4 qv = reinterpret_cast<const u32x4*>(q)[c];
    const float sc = scales[c >> 4];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = scale * (q8_f(qv[v], j) * sc);
      if (ADD) {
        const f32x4 d = reinterpret_cast<const f32x4*>(dst)[4 * c + v];
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = d[j] + o[j];
      }
      reinterpret_cast<f32x4*>(dst)[4 * c + v] = o;
    }
  }
}

}  // namespace psx

using namespace psx;

// [off, off + cnt) must start on a block and end on a block or at n
static bool q8_range_ok(long n, long off, long cnt) {
  return n > 0 && n <= 0x7fffffffL && off >= 0 && cnt >= 0 && off % kQ8Block == 0 && off + cnt <= n &&
         ((off + cnt) % kQ8Block == 0 || off + cnt == n);
}

extern "C" {

long psx_q8_payload_bytes(long n) { return q8_layout(n).bytes; }

// Encode elements [off, off + cnt) of acc = resid + g into `payload` (the whole arena's payload,
// 16-byte aligned) and leave resid = acc - deq. g, resid: element 0 of the n-element arrays; g is
// fp32 or fp16 (g_fp16). The header is written by the call that covers block 0.
int psx_q8_encode(const void* g, int g_fp16, float* resid, long n, void* payload, long off, long cnt,
                  hipStream_t st) {
  if (!q8_range_ok(n, off, cnt) || (uintptr_t)payload % 16 != 0) return (int)hipErrorInvalidValue;
  if (cnt == 0) return 0;
  const Q8Layout l = q8_layout(n);
  uint8_t* pl = (uint8_t*)payload;
  float* scales = (float*)(pl + l.scales_off);
  uint32_t* qw = (uint32_t*)(pl + l.q_off);
  const long qwords = (l.bytes - l.q_off) / 4;
  const long blk0 = off / kQ8Block, blk1 = (off + cnt + kQ8Block - 1) / kQ8Block;
  int* hdr = off == 0 ? (int*)pl : nullptr;
  const bool vec = (uintptr_t)resid % 16 == 0 && (uintptr_t)g % (g_fp16 ? 8 : 16) == 0;
  const dim3 grid(stream_grid((blk1 - blk0) * 64));
#define PSX_Q8E(G, V)                                                                                            \
  hipLaunchKernelGGL((q8_encode_kernel<G, V>), grid, dim3(256), 0, st, (const G*)g, resid, n, blk0, blk1, scales, \
                     qw, qwords, hdr)
  if (g_fp16 && vec) PSX_Q8E(uint16_t, true);
  else if (g_fp16) PSX_Q8E(uint16_t, false);
  else if (vec) PSX_Q8E(float, true);
  else PSX_Q8E(float, false);
#undef PSX_Q8E
  return (int)hipGetLastError();
}

// Encode elements [off, off + cnt) of d = arena - shadow into `payload` (the whole arena's payload,
// 16-byte aligned) and leave shadow = shadow + deq. arena, shadow: element 0 of the n-element fp32
// arrays. The header is written by the call that covers block 0.
int psx_fetchq8_encode(const float* arena, float* shadow, long n, void* payload, long off, long cnt,
                       hipStream_t st) {
  if (!q8_range_ok(n, off, cnt) || (uintptr_t)payload % 16 != 0) return (int)hipErrorInvalidValue;
  if (cnt == 0) return 0;
  const Q8Layout l = q8_layout(n);
  uint8_t* pl = (uint8_t*)payload;
  float* scales = (float*)(pl + l.scales_off);
  uint32_t* qw = (uint32_t*)(pl + l.q_off);
  const long qwords = (l.bytes - l.q_off) / 4;
  const long blk0 = off / kQ8Block, blk1 = (off + cnt + kQ8Block - 1) / kQ8Block;
  int* hdr = off == 0 ? (int*)pl : nullptr;
  const dim3 grid(stream_grid((blk1 - blk0) * 64));
  if ((uintptr_t)arena % 16 == 0 && (uintptr_t)shadow % 16 == 0)
    hipLaunchKernelGGL(fetchq8_encode_kernel<true>, grid, dim3(256), 0, st, arena, shadow, n, blk0, blk1, scales, qw,
                       qwords, hdr);
  else
    hipLaunchKernelGGL(fetchq8_encode_kernel<false>, grid, dim3(256), 0, st, arena, shadow, n, blk0, blk1, scales, qw,
                       qwords, hdr);
  return (int)hipGetLastError();
}

// p[off:off+cnt] -= lr * (gscale * sum_k deq_k [+ wd p]) [momentum] straight from nsrc <= 32
// payloads (host array of device pointers, each the whole arena's payload), decoded and summed
// in fp32 in source order; img (optional): bf16 image of the updated parameters. p, buf, img:
// element 0 of the n-element arrays.
int psx_q8_apply_multi(float* p, const void* const* payloads, int nsrc, float* buf, long n, long off, long cnt,
                       float lr, float gscale, float momentum, float wd, int first, void* img, hipStream_t st) {
  if (nsrc < 1 || nsrc > kMaxSrc || !q8_range_ok(n, off, cnt)) return (int)hipErrorInvalidValue;
  if (cnt == 0) return 0;
  const Q8Layout l = q8_layout(n);
  Q8Srcs sl{};
  sl.n = nsrc;
  bool aligned = (uintptr_t)p % 16 == 0 && (uintptr_t)buf % 16 == 0 && (uintptr_t)img % 16 == 0;
  for (int k = 0; k < nsrc; ++k) {
    sl.p[k] = (const uint8_t*)payloads[k];
    if ((uintptr_t)payloads[k] % 16 != 0) return (int)hipErrorInvalidValue;
  }
  const bool mom = buf != nullptr && momentum != 0.f;
  uint16_t* im = (uint16_t*)img;
  const long e0 = off, e1 = off + cnt;
  if (aligned && cnt >= 1024) {
    const dim3 grid(stream_grid((cnt >> 10) * 64));
#define PSX_Q8A(M, I)                                                                                            \
  hipLaunchKernelGGL((q8_apply_multi_rows_kernel<M, I>), grid, dim3(256), 0, st, p, sl, l.q_off, buf, e0, e1, lr, \
                     gscale, momentum, wd, first, im)
    if (mom && im) PSX_Q8A(true, true);
    else if (mom) PSX_Q8A(true, false);
    else if (im) PSX_Q8A(false, true);
    else PSX_Q8A(false, false);
#undef PSX_Q8A
    return (int)hipGetLastError();
  }
  const dim3 grid(stream_grid(cnt));
  if (mom)
    hipLaunchKernelGGL(q8_apply_multi_kernel<true>, grid, dim3(256), 0, st, p, sl, l.q_off, buf, e0, e1, lr, gscale,
                       momentum, wd, first, im);
  else
    hipLaunchKernelGGL(q8_apply_multi_kernel<false>, grid, dim3(256), 0, st, p, sl, l.q_off, buf, e0, e1, lr, gscale,
                       momentum, wd, first, im);
  return (int)hipGetLastError();
}

// dst[off:off+cnt] = [dst +] scale * deq (dst: element 0 of the n-element fp32 array).
int psx_q8_decode(const void* payload, float* dst, long n, long off, long cnt, float scale, int add,
                  hipStream_t st) {
  if (!q8_range_ok(n, off, cnt) || (uintptr_t)payload % 16 != 0) return (int)hipErrorInvalidValue;
  if (cnt == 0) return 0;
  const Q8Layout l = q8_layout(n);
  const uint8_t* pl = (const uint8_t*)payload;
  const float* scales = (const float*)(pl + l.scales_off);
  const int8_t* q = (const int8_t*)(pl + l.q_off);
  const long e0 = off, e1 = off + cnt;
  const bool vec = (uintptr_t)dst % 16 == 0 && cnt >= 16;
  const dim3 grid(stream_grid(vec ? cnt / 16 : cnt));
#define PSX_Q8D(A, V) \
  hipLaunchKernelGGL((q8_decode_kernel<A, V>), grid, dim3(256), 0, st, scales, q, dst, e0, e1, scale)
  if (add && vec) PSX_Q8D(true, true);
  else if (add) PSX_Q8D(true, false);
  else if (vec) PSX_Q8D(false, true);
  else PSX_Q8D(false, false);
#undef PSX_Q8D
  return (int)hipGetLastError();
}

}  // extern "C"
