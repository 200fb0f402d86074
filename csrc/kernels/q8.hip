// Block-scaled int8 gradient wire with error feedback (push codec --codec q8, parallel/q8.py).
//
// Payload (one uint8 buffer of fixed size for a given n):
//   [ header: 4 x int32 = {magic 'Q8B1', n, block = 256, nblk = ceil(n / 256)}      16 bytes
//   | scales: fp32[nblk], section padded to a multiple of 16 bytes
//   | q:      int8[n],    section padded to a multiple of 16 bytes ]
// Blocks are runs of 256 consecutive elements of the flat parameter arena and are independent:
// every entry point takes a 256-aligned element sub-range [off, off + cnt).
// The frame (layout, range check, gradient loaders, header write, the source list and the two
// forms of the update from payloads) is blockwire.hpp's; here is the codec's arithmetic.
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
#include "blockwire.hpp"

// Everything below keeps its multiplies and adds apart (hipcc contracts by default); the shared
// update tail above was parsed with the library default, as in optim.hip.
#pragma clang fp contract(off)

namespace psx {

constexpr int kQ8Magic = 0x31423851;  // the bytes 'Q' '8' 'B' '1'

// body: int8 q[n], padded to a multiple of 16 bytes
static inline BlockLayout q8_layout(long n) { return block_layout(n, (n + 15) & ~15L); }

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

// What an encode quantises and what it leaves behind, per element: `ro` is the array it only
// reads, `rw` the fp32 one it reads and writes back.
struct Q8Push {  // the push wire: the block is resid + g, and resid keeps block - deq
  PSX_DEV static float block(float rw, float ro) { return rw + ro; }
  PSX_DEV static float back(float, float blk, float deq) { return blk - deq; }
};
struct Q8Fetch {  // the fetch wire: the block is arena - shadow, and shadow becomes shadow + deq
  PSX_DEV static float block(float rw, float ro) { return ro - rw; }
  PSX_DEV static float back(float rw, float, float deq) { return rw + deq; }
};

// Blocks [blk0, blk1) of the arena. VEC: ro, rw 16-byte (fp16 ro: 8-byte) aligned; the tail
// block (the one holding element n - 1 when n % 256 != 0) and the unaligned form go element by
// element and touch nothing at or past n in ro or rw. q words past n within the padded section
// [0, qwords) are written as zeros.
template <typename P, typename GT, bool VEC>
PSX_DEV void q8_encode_blocks(const GT* __restrict__ ro, float* __restrict__ rw, long n, long blk0, long blk1,
                              float* __restrict__ scales, uint32_t* __restrict__ qw, long qwords,
                              int* __restrict__ hdr) {
  const int lane = threadIdx.x & 63;
  block_write_header(hdr, kQ8Magic, n);
  const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long)gridDim.x * 4;
  for (long b = blk0 + wave; b < blk1; b += nwaves) {
    const long e = b * kBlock + lane * 4;
    const bool full = (b + 1) * kBlock <= n;  // wave-uniform
    float old[4], blk[4];
    if (VEC && full) {
      float rv[4];
      ld_g4(ro, e, rv);
      const f32x4 t = *reinterpret_cast<const f32x4*>(rw + e);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        old[j] = t[j];
        blk[j] = P::block(t[j], rv[j]);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        old[j] = e + j < n ? rw[e + j] : 0.f;
        blk[j] = e + j < n ? P::block(old[j], ld_g1(ro, e + j)) : 0.f;
      }
    }
    uint32_t w;
    float scale, deq[4], out[4];
    q8_quant4(blk, scale, w, deq);
#pragma unroll
    for (int j = 0; j < 4; ++j) out[j] = P::back(old[j], blk[j], deq[j]);
    if (VEC && full) {
      *reinterpret_cast<f32x4*>(rw + e) = (f32x4){out[0], out[1], out[2], out[3]};
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (e + j < n) rw[e + j] = out[j];
    }
    if ((e >> 2) < qwords) qw[e >> 2] = w;
    if (lane == 0) scales[b] = scale;
  }
}

template <typename GT, bool VEC>
__global__ __launch_bounds__(256) void q8_encode_kernel(const GT* __restrict__ g, float* __restrict__ resid, long n,
                                                        long blk0, long blk1, float* __restrict__ scales,
                                                        uint32_t* __restrict__ qw, long qwords,
                                                        int* __restrict__ hdr) {
  q8_encode_blocks<Q8Push, GT, VEC>(g, resid, n, blk0, blk1, scales, qw, qwords, hdr);
}

// The fetch wire's encode (--fetch-codec q8delta, parallel/fetchq8.py): the same pass over
// arena and shadow. 13 bytes per element: 8 read, 4 + 1 written.
template <bool VEC>
__global__ __launch_bounds__(256) void fetchq8_encode_kernel(const float* __restrict__ arena,
                                                             float* __restrict__ shadow, long n, long blk0, long blk1,
                                                             float* __restrict__ scales, uint32_t* __restrict__ qw,
                                                             long qwords, int* __restrict__ hdr) {
  q8_encode_blocks<Q8Fetch, float, VEC>(arena, shadow, n, blk0, blk1, scales, qw, qwords, hdr);
}

// The codec policy of the shared update forms (blockwire.hpp). The rows form takes q as one dword
// per row and source and the row's scale, wave-uniform, and issues two sources' loads ahead of
// their first use. The form with one 16-byte q load per lane (a lane owning 16 consecutive
// elements) makes each of its four p loads touch a quarter of 64 separate 64-byte segments; it
// measured 21.7 us against 16.2 us for this one (W = 1, n = 11.2 M; the fp16-wire kernel: 17.5 us).
struct Q8Wire {
  PSX_DEV static float deq1(const uint8_t* payload, long q_off, long i) {
    const float sc = reinterpret_cast<const float*>(payload + 16)[i / kBlock];
    const float qf = (float)reinterpret_cast<const int8_t*>(payload + q_off)[i];
    return qf * sc;
  }
  PSX_DEV static long unit_base(long e0, long u) { return e0 + (u << 10); }
  static constexpr int kAhead = 2;
  struct Unit {
    uint32_t qv[4];
    float sc[4];
  };
  PSX_DEV static void load(const uint8_t* payload, long q_off, long ub, int lane, Unit& un) {
    const long e = ub + lane * 4;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      un.qv[v] = *reinterpret_cast<const uint32_t*>(payload + q_off + e + 256 * v);
      un.sc[v] = reinterpret_cast<const float*>(payload + 16)[(e >> 8) + v];
    }
  }
  PSX_DEV static void add(const Unit& un, float (&s)[16]) {
#pragma unroll
    for (int j = 0; j < 16; ++j) s[j] = s[j] + q8_f(un.qv[j >> 2], j & 3) * un.sc[j >> 2];
  }
};

// Elements [e0, e1) (e0 a multiple of 256). Element-wise form: any alignment.
template <bool MOM>
__global__ __launch_bounds__(256) void q8_apply_multi_kernel(float* __restrict__ p, BlockSrcs srcs, long q_off,
                                                             float* __restrict__ buf, long e0, long e1, float lr,
                                                             float gscale, float momentum, float wd, int first,
                                                             uint16_t* __restrict__ img) {
  block_apply_elems<MOM, Q8Wire>(p, srcs, q_off, buf, e0 + blockIdx.x * (long)blockDim.x + threadIdx.x,
                                 (long)gridDim.x * blockDim.x, e1, lr, gscale, momentum, wd, first, img, img != nullptr);
}

// Vectorised form (blockwire.hpp block_apply_rows): p, buf, img 16-byte aligned.
template <bool MOM, bool IMG>
__global__ __launch_bounds__(256) void q8_apply_multi_rows_kernel(float* __restrict__ p, BlockSrcs srcs, long q_off,
                                                                  float* __restrict__ buf, long e0, long e1, float lr,
                                                                  float gscale, float momentum, float wd, int first,
                                                                  uint16_t* __restrict__ img) {
  block_apply_rows<MOM, IMG, Q8Wire>(p, srcs, q_off, buf, e0, e1, lr, gscale, momentum, wd, first, img, blockDim.x);
}

// dst[i] = [dst[i] +] scale * (float(q[i]) * scales[i / 256]) over [e0, e1); VEC: dst 16-byte
// aligned, 16 elements per lane, the e1 % 16 tail element by element in workgroup 0.
template <bool ADD>
PSX_DEV void q8_dec1(const float* scales, const int8_t* q, float* dst, long i, float scale) {
  const float v = scale * ((float)q[i] * scales[i / kBlock]);
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

// What the two encodes hand their kernels: the sections of `payload` and the blocks of the range.
struct Q8EncodeArgs {
  float* scales;
  uint32_t* qw;
  long qwords, blk0, blk1;
  int* hdr;  // written by the call that covers block 0
  dim3 grid;
};
static bool q8_encode_args(long n, void* payload, long off, long cnt, Q8EncodeArgs& a) {
  if (!block_range_ok(n, off, cnt) || !al16(payload)) return false;
  const BlockLayout l = q8_layout(n);
  uint8_t* pl = (uint8_t*)payload;
  a.scales = (float*)(pl + l.scales_off);
  a.qw = (uint32_t*)(pl + l.body_off);
  a.qwords = (l.bytes - l.body_off) / 4;
  a.blk0 = off / kBlock;
  a.blk1 = (off + cnt + kBlock - 1) / kBlock;
  a.hdr = off == 0 ? (int*)pl : nullptr;
  a.grid = dim3(stream_grid((a.blk1 - a.blk0) * 64));
  return true;
}

extern "C" {

long psx_q8_payload_bytes(long n) { return q8_layout(n).bytes; }

// Encode elements [off, off + cnt) of acc = resid + g into `payload` (the whole arena's payload,
// 16-byte aligned) and leave resid = acc - deq. g, resid: element 0 of the n-element arrays; g is
// fp32 or fp16 (g_fp16). The header is written by the call that covers block 0.
int psx_q8_encode(const void* g, int g_fp16, float* resid, long n, void* payload, long off, long cnt,
                  hipStream_t st) {
  Q8EncodeArgs a;
  if (!q8_encode_args(n, payload, off, cnt, a)) return (int)hipErrorInvalidValue;
  if (cnt == 0) return 0;
  const bool vec = al16(resid) && (uintptr_t)g % (g_fp16 ? 8 : 16) == 0;
  dispatch2(g_fp16 != 0, vec, [&](auto fp16, auto v) {
    hipLaunchKernelGGL((q8_encode_kernel<wire_t<decltype(fp16)>, decltype(v)::value>), a.grid, dim3(256), 0, st,
                       (const wire_t<decltype(fp16)>*)g, resid, n, a.blk0, a.blk1, a.scales, a.qw, a.qwords, a.hdr);
  });
  return (int)hipGetLastError();
}

// Encode elements [off, off + cnt) of d = arena - shadow into `payload` (the whole arena's payload,
// 16-byte aligned) and leave shadow = shadow + deq. arena, shadow: element 0 of the n-element fp32
// arrays. The header is written by the call that covers block 0.
int psx_fetchq8_encode(const float* arena, float* shadow, long n, void* payload, long off, long cnt,
                       hipStream_t st) {
  Q8EncodeArgs a;
  if (!q8_encode_args(n, payload, off, cnt, a)) return (int)hipErrorInvalidValue;
  if (cnt == 0) return 0;
  if (al16(arena) && al16(shadow))
    hipLaunchKernelGGL(fetchq8_encode_kernel<true>, a.grid, dim3(256), 0, st, arena, shadow, n, a.blk0, a.blk1,
                       a.scales, a.qw, a.qwords, a.hdr);
  else
    hipLaunchKernelGGL(fetchq8_encode_kernel<false>, a.grid, dim3(256), 0, st, arena, shadow, n, a.blk0, a.blk1,
                       a.scales, a.qw, a.qwords, a.hdr);
  return (int)hipGetLastError();
}

// p[off:off+cnt] -= lr * (gscale * sum_k deq_k [+ wd p]) [momentum] straight from nsrc <= 32
// payloads (host array of device pointers, each the whole arena's payload), decoded and summed
// in fp32 in source order; img (optional): bf16 image of the updated parameters. p, buf, img:
// element 0 of the n-element arrays. A payload may share no byte with p, buf or img.
int psx_q8_apply_multi(float* p, const void* const* payloads, int nsrc, float* buf, long n, long off, long cnt,
                       float lr, float gscale, float momentum, float wd, int first, void* img, hipStream_t st) {
  const BlockLayout l = q8_layout(n);
  BlockSrcs sl{};
  if (const int e = block_apply_prologue(payloads, nsrc, l.bytes, n, off, cnt, p, buf, img, sl); e != 0 || sl.n == 0)
    return e;
  const bool mom = buf != nullptr && momentum != 0.f;
  uint16_t* im = (uint16_t*)img;
  const long e0 = off, e1 = off + cnt;
  if (al16(p) && al16(buf) && al16(img) && cnt >= 1024) {
    const dim3 grid(stream_grid((cnt >> 10) * 64));
    dispatch2(mom, im != nullptr, [&](auto m, auto i) {
      hipLaunchKernelGGL((q8_apply_multi_rows_kernel<decltype(m)::value, decltype(i)::value>), grid, dim3(256), 0, st,
                         p, sl, l.body_off, buf, e0, e1, lr, gscale, momentum, wd, first, im);
    });
    return (int)hipGetLastError();
  }
  const dim3 grid(stream_grid(cnt));
  if (mom)
    hipLaunchKernelGGL(q8_apply_multi_kernel<true>, grid, dim3(256), 0, st, p, sl, l.body_off, buf, e0, e1, lr, gscale,
                       momentum, wd, first, im);
  else
    hipLaunchKernelGGL(q8_apply_multi_kernel<false>, grid, dim3(256), 0, st, p, sl, l.body_off, buf, e0, e1, lr,
                       gscale, momentum, wd, first, im);
  return (int)hipGetLastError();
}

// dst[off:off+cnt] = [dst +] scale * deq (dst: element 0 of the n-element fp32 array, sharing no
// byte with the payload).
int psx_q8_decode(const void* payload, float* dst, long n, long off, long cnt, float scale, int add,
                  hipStream_t st) {
  if (!block_range_ok(n, off, cnt) || !al16(payload)) return (int)hipErrorInvalidValue;
  if (cnt == 0) return 0;
  const BlockLayout l = q8_layout(n);
  if (ranges_overlap(payload, (size_t)l.bytes, dst, (size_t)n * 4)) return (int)hipErrorInvalidValue;
  const uint8_t* pl = (const uint8_t*)payload;
  const float* scales = (const float*)(pl + l.scales_off);
  const int8_t* q = (const int8_t*)(pl + l.body_off);
  const long e0 = off, e1 = off + cnt;
  const bool vec = al16(dst) && cnt >= 16;
  const dim3 grid(stream_grid(vec ? cnt / 16 : cnt));
  dispatch2(add != 0, vec, [&](auto a, auto v) {
    hipLaunchKernelGGL((q8_decode_kernel<decltype(a)::value, decltype(v)::value>), grid, dim3(256), 0, st, scales, q,
                       dst, e0, e1, scale);
  });
  return (int)hipGetLastError();
}

}  // extern "C"
