// 1-bit sign gradient wire with error feedback (push codec --codec sign1, parallel/sign1.py).
//
// Payload (one uint8 buffer of fixed size for a given n):
//   [ header: 4 x int32 = {magic 'S1B1', n, block = 256, nblk = ceil(n / 256)}      16 bytes
//   | scales: fp32[nblk], section padded to a multiple of 16 bytes
//   | signs:  uint64[4 * nblk]   (32 bytes per block) ]
// Blocks are runs of 256 consecutive elements of the flat parameter arena and are independent:
// every entry point takes a 256-aligned element sub-range [off, off + cnt).
// The frame (layout, range check, gradient loaders, header write, the source list and the two
// forms of the update from payloads) is blockwire.hpp's; here is the codec's arithmetic.
// Word j (0..3) of a block has bit l (0..63) equal to the sign of block element 4 l + j: the lane
// that owns elements 4 l .. 4 l + 3 contributes bit l to each of four ballots, and a word read
// back is the lane mask of its row of elements.
//
// Arithmetic per block, acc = resid + float(g) (fixed: the torch CPU path of parallel/sign1.py
// follows it literally and both agree bit for bit):
//   t_l   = ((|a[4l]| + |a[4l+1]|) + |a[4l+2]|) + |a[4l+3]|   (elements at or past n count as 0)
//   sum   = wave_sum(t)            (xor butterfly, offsets 32, 16, 8, 4, 2, 1)
//   scale = sum / float(cnt)       (cnt = 256, or n % 256 in the tail block)
//   bit   = acc < 0                (-0.0, +0.0 and NaN give 0)
//   deq   = bit ? -scale : scale,  resid = acc - deq
// A block holding a NaN or an Inf sends scale = NaN and all bits 0 (and keeps resid = NaN): the
// server's parameters go NaN as they would with the fp16 wire, so a diverged run stays visible.
// Decode-and-sum over sources: s = 0; s = s + deq_k in source order.
//
//   * sign1_encode      : one streaming pass, a wave owns a block (64 lanes x 4 elements; 16-byte
//                         loads of g and resid, wave_sum and four ballots, no LDS, no barrier)
//   * sign1_apply_multi : the server update straight from the gathered payloads; a wave's 1024
//                         elements take 16 sign words and 4 scales per source, all of them
//                         wave-uniform scalar loads; same update tail as sgd_apply_multi
//                         (sgd_tail.hpp)
//   * sign1_decode      : dst = [dst +] scale * deq (every other rule, in-process accumulation,
//                         reference semantics)
#include "blockwire.hpp"

// Everything below keeps its multiplies and adds apart (hipcc contracts by default); the shared
// update tail above was parsed with the library default, as in optim.hip.
#pragma clang fp contract(off)

namespace psx {

constexpr int kS1Magic = 0x31423153;  // the bytes 'S' '1' 'B' '1'

// body: uint64 signs[4 * nblk] (32 bytes per block)
static inline BlockLayout s1_layout(long n) { return block_layout(n, 32 * block_count(n)); }

// A payload is only read by the kernels that take one, so its scales and sign words are loaded
// through the constant address space: with a wave-uniform address such a load is a scalar load.
typedef const __attribute__((address_space(4))) float* s1_cf32;
typedef const __attribute__((address_space(4))) uint64_t* s1_cu64;
PSX_DEV s1_cf32 s1_scales(const uint8_t* payload) { return (s1_cf32)(uintptr_t)(payload + 16); }
PSX_DEV s1_cu64 s1_words(const uint8_t* payload, long w_off) { return (s1_cu64)(uintptr_t)(payload + w_off); }

// this lane's bit of a sign word that is the same in every lane (bit l belongs to lane l: the
// word is a lane mask, and the select on it takes the scalar pair as its condition)
PSX_DEV bool s1_lane_bit(uint64_t w) { return __builtin_amdgcn_inverse_ballot_w64(w); }
PSX_DEV float s1_deq(bool bit, float sc) { return bit ? -sc : sc; }

// Blocks [blk0, blk1) of the arena. VEC: g, resid 16-byte (fp16 g: 8-byte) aligned; the tail
// block (the one holding element n - 1 when n % 256 != 0) and the unaligned form go element by
// element and touch nothing at or past n in g or resid.
template <typename GT, bool VEC>
__global__ __launch_bounds__(256) void sign1_encode_kernel(const GT* __restrict__ g, float* __restrict__ resid,
                                                           long n, long blk0, long blk1, float* __restrict__ scales,
                                                           uint64_t* __restrict__ words, int* __restrict__ hdr) {
  const int lane = threadIdx.x & 63;
  block_write_header(hdr, kS1Magic, n);
  const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long)gridDim.x * 4;
  for (long b = blk0 + wave; b < blk1; b += nwaves) {
    const long e = b * kBlock + lane * 4;
    const bool full = (b + 1) * kBlock <= n;  // wave-uniform
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
    float a[4];
    bool bad = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      a[j] = fabsf(acc[j]);
      bad = bad || !(a[j] <= FLT_MAX);  // NaN or Inf
    }
    const float sum = wave_sum(((a[0] + a[1]) + a[2]) + a[3]);
    const bool blk_bad = __ballot(bad) != 0ull;
    const float cnt = full ? (float)kBlock : (float)(n - b * kBlock);
    const float scale = blk_bad ? __builtin_nanf("") : sum / cnt;
    unsigned long long w[4];
    float res[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool bit = !blk_bad && acc[j] < 0.f;
      w[j] = __ballot(bit);
      res[j] = acc[j] - s1_deq(bit, scale);
    }
    if (VEC && full) {
      *reinterpret_cast<f32x4*>(resid + e) = (f32x4){res[0], res[1], res[2], res[3]};
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (e + j < n) resid[e + j] = res[j];
    }
    if (lane < 4) words[4 * b + lane] = lane == 0 ? w[0] : lane == 1 ? w[1] : lane == 2 ? w[2] : w[3];
    if (lane == 0) scales[b] = scale;
  }
}

// The codec policy of the shared update forms (blockwire.hpp). Of a source the wave needs its
// unit's 4 scales and 16 sign words, 144 contiguous-by-section bytes at wave-uniform addresses (the
// block index goes through readfirstlane, the pointers are to constant memory): scalar loads,
// which leave the vector memory path to p, buf and img. Word 4 v + j is the lane mask of element j
// of row v: the decode of an element is one select between scale and -scale. What a further
// source costs follows the number of scalar load requests (three per source and unit here: the
// scales, two times eight words), not their bytes and not their latency: units of 512 or 256
// elements (four and eight requests per 1024 elements) measured 63 and 96 us against 51 us at
// W = 32, n = 11.2 M, and issuing two or four sources' loads together before the first use
// changed nothing (profiles/sign1_kernels.txt).
struct S1Wire {
  PSX_DEV static float deq1(const uint8_t* payload, long w_off, long i) {
    const long b = i / kBlock;
    const int r = (int)(i - b * kBlock);
    const uint64_t w = reinterpret_cast<const uint64_t*>(payload + w_off)[4 * b + (r & 3)];
    return s1_deq((w >> (r >> 2)) & 1, reinterpret_cast<const float*>(payload + 16)[b]);
  }
  // the unit's first block is below 2^23 (n < 2^31) and the same in every lane
  PSX_DEV static long unit_base(long e0, long u) {
    return (long)__builtin_amdgcn_readfirstlane((int)((e0 >> 8) + (u << 2))) * kBlock;
  }
  static constexpr int kAhead = 1;
  struct Unit {
    float sc[4];
    uint64_t w[16];
  };
  PSX_DEV static void load(const uint8_t* payload, long w_off, long ub, int, Unit& un) {
    const int b = (int)(ub >> 8);
    const s1_cf32 scp = s1_scales(payload) + b;
    const s1_cu64 wp = s1_words(payload, w_off) + 4 * (long)b;
#pragma unroll
    for (int v = 0; v < 4; ++v) un.sc[v] = scp[v];
#pragma unroll
    for (int j = 0; j < 16; ++j) un.w[j] = wp[j];
  }
  PSX_DEV static void add(const Unit& un, float (&s)[16]) {
#pragma unroll
    for (int j = 0; j < 16; ++j) s[j] = s[j] + s1_deq(s1_lane_bit(un.w[j]), un.sc[j >> 2]);
  }
};

// Elements [e0, e1) (e0 a multiple of 256). Element-wise form: any alignment.
template <bool MOM>
__global__ __launch_bounds__(256) void sign1_apply_multi_kernel(float* __restrict__ p, BlockSrcs srcs, long w_off,
                                                                float* __restrict__ buf, long e0, long e1, float lr,
                                                                float gscale, float momentum, float wd, int first,
                                                                uint16_t* __restrict__ img) {
  block_apply_elems<MOM, S1Wire>(p, srcs, w_off, buf, e0 + blockIdx.x * (long)blockDim.x + threadIdx.x,
                                 (long)gridDim.x * blockDim.x, e1, lr, gscale, momentum, wd, first, img, img != nullptr);
}

// Vectorised form (blockwire.hpp block_apply_rows): p, buf, img 16-byte aligned.
template <bool MOM, bool IMG>
__global__ __launch_bounds__(256) void sign1_apply_multi_rows_kernel(float* __restrict__ p, BlockSrcs srcs, long w_off,
                                                                     float* __restrict__ buf, long e0, long e1,
                                                                     float lr, float gscale, float momentum, float wd,
                                                                     int first, uint16_t* __restrict__ img) {
  block_apply_rows<MOM, IMG, S1Wire>(p, srcs, w_off, buf, e0, e1, lr, gscale, momentum, wd, first, img, blockDim.x);
}

// dst[i] = [dst[i] +] scale * deq[i] over blocks [blk0, blk1), nothing at or past e1. A wave owns
// a block as in the encode; VEC: dst 16-byte aligned, one 16-byte access per lane in whole blocks.
template <bool ADD, bool VEC>
__global__ __launch_bounds__(256) void sign1_decode_kernel(const uint8_t* __restrict__ payload, long w_off,
                                                           float* __restrict__ dst, long blk0, long blk1, long e1,
                                                           float scale) {
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = gridDim.x * 4;
  for (long bb = blk0 + wave; bb < blk1; bb += nwaves) {
    const int b = __builtin_amdgcn_readfirstlane((int)bb);
    const long e = (long)b * kBlock + lane * 4;
    const float sc = s1_scales(payload)[b];
    const s1_cu64 wp = s1_words(payload, w_off) + 4 * (long)b;
    float o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = scale * s1_deq(s1_lane_bit(wp[j]), sc);
    if (VEC && (long)(b + 1) * kBlock <= e1) {
      f32x4 d = {o[0], o[1], o[2], o[3]};
      if (ADD) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(dst + e);
#pragma unroll
        for (int j = 0; j < 4; ++j) d[j] = t[j] + o[j];
      }
      *reinterpret_cast<f32x4*>(dst + e) = d;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (e + j < e1) dst[e + j] = ADD ? dst[e + j] + o[j] : o[j];
    }
  }
}

}  // namespace psx

using namespace psx;

extern "C" {

long psx_sign1_payload_bytes(long n) { return s1_layout(n).bytes; }

// Encode elements [off, off + cnt) of acc = resid + g into `payload` (the whole arena's payload,
// 16-byte aligned) and leave resid = acc - deq. g, resid: element 0 of the n-element arrays; g is
// fp32 or fp16 (g_fp16). The header is written by the call that covers block 0.
int psx_sign1_encode(const void* g, int g_fp16, float* resid, long n, void* payload, long off, long cnt,
                     hipStream_t st) {
  if (!block_range_ok(n, off, cnt) || !al16(payload)) return (int)hipErrorInvalidValue;
  if (cnt == 0) return 0;
  const BlockLayout l = s1_layout(n);
  uint8_t* pl = (uint8_t*)payload;
  float* scales = (float*)(pl + l.scales_off);
  uint64_t* words = (uint64_t*)(pl + l.body_off);
  const long blk0 = off / kBlock, blk1 = (off + cnt + kBlock - 1) / kBlock;
  int* hdr = off == 0 ? (int*)pl : nullptr;
  const bool vec = al16(resid) && (uintptr_t)g % (g_fp16 ? 8 : 16) == 0;
  const dim3 grid(stream_grid((blk1 - blk0) * 64));
  dispatch2(g_fp16 != 0, vec, [&](auto fp16, auto v) {
    hipLaunchKernelGGL((sign1_encode_kernel<wire_t<decltype(fp16)>, decltype(v)::value>), grid, dim3(256), 0, st,
                       (const wire_t<decltype(fp16)>*)g, resid, n, blk0, blk1, scales, words, hdr);
  });
  return (int)hipGetLastError();
}

// p[off:off+cnt] -= lr * (gscale * sum_k deq_k [+ wd p]) [momentum] straight from nsrc <= 32
// payloads (host array of device pointers, each the whole arena's payload), decoded and summed
// in fp32 in source order; img (optional): bf16 image of the updated parameters. p, buf, img:
// element 0 of the n-element arrays. A payload may share no byte with p, buf or img.
int psx_sign1_apply_multi(float* p, const void* const* payloads, int nsrc, float* buf, long n, long off, long cnt,
                          float lr, float gscale, float momentum, float wd, int first, void* img, hipStream_t st) {
  const BlockLayout l = s1_layout(n);
  BlockSrcs sl{};
  if (const int e = block_apply_prologue(payloads, nsrc, l.bytes, n, off, cnt, p, buf, img, sl); e != 0 || sl.n == 0)
    return e;
  const bool mom = buf != nullptr && momentum != 0.f;
  uint16_t* im = (uint16_t*)img;
  const long e0 = off, e1 = off + cnt;
  if (al16(p) && al16(buf) && al16(img) && cnt >= 1024) {
    const dim3 grid(stream_grid((cnt >> 10) * 64));
    dispatch2(mom, im != nullptr, [&](auto m, auto i) {
      hipLaunchKernelGGL((sign1_apply_multi_rows_kernel<decltype(m)::value, decltype(i)::value>), grid, dim3(256), 0,
                         st, p, sl, l.body_off, buf, e0, e1, lr, gscale, momentum, wd, first, im);
    });
    return (int)hipGetLastError();
  }
  const dim3 grid(stream_grid(cnt));
  if (mom)
    hipLaunchKernelGGL(sign1_apply_multi_kernel<true>, grid, dim3(256), 0, st, p, sl, l.body_off, buf, e0, e1, lr,
                       gscale, momentum, wd, first, im);
  else
    hipLaunchKernelGGL(sign1_apply_multi_kernel<false>, grid, dim3(256), 0, st, p, sl, l.body_off, buf, e0, e1, lr,
                       gscale, momentum, wd, first, im);
  return (int)hipGetLastError();
}

// dst[off:off+cnt] = [dst +] scale * deq (dst: element 0 of the n-element fp32 array, sharing no
// byte with the payload).
int psx_sign1_decode(const void* payload, float* dst, long n, long off, long cnt, float scale, int add,
                     hipStream_t st) {
  if (!block_range_ok(n, off, cnt) || !al16(payload)) return (int)hipErrorInvalidValue;
  if (cnt == 0) return 0;
  const BlockLayout l = s1_layout(n);
  if (ranges_overlap(payload, (size_t)l.bytes, dst, (size_t)n * 4)) return (int)hipErrorInvalidValue;
  const long e1 = off + cnt;
  const long blk0 = off / kBlock, blk1 = (e1 + kBlock - 1) / kBlock;
  const dim3 grid(stream_grid((blk1 - blk0) * 64));
  dispatch2(add != 0, al16(dst), [&](auto a, auto v) {
    hipLaunchKernelGGL((sign1_decode_kernel<decltype(a)::value, decltype(v)::value>), grid, dim3(256), 0, st,
                       (const uint8_t*)payload, l.body_off, dst, blk0, blk1, e1, scale);
  });
  return (int)hipGetLastError();
}

}  // extern "C"
