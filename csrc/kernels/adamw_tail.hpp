// The per-element arithmetic of the AdamW server update (adamw.hip), shared by every form of the
// kernel so that all of them end in the same bits for the same fp32 gradient sum s:
//   g  = s * gscale
//   m' = beta1 * m + (1 - beta1) * g
//   v' = beta2 * v + (1 - beta2) * g * g
//   p' = p * decay - step_size * m' / (sqrt(v') * rsqrt_bc2 + eps)
// with the eight fp32 scalars the host derives from (lr, beta1, beta2, eps, wd, t) in double
// (psx_adamw_scalars): step_size = lr / (1 - beta1^t), rsqrt_bc2 = 1 / sqrt(1 - beta2^t), decay =
// 1 - lr * wd. torch.optim.AdamW's form; with wd = 0 it is plain Adam.
//
// Every multiply-add that fuses is written as an explicit fma and contraction is off for the rest,
// so the rounding chain does not depend on what the compiler sees around the call: product,
// product, fma (m'); square, product, fma (v'); sqrt, fma, divide (the step); product, fma (p').
// sqrt and the divide are the correctly rounded ones, not the approximate intrinsics.
#pragma once
#include "common.hpp"

namespace psx {

struct AdamwScalars {
  float step_size, beta1, omb1, beta2, omb2, rsqrt_bc2, eps, decay;
};

// The moments and the step, shared with lamb_tail.hpp (the LAMB update forms the same m', v' and
// quotient, so its moments are AdamW's bit for bit). m, v: this element's moments, read and
// replaced. Returns m' / (sqrt(v') * rsqrt_bc2 + eps): sqrt, fma, divide.
PSX_DEV float adamw_moments(float s, float& m, float& v, float gscale, const AdamwScalars& c) {
#pragma clang fp contract(off)
  const float g = s * gscale;
  const float mn = __builtin_fmaf(c.beta1, m, c.omb1 * g);
  const float vn = __builtin_fmaf(c.beta2, v, c.omb2 * (g * g));
  const float den = __builtin_fmaf(__builtin_sqrtf(vn), c.rsqrt_bc2, c.eps);
  m = mn;
  v = vn;
  return mn / den;
}

// m, v: this element's moments, read and replaced. Returns p'.
PSX_DEV float adamw_tail(float s, float pv, float& m, float& v, float gscale, const AdamwScalars& c) {
#pragma clang fp contract(off)
  const float upd = adamw_moments(s, m, v, gscale, c);
  return __builtin_fmaf(-c.step_size, upd, pv * c.decay);
}

}  // namespace psx
