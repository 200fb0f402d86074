// The per-element arithmetic of the LAMB server update (lamb.hip), shared by every form of its
// kernels so that all of them end in the same bits for the same fp32 gradient sum s:
//   g  = s * gscale
//   m' = beta1 * m + (1 - beta1) * g
//   v' = beta2 * v + (1 - beta2) * g * g
//   r  = bc1 * (m' / (sqrt(v') * rsqrt_bc2 + eps))
//   u  = r + wd * w        (tensors with ndim > 1)         u = r   (1-D tensors)
//   p' = p - (lr * phi) * u
// m', v' and the quotient are adamw_tail.hpp's own expressions (adamw_moments), so the moments are
// AdamW's bit for bit. The scalars are AdamW's too: the host calls the psx_adamw_scalars
// computation with lr = 1 and wd = 0, which makes its step_size the bias correction
// bc1 = 1 / (1 - beta1^t) (computed in double, rounded once) and its decay exactly 1 (unused).
//
// Rounding chain, every multiply-add that fuses written as an explicit fma and contraction off
// for the rest: product, product, fma (m'); square, product, fma (v'); sqrt, fma, divide (the
// quotient); product with bc1 (r); fma with wd * w (u, adapted tensors only); product lr * phi
// (once per workgroup), fma (p'). sqrt and the divide are the correctly rounded ones.
#pragma once
#include "adamw_tail.hpp"

namespace psx {

// launch 1. m, v: this element's moments, read and replaced; w: the parameter; adapt: the tensor
// takes weight decay (ndim > 1). Returns u.
PSX_DEV float lamb_update(float s, float w, float& m, float& v, float gscale, float wd, bool adapt,
                          const AdamwScalars& c) {
#pragma clang fp contract(off)
  const float r = c.step_size * adamw_moments(s, m, v, gscale, c);
  return adapt ? __builtin_fmaf(wd, w, r) : r;
}

// launch 2. step = lr * phi (one fp32 product per workgroup). Returns p'.
PSX_DEV float lamb_step(float pv, float u, float step) { return __builtin_fmaf(-step, u, pv); }

}  // namespace psx
