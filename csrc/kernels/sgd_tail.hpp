// The tail of the server update, shared by every apply kernel that has to agree bit for bit:
// sgd_apply (its scalar kernel and its 8-per-lane fp16 kernel, which a slice's alignment chooses
// between) / sgd_apply_multi (optim.hip), q8_apply_multi (q8.hip), and the LARS, guard and
// DC-ASGD applies, which are checked against them. A loopback round sums its
// workers' gradients into a dense fp32 buffer and goes through sgd_apply; a gathered round sums
// them inside sgd_apply_multi / q8_apply_multi. Both end here with the same fp32 sum s:
//   d = s * gscale [+ wd * p];  [v = first ? d : momentum * buf + d;  buf = v;  d = v;]
//   p_new = p - lr * d
// One definition with its roundings spelled out: left to the compiler's contraction, the same
// source fused differently from one instantiation to the next (the momentum kernels and some
// lanes of the 8-per-lane kernels paired s * gscale with wd * p in one packed multiply and added
// the two rounded products, the others fused wd * p into the add), so the bits of an update
// depended on which kernel a slice's alignment selected. In every user now: the product
// s * gscale rounded, wd * p and momentum * buf each fused into their add (one rounding), and
// the step lr * d rounded before it is subtracted (two roundings) — the step of the plain
// single-worker round, p - fl(lr * g), as the 8-per-lane kernel has always taken it.
#pragma once
#include "common.hpp"

namespace psx {

// bufp: this element's momentum slot (read unless `first`, then written); unused without MOM.
template <bool MOM>
PSX_DEV float sgd_tail(float s, float pv, float* bufp, float lr, float gscale, float momentum, float wd,
                       int first) {
#pragma clang fp contract(off)
  float d = s * gscale;
  if (wd != 0.f) d = __builtin_fmaf(wd, pv, d);
  if (MOM) {
    const float v = first ? d : __builtin_fmaf(momentum, *bufp, d);
    *bufp = v;
    d = v;
  }
  const float step = lr * d;
  return pv - step;
}

}  // namespace psx
