// The tail of the server update, shared by every apply kernel that has to agree bit for bit:
// sgd_apply / sgd_apply_multi (optim.hip) and q8_apply_multi (q8.hip). A loopback round sums its
// workers' gradients into a dense fp32 buffer and goes through sgd_apply; a gathered round sums
// them inside sgd_apply_multi / q8_apply_multi. Both end here with the same fp32 sum s:
//   d = s * gscale [+ wd * p];  [v = first ? d : momentum * buf + d;  buf = v;  d = v;]
//   p_new = p - lr * d
// One definition, compiled with the library's default floating-point contraction in every
// translation unit that uses it (q8.hip switches contraction off only after this header), so the
// same multiplies and adds fuse everywhere.
#pragma once
#include "common.hpp"

namespace psx {

// bufp: this element's momentum slot (read unless `first`, then written); unused without MOM.
template <bool MOM>
PSX_DEV float sgd_tail(float s, float pv, float* bufp, float lr, float gscale, float momentum, float wd,
                       int first) {
  float d = s * gscale;
  if (wd != 0.f) d += wd * pv;
  if (MOM) {
    const float v = first ? d : momentum * *bufp + d;
    *bufp = v;
    d = v;
  }
  return pv - lr * d;
}

}  // namespace psx
