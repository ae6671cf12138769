// Steps shared by the row-wise loss kernels (xent.hip, distill.hip): the f32
// merge of two (max, sum-exp) partials and the first-index argmax combine.
// One copy, so that both kernels order their sums and break their ties the
// same way. (The third shared step, the bf16 pack of a gradient element, is
// tdg_common.h's pack_bf.)
#pragma once
#include "tdg_common.h"

namespace tdg {

// (m, s) <- the softmax partial of both: s = sum exp(x - m) over what was seen
__device__ __forceinline__ void merge(float& m, float& s, float m2, float s2) {
  const float mn = fmaxf(m, m2);
  if (mn == -INFINITY) return;
  s = s * __expf(m - mn) + s2 * __expf(m2 - mn);
  m = mn;
}

}  // namespace tdg

// (bv, bi) <- the larger value; of equal values the lower index. A statement
// macro, not a function: an inlined function is optimised on its own first,
// and as one this branch changed the code of the loops around it
// (docs/KERNELS.md, "Refactoring a kernel file").
#define TDG_ARGMAX_TAKE(bv, bi, bv2, bi2) \
  if ((bv2) > (bv) || ((bv2) == (bv) && (bi2) < (bi))) { (bv) = (bv2); (bi) = (bi2); }
