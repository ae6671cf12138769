// Argument block of the distillation loss kernel (distill.hip), host <-> device.
#pragma once
#include <stdint.h>

#include "tdg_decode.h"

namespace tdg {

// Word-level knowledge distillation: cross entropy of the student against
//   target = (1 - alpha) * ((1 - s) * onehot(label) + s / V) + alpha * q,
//   q = sum_m w_m * softmax(teacher_m),
// one row per label. The teachers are the mixture's members (tdg_decode.h
// MemberRows). All strides are in bf16 elements.
constexpr int DISTILL_MAX = MEMBERS_MAX;
struct DistillArgs {
  uint16_t* x;                      // student bf16 [M, ldl]; with write_grad overwritten by dlogits
  MemberRows t;                     // teachers, [M, t.ld[m]]: only the first V columns are read
  const void* labels;               // [M] int32, or int64 when lab64; 0 = PAD
  const float* ntok;                // [1] label count the gradient is divided by (clamped to >= 1)
  float* row_loss;                  // [M] the objective
  float* row_label;                 // [M] the label part alone (what tdg_xent writes), or null
  float* row_correct;               // [M] 1 where the student's first argmax is the label
  float workers, smoothing, alpha;
  int lab64, write_grad;
  int M, V, T, ldl;
};

}  // namespace tdg
