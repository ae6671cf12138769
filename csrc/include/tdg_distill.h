// Argument block of the distillation loss kernel (distill.hip), host <-> device.
#pragma once
#include <stdint.h>

namespace tdg {

// Word-level knowledge distillation: cross entropy of the student against
//   target = (1 - alpha) * ((1 - s) * onehot(label) + s / V) + alpha * q,
//   q = sum_m w_m * softmax(teacher_m),
// one row per label. The teachers ride in the block by value: no pointer
// table on the device. All strides are in bf16 elements.
constexpr int DISTILL_MAX = 8;
struct DistillArgs {
  uint16_t* x;                      // student bf16 [M, ldl]; with write_grad overwritten by dlogits
  const uint16_t* t[DISTILL_MAX];   // teacher m: bf16 [M, ldt[m]], only the first V columns are read
  float logw[DISTILL_MAX];          // log of the weights (> 0, sum 1)
  int ldt[DISTILL_MAX];
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
