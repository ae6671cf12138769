// Argument block of the R-Drop paired-row loss kernel (rdrop.hip), host <-> device.
#pragma once
#include <stdint.h>

namespace tdg {

// R-Drop (Liang et al. 2021): the batch runs twice through the model under two
// dropout masks, copy 2 after copy 1, so logits row i and row i + M are the two
// next-token distributions of one label. All strides are in bf16 elements.
struct RdropArgs {
  uint16_t* x;          // bf16 [2 M, ldl]; with write_grad overwritten by dlogits
  const void* labels;   // [2 M] int32, or int64 when lab64; 0 = PAD. labels[i + M] == labels[i]
                        // by construction: only the first M are read
  const float* ntok;    // [1] label count of the doubled batch (clamped to >= 1)
  float* row_loss;      // [2 M] the objective: label part + (alpha / 2) KL(own || other)
  float* row_label;     // [2 M] the label part alone (what tdg_xent writes), or null
  float* row_correct;   // [2 M] 1 where the row's first argmax is the label
  float workers, smoothing, alpha;
  int lab64, write_grad;
  int M, V, ldl;        // M: pairs
};

}  // namespace tdg
