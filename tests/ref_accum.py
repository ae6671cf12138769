"""CPU reference of the update-wide label count (xent.hip
count_labels_multi_kernel, ops.kernels.count_labels_multi): for target batches
[B, T1] of token ids, the labels are tgt[:, 1:] and a label counts when it is
not PAD (0). Integer arithmetic; the total as the f32 the kernel stores."""
from typing import Sequence, Tuple

import torch

MAX_ENTRIES = 32


def count_labels_ref(tgts: Sequence[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """(total f32 [1], per-entry int32 [len(tgts)])."""
    counts = torch.stack([(t.cpu()[:, 1:] != 0).sum() for t in tgts]).to(torch.int64)
    return counts.sum().to(torch.float32).reshape(1), counts.to(torch.int32)
