"""Teacher-forced scoring: how probable a model, or an ensemble, finds a
target that already exists -- test-set perplexity, rescoring of n-best or
sample lists, filtering of back-translated or distilled data.

Every member runs the training forward once (no K/V cache: all positions are
known) and its logits go to `ops.kernels.decode.score_tokens`
(csrc/kernels/decode.hip) as the projection wrote them: bf16 [B * T,
vocab_pad] on the GPU, no f32 copy, no slice, nothing vocabulary-wide stored.
The kernel keeps one number per position, the log of the weighted mean of the
members' probabilities of the label, and where asked for the largest such
value of the row, which says whether the label is the model's first choice.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Union

import torch

from tensorflow_distributed_on_gke_amd.infer.ensemble import Ensemble, members
from tensorflow_distributed_on_gke_amd.infer.tokenizer import END
from tensorflow_distributed_on_gke_amd.models.layers import RunCtx
from tensorflow_distributed_on_gke_amd.models.transformer import PAD_ID, Transformer
from tensorflow_distributed_on_gke_amd.ops.kernels.decode import score_tokens


class Scores(NamedTuple):
    tok_lp: torch.Tensor            # f32 [B, T], 0 at ignored positions
    sent_lp: torch.Tensor           # f64 [B], the sum of tok_lp
    n_tok: torch.Tensor             # int64 [B], scored positions
    top_lp: Optional[torch.Tensor]  # f32 [B, T] or None
    logits: Optional[List[torch.Tensor]] = None  # per member [B * T, >= vocab] (return_logits)


def mask_after_end(labels: torch.Tensor, end: int) -> torch.Tensor:
    """labels with every position after the first `end` set to PAD."""
    is_end = (labels == end).long()
    after = is_end.cumsum(dim=1) - is_end > 0
    return labels.masked_fill(after, PAD_ID)


@torch.no_grad()
def score_pairs(model: Union[Transformer, Ensemble], src: torch.Tensor, tgt: torch.Tensor,
                want_top: bool = False, return_logits: bool = False, end: int = END) -> Scores:
    """src int64 [B, S], tgt int64 [B, 1 + T] with [START] first -> `Scores`
    on the model's device. Position t scores label tgt[:, 1 + t] given
    tgt[:, :1 + t]; PAD labels and every position after the first `end` are
    ignored (tok_lp 0, not counted). Of an ensemble: the log of the weighted
    mean of the members' probabilities, token by token."""
    models, weights = members(model)
    dev = models[0].device
    src, tgt = src.to(dev), tgt.to(dev)
    B, T = tgt.shape[0], tgt.shape[1] - 1
    V = models[0].cfg.tgt_vocab
    tgt_in = tgt[:, :-1].contiguous()
    labels = mask_after_end(tgt[:, 1:], end).reshape(B * T)
    logits = []
    for m in models:
        rt = RunCtx(training=False, store=None)
        logits.append(m.project(m.features(src, tgt_in, rt)))
    tok_lp, top_lp = score_tokens(logits, V, labels, weights, pad_id=PAD_ID, want_top=want_top)
    tok_lp = tok_lp.view(B, T)
    return Scores(tok_lp, tok_lp.double().sum(dim=1), (labels != PAD_ID).view(B, T).sum(dim=1),
                  top_lp.view(B, T) if want_top else None, logits if return_logits else None)
