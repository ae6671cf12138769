"""Ensemble decoding: several models of one task vote on every next token.

`Ensemble(models, weights)` is accepted wherever the decoding loops and the
`Tester` take a `Transformer`. All members run on the same hypotheses (one
`infer.step.DecoderStep` each), and each step's next-token distribution is the
weighted arithmetic mean of the members' probabilities: their logits pass
through `ops.kernels.ensemble_logprobs` (csrc/kernels/decode.hip) and the
selection kernel of the loop (beam_topk or sample_token) runs on the result
unchanged. On the GPU that result is bf16: an ensemble's scores are those of
the rounded mixture, renormalised by the selection kernel. An ensemble of one
member skips the combine step and is bitwise that member.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple, Union

import torch

from tensorflow_distributed_on_gke_amd.models.transformer import Transformer
from tensorflow_distributed_on_gke_amd.ops.kernels import ENSEMBLE_MAX
from tensorflow_distributed_on_gke_amd.ops.mixture import normalised_weights


class Ensemble:
    def __init__(self, models: Sequence[Transformer], weights: Optional[Sequence[float]] = None):
        """1 to 8 built models on one device with equal vocabularies; `weights`
        one positive number per member (default: uniform), kept normalised
        to sum 1."""
        models = list(models)
        if not 1 <= len(models) <= ENSEMBLE_MAX:
            raise ValueError(f"an ensemble has 1 to {ENSEMBLE_MAX} members, got {len(models)}")
        first = models[0]
        for m in models[1:]:
            if m.device != first.device:
                raise ValueError(f"ensemble members on different devices: {first.device}, {m.device}")
            if (m.cfg.src_vocab, m.cfg.tgt_vocab) != (first.cfg.src_vocab, first.cfg.tgt_vocab):
                raise ValueError("ensemble members need equal src_vocab / tgt_vocab, got "
                                 f"{(first.cfg.src_vocab, first.cfg.tgt_vocab)} and "
                                 f"{(m.cfg.src_vocab, m.cfg.tgt_vocab)}")
        if weights is not None:
            weights = list(weights)
            if len(weights) != len(models):
                raise ValueError(f"{len(weights)} weights for {len(models)} ensemble members")
        self.models: List[Transformer] = models
        self.weights: List[float] = normalised_weights(
            len(models), weights, "ensemble weights must be finite and > 0", ValueError)

    def __len__(self) -> int:
        return len(self.models)

    @property
    def device(self) -> torch.device:
        return self.models[0].device

    @property
    def cfg(self):
        return self.models[0].cfg

    @torch.no_grad()
    def log_probs(self, src: torch.Tensor, tgt_in: torch.Tensor) -> torch.Tensor:
        """Teacher-forced f32 [B, T, V]: the log of the weighted mean of the
        members' next-token probabilities."""
        parts = [torch.log_softmax(m.logits(src, tgt_in), dim=-1) + math.log(w)
                 for m, w in zip(self.models, self.weights)]
        return parts[0] if len(parts) == 1 else torch.logsumexp(torch.stack(parts), dim=0)


def members(model: Union[Transformer, Ensemble]) -> Tuple[List[Transformer], Optional[List[float]]]:
    """(models, weights) of a decoding loop's `model` argument; weights None
    for a single `Transformer`."""
    if isinstance(model, Ensemble):
        return model.models, model.weights
    return [model], None
