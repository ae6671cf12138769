"""Word-level knowledge distillation (Kim & Rush 2016): a student trained on
the next-token distributions of frozen teachers.

`Teacher(models, weights)` holds 1 to 8 built `Transformer`s with the
student's vocabularies; their weighted arithmetic mean of probabilities -- the
distribution `infer.ensemble.Ensemble` decodes with -- is the soft part of
the student's target:

    target = (1 - alpha) * ((1 - s) * onehot(label) + s / V) + alpha * q

`Transformer.loss_and_backward(..., teacher=, alpha=)` runs the teachers'
forward (no gradient, no dropout) before the student's and hands their logits
to `ops.kernels.xent_distill` (csrc/kernels/distill.hip), one launch for loss
and gradient. Every member keeps its own parameter store: the student's flat
buffers, data-parallel spans, Adam and EMA never see a teacher, and a member
may be of another preset than the student (a `big` teacher for a `base`
student). Teacher weights never change, so a captured step holds their
forward and a training-state snapshot does not hold them.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch

from tensorflow_distributed_on_gke_amd.models.layers import RunCtx
from tensorflow_distributed_on_gke_amd.models.transformer import Transformer, seq_lengths
from tensorflow_distributed_on_gke_amd.ops.kernels import DISTILL_MAX, distill_weights


class Teacher:
    def __init__(self, models: Sequence[Transformer], weights: Optional[Sequence[float]] = None):
        """1 to 8 built models on one device with equal vocabularies;
        `weights` one positive number per member (default: uniform), kept
        normalised to sum 1."""
        models = list(models)
        if not 1 <= len(models) <= DISTILL_MAX:
            raise ValueError(f"a teacher has 1 to {DISTILL_MAX} members, got {len(models)}")
        first = models[0]
        for m in models[1:]:
            if m.device != first.device:
                raise ValueError(f"teacher members on different devices: {first.device}, {m.device}")
            if (m.cfg.src_vocab, m.cfg.tgt_vocab) != (first.cfg.src_vocab, first.cfg.tgt_vocab):
                raise ValueError("teacher members need equal src_vocab / tgt_vocab, got "
                                 f"{(first.cfg.src_vocab, first.cfg.tgt_vocab)} and "
                                 f"{(m.cfg.src_vocab, m.cfg.tgt_vocab)}")
        if weights is not None and len(weights) != len(models):
            raise ValueError(f"{len(weights)} weights for {len(models)} teacher members")
        try:
            self.weights: List[float] = distill_weights(len(models), weights)
        except RuntimeError as e:
            raise ValueError(str(e)) from None
        self.models: List[Transformer] = models
        # inference contexts: no dropout, no RNG counter, no gradient store
        self._rt = [RunCtx(training=False, store=None) for _ in models]

    @property
    def device(self) -> torch.device:
        return self.models[0].device

    @property
    def cfg(self):
        return self.models[0].cfg

    def check_student(self, student: Transformer) -> None:
        c, t = student.cfg, self.cfg
        if (c.src_vocab, c.tgt_vocab) != (t.src_vocab, t.tgt_vocab):
            raise ValueError(f"the teacher's vocabularies {(t.src_vocab, t.tgt_vocab)} are not the "
                             f"student's {(c.src_vocab, c.tgt_vocab)}")
        if student.device != self.device:
            raise ValueError(f"teacher on {self.device}, student on {student.device}")

    @torch.no_grad()
    def logits(self, src: torch.Tensor, tgt_in: torch.Tensor, lengths=None) -> List[torch.Tensor]:
        """Every member's teacher-forced logits for the batch: GPU bf16
        [B * T, vocab_pad] (each member's own padded row), CPU f32 [B * T, V].
        `lengths`: the (source, decoder input) key lengths, when known."""
        if lengths is None:
            lengths = (seq_lengths(src), seq_lengths(tgt_in))
        return [m.project(m.features(src, tgt_in, rt, lengths)) for m, rt in zip(self.models, self._rt)]


def load_teacher(prefixes: Sequence[str], build, weights: Optional[Sequence[float]] = None) -> Teacher:
    """A Teacher of one model per weights prefix (or snapshot directory);
    `build()` returns a fresh built model of the teachers' configuration."""
    from tensorflow_distributed_on_gke_amd.checkpoint import bundle

    models = []
    for p in prefixes:
        m = build()
        bundle.load_weights(m.store, p)
        models.append(m)
    return Teacher(models, weights)
