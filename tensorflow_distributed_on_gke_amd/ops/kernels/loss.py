"""Loss family (csrc/kernels/xent.hip, distill.hip): cross entropy, its
step statistics, and the word-level distillation loss with its CPU arm."""
from __future__ import annotations

import math
from typing import List

import torch

from tensorflow_distributed_on_gke_amd.ops._ext import C
from tensorflow_distributed_on_gke_amd.ops.mixture import normalised_weights


def xent(logits, V, labels, ntok, workers, smoothing, row_loss, row_correct, write_grad=True):
    C().xent(logits, V, labels, ntok, workers, smoothing, row_loss, row_correct, write_grad)


def xent_stats(row_loss, row_correct, ntok, workers, step_out=None, accum=None):
    C().xent_stats(row_loss, row_correct, ntok, workers, step_out, accum)


DISTILL_MAX = 8


def distill_weights(n: int, weights=None) -> List[float]:
    """n positive teacher weights (default uniform), normalised to sum 1."""
    return normalised_weights(n, weights, f"xent_distill: needs {n} finite weights > 0")


def distill_target(teachers, V: int, labels, smoothing: float, alpha: float, w) -> torch.Tensor:
    """f32 [M, V]: (1 - alpha) ((1 - s) onehot(label) + s / V) + alpha sum_m
    w_m softmax(teacher_m[:, :V]), w already normalised."""
    lab = labels.reshape(-1).to(torch.int64)
    hard = torch.nn.functional.one_hot(lab, V).to(torch.float32) * (1.0 - smoothing) + smoothing / V
    q = sum(wm * torch.softmax(t[:, :V].float(), dim=-1) for t, wm in zip(teachers, w))
    return (1.0 - alpha) * hard + alpha * q


def xent_distill(logits, teachers, V, labels, ntok, workers, smoothing, alpha, weights, row_loss,
                 row_correct, row_label=None, write_grad=True):
    """Word-level distillation loss, forward and backward in one launch
    (csrc/kernels/distill.hip): the cross entropy of softmax(logits[:, :V])
    against target = (1 - alpha) ((1 - s) onehot(label) + s / V) + alpha q,
    q = sum_m w_m softmax(teachers[m][:, :V]); `weights` one positive number per
    teacher (None: uniform), normalised here to sum 1.

    Writes row_loss (the objective), row_correct (first argmax == label),
    row_label when given (the label part alone: what `xent` writes as
    row_loss) and, with write_grad, dlogits = (softmax - target) / (max(ntok,
    1) workers) in place over `logits`, columns [V, ldl) zeroed. PAD rows
    (label 0) give zeros throughout. Teachers are only read, and only their
    first V columns. GPU: bf16 student [M, ldl] and 1 to 8 bf16 teachers, each
    with its own row stride. CPU: the same formulas in f32."""
    T = len(teachers)
    if not 1 <= T <= DISTILL_MAX:
        raise RuntimeError(f"xent_distill: {T} teachers outside [1, {DISTILL_MAX}]")
    if not 1 <= V <= 65536:
        raise RuntimeError(f"xent_distill: V {V} outside [1, 65536]")
    if not 0.0 <= alpha <= 1.0:
        raise RuntimeError(f"xent_distill: alpha {alpha} outside [0, 1]")
    w = distill_weights(T, weights)
    if logits.is_cuda:
        C().xent_distill(logits, list(teachers), V, labels, ntok, workers, smoothing, alpha,
                         [math.log(x) for x in w], row_loss, row_correct, row_label, write_grad)
        return
    x = logits[:, :V].float()
    lab = labels.reshape(-1).to(torch.int64)
    valid = (lab != 0).to(torch.float32)
    logp = torch.log_softmax(x, dim=-1)
    hard = -((1.0 - smoothing) * logp.gather(1, lab.view(-1, 1)).squeeze(1) + smoothing * logp.mean(-1))
    target = distill_target(teachers, V, lab, smoothing, alpha, w)
    row_loss.copy_(-(target * logp).sum(-1) * valid)
    row_correct.copy_((x.argmax(-1) == lab).to(torch.float32) * valid)
    if row_label is not None:
        row_label.copy_(hard * valid)
    if write_grad:
        n = torch.as_tensor(ntok, dtype=torch.float32).reshape(-1)[0].clamp_min(1.0)
        d = (torch.exp(logp) - target) * (valid / (n * workers)).view(-1, 1)
        logits.zero_()
        logits[:, :V] = d.to(logits.dtype)
