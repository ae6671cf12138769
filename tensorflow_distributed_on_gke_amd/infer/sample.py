"""Sampled decoding (temperature, top-k, top-p) on the single-query KV-cache
attention kernel.

Each of the B sentences draws `n` translations, so the decoder runs on
R = B * n rows (r = sentence * n + sample), one new token per row and step.
The loop is beam search's (infer/beam.py) without the ancestry table: a
sample never changes rows, so the decoder step (infer/step.py) runs the
self-attention on identity rows with the K / V append fused into the launch,
and the cross-attention reads the encoder K / V of sentence r // n through a
row map. The selection step is
`ops.kernels.sample_token` (csrc/kernels/decode.hip): row r draws from the
Philox stream of (seed, step t, row_id0 + r), so a row's translation depends
on its identity, not on what else is in the batch.
"""
from __future__ import annotations

from typing import Union

import torch

from tensorflow_distributed_on_gke_amd.infer.ensemble import Ensemble, members
from tensorflow_distributed_on_gke_amd.infer.step import DecoderStep
from tensorflow_distributed_on_gke_amd.models.transformer import PAD_ID, Transformer, seq_lengths
from tensorflow_distributed_on_gke_amd.ops import kernels as K


@torch.no_grad()
def sample_search(model: Union[Transformer, Ensemble], src: torch.Tensor, start: int, end: int,
                  n: int = 1, max_length: int = 20, temperature: float = 1.0, top_k: int = 0,
                  top_p: float = 1.0, seed: int = 0, row_id0: int = 0, return_steps: bool = False):
    """src int64 [B, S] -> (tokens int64 [B, n, 1 + len], scores f32 [B, n]).

    Scores are sums of the model's own f32 log-probabilities (T = 1,
    unfiltered: comparable with beam search's); an ended row keeps its score
    and is padded with PAD. Row r's identity in the random stream is
    row_id0 + r, or, with one `row_id0` per sentence, row_id0[r // n] + r % n.
    With `return_steps` a third value lists, per step,
    the (logits [R, >= V], token int32 [R], fin int32 [R]) the step saw and
    gave.

    `model` may be an `Ensemble` (infer/ensemble.py): its members run on the
    same rows, one `DecoderStep` each, and the draw is from the weighted mean
    of their probabilities (`ops.kernels.ensemble_logprobs`, bf16 on the GPU:
    the scores are those of the rounded, renormalised mixture). A step is then
    listed as (combined, token, fin, member_logits). One member skips the
    combine step and is bitwise that model."""
    if n < 1:
        raise ValueError(f"n must be at least 1, got {n}")
    models, weights = members(model)
    cfg = models[0].cfg
    dev = models[0].device
    src = src.to(dev)
    B = src.shape[0]
    R = B * n
    V = cfg.tgt_vocab
    for m in models:
        if max_length + 1 > m.cfg.max_tgt_len:
            raise ValueError(f"max_length {max_length} + 1 > positional table {m.cfg.max_tgt_len}")
    src_len = seq_lengths(src)
    dec = [DecoderStep(m, src, src_len, R, max_length) for m in models]
    rows = torch.arange(R, dtype=torch.int32, device=dev)
    row_map = torch.div(rows, n, rounding_mode="floor").to(torch.int32)
    if isinstance(row_id0, int):
        row_id = rows.long() + row_id0
    else:  # one base per sentence: its samples are base .. base + n - 1
        base = torch.as_tensor(row_id0, dtype=torch.int64).to(dev)
        if base.shape != (B,):
            raise ValueError(f"row_id0 must be an int or one int per sentence, got shape {tuple(base.shape)}")
        row_id = base[row_map.long()] + rows.long() % n
    row_id = row_id & 0xFFFFFFFF  # 32 bits of identity, as int32
    row_id = torch.where(row_id >= 2 ** 31, row_id - 2 ** 32, row_id).to(torch.int32)
    cross_len = src_len[row_map.long()].to(torch.int32).contiguous()
    score = torch.zeros(R, dtype=torch.float32, device=dev)
    fin = torch.zeros(R, dtype=torch.int32, device=dev)
    hist = [torch.full((R,), start, dtype=torch.int64, device=dev)]
    steps = []
    for t in range(max_length):
        tok = hist[-1]
        klen = torch.full((R,), t + 1, dtype=torch.int32, device=dev)
        lgs = [st.logits(tok, t, klen, cross_len, row_map=row_map) for st in dec]
        lg = lgs[0] if len(lgs) == 1 else K.ensemble_logprobs(lgs, V, weights)
        score, token, fin = K.sample_token(lg, V, score, fin, end, PAD_ID, temperature=temperature,
                                           top_k=top_k, top_p=top_p, seed=seed, step=t, row_id=row_id)
        if return_steps:
            steps.append((lg, token, fin) if len(lgs) == 1 else (lg, token, fin, lgs))
        hist.append(token.long())
        if bool(fin.all()):
            break
    tokens = torch.stack(hist, dim=1).view(B, n, len(hist))
    if return_steps:
        return tokens, score.view(B, n), steps
    return tokens, score.view(B, n)
