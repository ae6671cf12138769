"""Beam-search decoding on the single-query KV-cache attention kernel.

Each of the B sentences keeps `beam` hypotheses, so the decoder runs on
R = B * beam rows, one new token per row and step (infer/step.py holds the
model's side of it). Three things keep a step free of copies
(csrc/kernels/decode.hip, docs/ARCHITECTURE.md "Inference"):

* the ancestry table: one int32 [R, Tmax] table, shared by all layers, says
  for every live hypothesis and position which cache row holds that
  position's K / V. Selecting the survivors rewrites the table (inside the
  selection kernel); no self-attention cache is ever reordered;
* the cross-attention reads the encoder K / V of sentence r // beam through a
  row map, so they exist once per sentence;
* the attention launch itself appends the step's K / V to the caches.

`reorder="copy"` is the debug mode that gathers the caches by parent every
step instead (no ancestry table); it gives bitwise the same result.
"""
from __future__ import annotations

from typing import Tuple, Union

import torch

from tensorflow_distributed_on_gke_amd.infer.ensemble import Ensemble, members
from tensorflow_distributed_on_gke_amd.infer.step import DecoderStep
from tensorflow_distributed_on_gke_amd.models.transformer import PAD_ID, Transformer, seq_lengths
from tensorflow_distributed_on_gke_amd.ops import kernels as K


def length_penalty(length: torch.Tensor, alpha: float) -> torch.Tensor:
    """((5 + len) / 6) ** alpha, the GNMT length normalisation."""
    return ((5.0 + length.float()) / 6.0) ** alpha


@torch.no_grad()
def beam_search(model: Union[Transformer, Ensemble], src: torch.Tensor, start: int, end: int,
                beam: int = 4, max_length: int = 20, alpha: float = 0.6, reorder: str = "index"
                ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """src int64 [B, S] -> (tokens int64 [B, 1 + n], scores f32 [B],
    all_tokens int64 [B, beam, 1 + n], all_scores f32 [B, beam]).

    Scores are sums of f32 log-probabilities (an ended hypothesis keeps its
    score and is padded with PAD); `all_*` list every sentence's hypotheses by
    descending score, -inf marking a slot that never held one. `tokens` /
    `scores` are the hypothesis that maximises score / ((5 + len) / 6) **
    alpha, len counting the generated tokens including [END]; ended or not,
    all are ranked alike.

    `model` may be an `Ensemble` (infer/ensemble.py): its members run on the
    same rows, one `DecoderStep` each, sharing the ancestry table, and the
    candidates are scored by the log of the weighted mean of their
    probabilities (`ops.kernels.ensemble_logprobs`, bf16 on the GPU: the
    scores are those of the rounded, renormalised mixture). One member skips
    the combine step and is bitwise that model."""
    if reorder not in ("index", "copy"):
        raise ValueError(f"reorder must be 'index' or 'copy', got {reorder!r}")
    if not 1 <= beam <= 8:
        raise ValueError(f"beam must be in [1, 8], got {beam}")
    models, weights = members(model)
    cfg = models[0].cfg
    dev = models[0].device
    src = src.to(dev)
    B = src.shape[0]
    R = B * beam
    V = cfg.tgt_vocab
    for m in models:
        if max_length + 1 > m.cfg.max_tgt_len:
            raise ValueError(f"max_length {max_length} + 1 > positional table {m.cfg.max_tgt_len}")
    src_len = seq_lengths(src)
    steps = [DecoderStep(m, src, src_len, R, max_length) for m in models]
    Tm = max_length + 1
    rows = torch.arange(R, dtype=torch.int32, device=dev)
    row_map = torch.div(rows, beam, rounding_mode="floor").to(torch.int32)
    cross_len = src_len[row_map.long()].to(torch.int32).contiguous()
    index = reorder == "index"
    anc = nxt_anc = None
    if index:
        anc = torch.zeros(R, Tm, dtype=torch.int32, device=dev)
        anc[:, 0] = rows
        nxt_anc = torch.zeros_like(anc)
    score = torch.full((B, beam), float("-inf"), dtype=torch.float32, device=dev)
    score[:, 0] = 0.0
    score = score.view(R).contiguous()
    fin = torch.zeros(R, dtype=torch.int32, device=dev)
    length = torch.zeros(R, dtype=torch.int64, device=dev)
    hist = torch.full((R, 1), start, dtype=torch.int64, device=dev)
    tok = hist[:, 0]
    for t in range(max_length):
        klen = torch.full((R,), t + 1, dtype=torch.int32, device=dev)
        lgs = [st.logits(tok, t, klen, cross_len, row_map=row_map, anc=anc) for st in steps]
        lg = lgs[0] if len(lgs) == 1 else K.ensemble_logprobs(lgs, V, weights)
        score, parent, token, fin_new, new_anc = K.beam_topk(lg, V, score, fin, beam, end, PAD_ID,
                                                             anc=anc, t=t, anc_out=nxt_anc)
        par = parent.long()
        if index:
            anc, nxt_anc = new_anc, anc
        elif t + 1 < max_length:
            for st in steps:
                st.gather(par)
        tok = token.long()
        length = length[par] + (fin[par] == 0).long()
        hist = torch.cat([hist[par], tok.view(R, 1)], dim=1)
        fin = fin_new
        if bool(fin.all()):
            break
    n1 = hist.shape[1]
    all_tokens = hist.view(B, beam, n1)
    all_scores = score.view(B, beam)
    ranked = all_scores / length_penalty(length.view(B, beam), alpha)
    # first of equal maxima: the better raw score
    best = torch.sort(-ranked, dim=1, stable=True).indices[:, 0]
    pick = torch.arange(B, device=dev)
    return all_tokens[pick, best], all_scores[pick, best], all_tokens, all_scores
