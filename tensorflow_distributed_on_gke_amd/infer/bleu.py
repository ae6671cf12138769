"""Corpus BLEU (Papineni et al. 2002) of a hypothesis file against one
reference per line, on the n-gram match kernel.

No tokenisation or detokenisation is applied: the units are the
whitespace-separated words of the lines as given, which corresponds to a
"tokenize none" BLEU. Tokenise both sides beforehand, the same way, if scores
are to be compared with those of a tool that tokenises.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Sequence, Tuple

import torch

from tensorflow_distributed_on_gke_amd.ops.kernels.overlap import NGRAM_MAX_L, ngram_matches


class Bleu(NamedTuple):
    score: float                     # 100 * BP * exp(1/4 sum log p_n); 0 if a sum of matches is 0
    precisions: Tuple[float, ...]    # p_1 .. p_4 = matches / totals
    bp: float                        # 1 if hyp_len >= ref_len, else exp(1 - ref_len / hyp_len)
    hyp_len: int
    ref_len: int
    matches: Tuple[int, ...]         # sum over the lines of the clipped n-gram matches
    totals: Tuple[int, ...]          # sum over the lines of max(len_h - n + 1, 0)


def corpus_bleu(hyps: Sequence[str], refs: Sequence[str], lowercase: bool = False,
                device: Optional[str] = None) -> Bleu:
    """BLEU of `hyps` against `refs`, line k against line k, over
    whitespace-separated words as given (no tokenisation: see the module
    docstring); `lowercase` folds case first. The words of both sides get
    int32 ids from one dictionary, all 2N lines are packed into one [2N, L]
    matrix and a single `ngram_matches` launch on `device` (default: the GPU
    if there is one) counts the pairs (k, N + k). A line of more than 512
    words is a ValueError that names it: nothing is truncated."""
    if len(hyps) != len(refs):
        raise ValueError(f"corpus_bleu: {len(hyps)} hypotheses for {len(refs)} references")
    ids: dict = {}
    rows = []
    for side, lines in (("hypothesis", hyps), ("reference", refs)):
        for k, line in enumerate(lines):
            words = (line.lower() if lowercase else line).split()
            if len(words) > NGRAM_MAX_L:
                raise ValueError(f"corpus_bleu: {side} line {k + 1} has {len(words)} words, more "
                                 f"than {NGRAM_MAX_L}")
            rows.append([ids.setdefault(w, len(ids)) for w in words])
    N = len(hyps)
    lens = [len(r) for r in rows]
    hyp_len, ref_len = sum(lens[:N]), sum(lens[N:])
    totals = tuple(sum(max(n - k, 0) for n in lens[:N]) for k in range(4))
    matches = (0, 0, 0, 0)
    if N:
        dev = torch.device(device if device is not None else
                           ("cuda" if torch.cuda.is_available() else "cpu"))
        L = max(1, max(lens))
        length = torch.tensor(lens, dtype=torch.int32)
        tok = torch.zeros(2 * N, L, dtype=torch.int32)
        tok[torch.arange(L).view(1, L) < length.view(-1, 1)] = torch.tensor(
            [t for r in rows for t in r], dtype=torch.int32)
        k = torch.arange(N, dtype=torch.int32)
        m = ngram_matches(tok.to(dev), length.to(dev), k.to(dev), (k + N).to(dev))
        matches = tuple(int(v) for v in m.sum(dim=0, dtype=torch.int64).tolist())
    prec = tuple(m / t if t else 0.0 for m, t in zip(matches, totals))
    bp = 1.0 if hyp_len >= ref_len else (math.exp(1.0 - ref_len / hyp_len) if hyp_len else 0.0)
    score = 0.0
    if min(matches) > 0:
        score = 100.0 * bp * math.exp(0.25 * sum(math.log(p) for p in prec))
    return Bleu(score, prec, bp, hyp_len, ref_len, matches, totals)


def format_bleu(b: Bleu) -> str:
    """`BLEU = 44.15 77.8/57.1/40.0/33.3 (BP = 0.895 ratio = 0.900 hyp_len = 9 ref_len = 10)`"""
    ratio = b.hyp_len / b.ref_len if b.ref_len else 0.0
    return (f"BLEU = {b.score:.2f} " + "/".join(f"{100.0 * p:.1f}" for p in b.precisions)
            + f" (BP = {b.bp:.3f} ratio = {ratio:.3f} hyp_len = {b.hyp_len} ref_len = {b.ref_len})")
