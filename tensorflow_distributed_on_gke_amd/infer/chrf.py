"""chrF (Popović 2015): the character n-gram F-score of a hypothesis file
against one reference per line, on the sorted character n-gram kernel.

A line's units are the code points of the line with its whitespace removed; no
other normalisation is applied. The definition in `corpus_chrf` is meant to
coincide with sacreBLEU's `chrF2` (character order 6, word order 0, whitespace
excluded, eps smoothing off); that equality is UNVERIFIED, the package was not
at hand, so the definition written here is the binding one. Word n-grams
(chrF++) are out of scope.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence, Tuple

import torch

from tensorflow_distributed_on_gke_amd.ops.kernels.chrf import CHRF_MAX_L, CHRF_ORDERS, char_ngram_matches


class Chrf(NamedTuple):
    score: float                  # 100 * (1 + b^2) P R / (b^2 P + R); 0 without an effective order
    precision: float              # P: the mean over the effective orders of matches / hyp_totals
    recall: float                 # R: likewise of matches / ref_totals
    beta: float
    order: int
    hyp_chars: int
    ref_chars: int
    matches: Tuple[int, ...]      # per order, summed over the lines
    hyp_totals: Tuple[int, ...]   # sum over the lines of max(|h| - n + 1, 0)
    ref_totals: Tuple[int, ...]


def char_units(line: str, lowercase: bool = False):
    """The code points of `line` without its whitespace (`lowercase` folds case first)."""
    return [ord(c) for c in "".join((line.lower() if lowercase else line).split())]


def pack_rows(rows):
    """Lists of code points -> (chr int32 [N, max(L, 1)], length int32 [N]) on the CPU."""
    length = torch.tensor([len(r) for r in rows], dtype=torch.int32)
    L = max(1, int(length.max())) if rows else 1
    chr_ = torch.zeros(len(rows), L, dtype=torch.int32)
    chr_[torch.arange(L).view(1, L) < length.view(-1, 1)] = torch.tensor(
        [c for r in rows for c in r], dtype=torch.int32)
    return chr_, length


def sentence_chrf(m: torch.Tensor, len_h: torch.Tensor, len_r: torch.Tensor, beta: float = 2.0
                  ) -> torch.Tensor:
    """chrF in [0, 1] (f64) of hypotheses of `len_h` characters against
    references of `len_r` from their match counts m [..., K] (K <= 6 orders;
    len_h, len_r broadcast against m[..., 0]): over the orders n with both
    max(len - n + 1, 0) > 0, P = mean of m_n / hyp_n, R = mean of m_n / ref_n,
    F = (1 + b^2) P R / (b^2 P + R); 0 without such an order or when P + R = 0.
    So u(h, h) = 1 for every non-empty h."""
    m = m.double()
    k = torch.arange(m.shape[-1], dtype=torch.float64, device=m.device)
    th = (len_h.double().unsqueeze(-1) - k).clamp(min=0.0)
    tr = (len_r.double().unsqueeze(-1) - k).clamp(min=0.0)
    eff = (th > 0) & (tr > 0)
    cnt = eff.sum(dim=-1).double().clamp(min=1.0)
    p = torch.where(eff, m / th.clamp(min=1.0), torch.zeros_like(m)).sum(dim=-1) / cnt
    r = torch.where(eff, m / tr.clamp(min=1.0), torch.zeros_like(m)).sum(dim=-1) / cnt
    b2 = beta * beta
    den = b2 * p + r
    return torch.where(den > 0, (1.0 + b2) * p * r / den.clamp(min=1e-300), torch.zeros_like(den))


def corpus_chrf(hyps: Sequence[str], refs: Sequence[str], lowercase: bool = False, beta: float = 2.0,
                order: int = CHRF_ORDERS, device: Optional[str] = None) -> Chrf:
    """chrF of `hyps` against `refs`, line k against line k, over the lines'
    code points without whitespace (`char_units`). All 2N lines are packed
    into one [2N, L] matrix and a single `char_ngram_matches` launch on
    `device` (default: the GPU if there is one) counts the pairs (k, N + k).
    Per order n <= `order` the matches and both sides' n-gram totals are
    summed over the lines; over the orders with both totals > 0, P and R are
    the means of matches / totals and the score is 100 (1 + beta^2) P R /
    (beta^2 P + R), 0 without such an order or when P + R = 0 (see the module
    docstring: chrF2 as sacreBLEU defines it, unverified; no word n-grams). A
    line of more than 2048 characters is a ValueError that names it."""
    if len(hyps) != len(refs):
        raise ValueError(f"corpus_chrf: {len(hyps)} hypotheses for {len(refs)} references")
    if not 1 <= order <= CHRF_ORDERS:
        raise ValueError(f"corpus_chrf: order {order} outside [1, {CHRF_ORDERS}]")
    rows = []
    for side, lines in (("hypothesis", hyps), ("reference", refs)):
        for k, line in enumerate(lines):
            u = char_units(line, lowercase)
            if len(u) > CHRF_MAX_L:
                raise ValueError(f"corpus_chrf: {side} line {k + 1} has {len(u)} characters, more "
                                 f"than {CHRF_MAX_L}")
            rows.append(u)
    N = len(hyps)
    lens = [len(r) for r in rows]
    hyp_tot = tuple(sum(max(n - k, 0) for n in lens[:N]) for k in range(order))
    ref_tot = tuple(sum(max(n - k, 0) for n in lens[N:]) for k in range(order))
    matches = (0,) * order
    if N:
        dev = torch.device(device if device is not None else
                           ("cuda" if torch.cuda.is_available() else "cpu"))
        chr_, length = pack_rows(rows)
        k = torch.arange(N, dtype=torch.int32)
        m = char_ngram_matches(chr_.to(dev), length.to(dev), k.to(dev), (k + N).to(dev))
        matches = tuple(int(v) for v in m.sum(dim=0, dtype=torch.int64).tolist()[:order])
    eff = [n for n in range(order) if hyp_tot[n] > 0 and ref_tot[n] > 0]
    p = sum(matches[n] / hyp_tot[n] for n in eff) / len(eff) if eff else 0.0
    r = sum(matches[n] / ref_tot[n] for n in eff) / len(eff) if eff else 0.0
    b2 = beta * beta
    score = 100.0 * (1.0 + b2) * p * r / (b2 * p + r) if p + r > 0 else 0.0
    return Chrf(score, p, r, beta, order, sum(lens[:N]), sum(lens[N:]), matches, hyp_tot, ref_tot)


def format_chrf(c: Chrf) -> str:
    """`chrF2 = 38.89 (P = 38.9 R = 38.9 orders = 6 hyp_chars = 3 ref_chars = 3)`"""
    return (f"chrF{c.beta:g} = {c.score:.2f} (P = {100.0 * c.precision:.1f} R = {100.0 * c.recall:.1f} "
            f"orders = {c.order} hyp_chars = {c.hyp_chars} ref_chars = {c.ref_chars})")
