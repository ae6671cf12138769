"""Minimum-Bayes-risk selection: of n candidate translations of one source,
keep the one closest to all the others -- the highest expected utility when
the candidates themselves stand in as references. It needs no model, only a
pairwise utility, here a smoothed sentence BLEU.

All n (n - 1) / 2 unordered pairs of every group go through one
`ops.kernels.overlap.ngram_matches` launch (csrc/kernels/overlap.hip), which
returns the clipped n-gram match counts; u(i, j) and u(j, i) come from the same
counts, the diagonal from the lengths. What follows the counts is a handful of
f64 torch ops on the tokens' device: no per-group host loop, no device-to-host
copy.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from tensorflow_distributed_on_gke_amd.ops.kernels.overlap import NGRAM_MAX_L, ngram_matches


def sentence_bleu(m: torch.Tensor, len_h: torch.Tensor, len_r: torch.Tensor) -> torch.Tensor:
    """Smoothed sentence BLEU (f64) of hypotheses of `len_h` tokens against
    references of `len_r` from their clipped match counts m [..., 4] (len_h,
    len_r broadcast against m[..., 0]): p_1 = m_1 / len_h, p_n = (m_n + 1) /
    (max(len_h - n + 1, 0) + 1) for n = 2..4 (Lin & Och's add-one), BP = min(1,
    exp(1 - len_r / len_h)), u = BP * exp(1/4 sum log p_n); 0 when len_h == 0
    or m_1 == 0. So u(h, h) = 1 for every non-empty h."""
    m = m.double()
    lh, lr = len_h.double().unsqueeze(-1), len_r.double()
    k = torch.arange(1, 4, dtype=torch.float64, device=m.device)
    num = torch.cat([m[..., :1], m[..., 1:] + 1.0], dim=-1)
    den = torch.cat([lh.clamp(min=1.0), (lh - k).clamp(min=0.0) + 1.0], dim=-1)
    zero = (lh.squeeze(-1) == 0) | (m[..., 0] == 0)
    logs = torch.log(torch.where(zero.unsqueeze(-1), torch.ones_like(num), num) / den).sum(dim=-1)
    bp = torch.exp((1.0 - lr / lh.squeeze(-1).clamp(min=1.0)).clamp(max=0.0))
    return torch.where(zero, torch.zeros_like(logs), bp * torch.exp(0.25 * logs))


def candidate_rows(tokens: torch.Tensor, end: int, pad_id: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """tokens int64 [B, n, 1 + T] ([START] first) -> (tok int32 [B * n,
    max(T, 1)], length int32 [B * n]): a candidate's content is its tokens
    after [START] up to, and excluding, the first `end`, less the `pad_id`s
    it ends in (the padding of a row that stopped without an `end`)."""
    B, n = tokens.shape[:2]
    body = tokens[:, :, 1:]
    T = body.shape[2]
    if T > NGRAM_MAX_L:
        raise ValueError(f"mbr_select: candidates of up to {T} tokens, more than {NGRAM_MAX_L}")
    if T == 0:
        return (torch.zeros(B * n, 1, dtype=torch.int32, device=tokens.device),
                torch.zeros(B * n, dtype=torch.int32, device=tokens.device))
    before_end = (body == end).long().cumsum(dim=2) == 0
    pos = torch.arange(1, T + 1, device=tokens.device)
    length = (pos * (before_end & (body != pad_id))).max(dim=2).values
    return body.reshape(B * n, T).to(torch.int32), length.reshape(B * n).to(torch.int32)


def pairwise_utility(tok: torch.Tensor, length: torch.Tensor, B: int, n: int) -> torch.Tensor:
    """f64 [B, n, n]: u[b, i, j] = sentence_bleu of candidate i of group b as
    the hypothesis against candidate j as the reference (rows b * n + i of
    tok / length)."""
    dev = tok.device
    iu = torch.triu_indices(n, n, 1, device=dev)
    base = (torch.arange(B, device=dev) * n).view(B, 1)
    pair_a = (base + iu[0]).reshape(-1).to(torch.int32)
    pair_b = (base + iu[1]).reshape(-1).to(torch.int32)
    m = ngram_matches(tok, length, pair_a, pair_b).view(B, -1, 4)
    ln = length.view(B, n).long()
    M = torch.empty(B, n, n, 4, dtype=torch.int32, device=dev)
    M[:, iu[0], iu[1]] = m
    M[:, iu[1], iu[0]] = m
    d = torch.arange(n, device=dev)
    # a row against itself: every n-gram it has
    M[:, d, d] = (ln.unsqueeze(-1) - torch.arange(4, device=dev)).clamp(min=0).to(torch.int32)
    return sentence_bleu(M, ln.view(B, n, 1), ln.view(B, 1, n))


@torch.no_grad()
def mbr_select(tokens: torch.Tensor, end: int, pad_id: int, valid: Optional[torch.Tensor] = None
               ) -> Tuple[torch.Tensor, torch.Tensor]:
    """tokens int64 [B, n, 1 + T] -> (best int64 [B], expected f64 [B, n]) on
    the tokens' device. `valid` (bool [B, n], default all): an invalid slot
    (an n-best slot of score -inf) is neither a hypothesis nor a reference.
    expected[b, i] = the mean over the valid j, i itself included, of u(i, j)
    (`sentence_bleu` on the candidates' contents, `candidate_rows`), -inf for
    an invalid i; best = its argmax, ties to the lower index, 0 for a group
    without a valid candidate. Candidates with equal content get bitwise equal
    expected utilities, so among duplicates the first wins."""
    if tokens.dim() != 3 or tokens.shape[1] < 1 or tokens.shape[2] < 1:
        raise ValueError(f"mbr_select: tokens must be [B, n, 1 + T], got {tuple(tokens.shape)}")
    B, n = tokens.shape[:2]
    dev = tokens.device
    valid = torch.ones(B, n, dtype=torch.bool, device=dev) if valid is None else valid.to(dev)
    tok, length = candidate_rows(tokens, end, pad_id)
    u = pairwise_utility(tok, length, B, n)
    count = valid.sum(dim=1).clamp(min=1).double().view(B, 1)
    expected = (u * valid.double().view(B, 1, n)).sum(dim=2) / count
    expected = expected.masked_fill(~valid, float("-inf"))
    top = expected.max(dim=1, keepdim=True).values
    idx = torch.arange(n, device=dev).view(1, n).expand(B, n)
    best = torch.where(expected == top, idx, torch.full_like(idx, n)).min(dim=1).values
    return best, expected


def select_text(groups, lowercase: bool = False, device=None, pairs_per_launch: int = 1 << 22):
    """MBR selection among candidate strings, without a model: `groups` is a
    list of candidate lists, a candidate's units are its whitespace-separated
    words (`lowercase` folds case first) -> per group (index of the kept
    candidate, its expected utility), ties to the first. Groups of unequal
    size are padded with invalid slots; about `pairs_per_launch` candidate
    pairs go through one `mbr_select`. A candidate of more than 512 words is
    a ValueError that names its group and position."""
    PAD, END, FIRST = 0, 1, 2
    ids: dict = {}
    rows = []
    for g, cands in enumerate(groups):
        if not cands:
            raise ValueError(f"group {g + 1} has no candidate")
        for k, c in enumerate(cands):
            words = (c.lower() if lowercase else c).split()
            if len(words) > NGRAM_MAX_L:
                raise ValueError(f"candidate {k + 1} of group {g + 1} has {len(words)} words, more "
                                 f"than {NGRAM_MAX_L}")
            rows.append([ids.setdefault(w, len(ids) + FIRST) for w in words])
    dev = torch.device(device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu"))
    out = []
    g0 = r0 = 0
    while g0 < len(groups):
        # consecutive groups while the padded pair count stays within the budget
        g1, n = g0, 0
        while g1 < len(groups):
            n_new = max(n, len(groups[g1]))
            if g1 > g0 and (g1 + 1 - g0) * n_new * n_new > pairs_per_launch:
                break
            g1, n = g1 + 1, n_new
        B = g1 - g0
        sizes = [len(g) for g in groups[g0:g1]]
        T = max(1, max(len(r) for r in rows[r0:r0 + sum(sizes)]))
        tokens = torch.full((B, n, 1 + T), PAD, dtype=torch.int64)  # a row's content ends at its padding
        r = r0
        for b, size in enumerate(sizes):
            for i in range(size):
                row = rows[r]
                tokens[b, i, 1:1 + len(row)] = torch.tensor(row, dtype=torch.int64)
                r += 1
        valid = torch.arange(n).view(1, n) < torch.tensor(sizes).view(B, 1)
        best, expected = mbr_select(tokens.to(dev), END, PAD, valid.to(dev))
        util = expected.gather(1, best.view(B, 1)).view(B)
        out += list(zip(best.tolist(), util.tolist()))
        g0, r0 = g1, r
    return out
