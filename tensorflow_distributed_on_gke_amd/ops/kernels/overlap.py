"""N-gram overlap (csrc/kernels/overlap.hip): BLEU's clipped match counts
between pairs of token rows -- the GPU arm with its CPU arm."""
from __future__ import annotations

import torch

from tensorflow_distributed_on_gke_amd.ops._ext import C

NGRAM_MAX_L = 512


def ngram_matches_torch(tok, length, pair_a, pair_b, chunk_elems: int = 1 << 24):
    """`ngram_matches` as a composition of torch ops, on the tensors' device:
    per pair a broadcast equality tensor [L, L] of x against y and of x
    against itself, ANDs of its diagonal shifts for n = 2..4, and the rank /
    count sums of the kernel's formulation (m_n = sum_i [r_n(i) < c_n(i)]),
    `chunk_elems` elements of such a tensor at a time. The CPU arm, and the
    composition the kernel is measured against."""
    N, L = tok.shape
    P = pair_a.numel()
    dev = tok.device
    out = torch.full((P, 4), -1, dtype=torch.int32, device=dev)
    if P == 0 or N == 0:
        return out
    ln = length.long().clamp(0, L)
    a, b = pair_a.long(), pair_b.long()
    ok = (a >= 0) & (a < N) & (b >= 0) & (b < N)
    a, b = a.clamp(0, N - 1), b.clamp(0, N - 1)
    Lm = max(1, int(ln.max()))
    pos = torch.arange(Lm, device=dev)
    below = pos.view(1, Lm) < pos.view(Lm, 1)  # [i, j]: j < i
    step = max(1, chunk_elems // (Lm * Lm))
    res = torch.zeros(P, 4, dtype=torch.int32, device=dev)
    for p0 in range(0, P, step):
        ia, ib = a[p0:p0 + step], b[p0:p0 + step]
        X, Y = tok[ia, :Lm], tok[ib, :Lm]
        lx, ly = ln[ia].view(-1, 1), ln[ib].view(-1, 1)
        exy = X.unsqueeze(2) == Y.unsqueeze(1)  # [p, i, j]
        exx = X.unsqueeze(2) == X.unsqueeze(1)
        gxy, gxx = exy, exx
        for n in range(1, 5):
            W = Lm - n + 1  # n-gram start positions
            if W <= 0:
                break
            if n > 1:
                gxy = gxy[:, :-1, :-1] & exy[:, n - 1:, n - 1:]
                gxx = gxx[:, :-1, :-1] & exx[:, n - 1:, n - 1:]
            vi = pos[:W].view(1, W) + n <= lx  # the n-gram at i lies inside x
            vj = pos[:W].view(1, W) + n <= ly
            c = (gxy & vj.unsqueeze(1)).sum(dim=2)
            r = (gxx & below[:W, :W]).sum(dim=2)
            res[p0:p0 + step, n - 1] = (vi & (r < c)).sum(dim=1).to(torch.int32)
    return torch.where(ok.view(P, 1), res, out)


def ngram_matches(tok, length, pair_a, pair_b, prepass=None):
    """Clipped n-gram match counts between pairs of token rows, n = 1..4.

    tok int32 [N, L] (1 <= L <= 512, any row stride >= L), length int32 [N],
    pair_a / pair_b int32 [P] -> int32 [P, 4]. With x = tok[pair_a[p],
    :length[pair_a[p]]] and y likewise of pair_b[p], column n - 1 of row p is
    m_n = sum over the distinct n-grams g of x of min(count_x(g), count_y(g)):
    BLEU's clipped match count, symmetric in x and y; a row paired with itself
    gives max(len - n + 1, 0). Only positions below a row's length count (a
    length outside [0, L] is clamped into it) and every int32 value is a
    token. A pair with an index outside [0, N) gets -1 in all four columns.
    Exact integers, no atomics: the result does not depend on the order or
    number of pairs. GPU: one wave per pair (csrc/kernels/overlap.hip).
    `prepass` computes every row's n-gram ranks once, in a launch of its own,
    instead of once per pair inside the pair kernel: the same result, 1.6 to
    1.75 x faster where a row takes part in many pairs (MBR: 64 candidates, 63
    pairs per row; profiles/mbr_cost.txt) and 1.55 x slower where it takes part
    in one (corpus BLEU's pairs). The default does it when P >= 2 N. CPU:
    `ngram_matches_torch`."""
    if tok.dim() != 2 or tok.dtype != torch.int32:
        raise RuntimeError(f"ngram_matches: tok must be int32 [N, L], got {tok.dtype} {tuple(tok.shape)}")
    N, L = tok.shape
    if not 1 <= L <= NGRAM_MAX_L:
        raise RuntimeError(f"ngram_matches: L {L} outside [1, {NGRAM_MAX_L}]")
    for name, t, size in (("length", length, N), ("pair_a", pair_a, pair_a.numel()),
                          ("pair_b", pair_b, pair_a.numel())):
        if t.dim() != 1 or t.numel() != size or t.dtype != torch.int32 or t.device != tok.device:
            raise RuntimeError(f"ngram_matches: {name} must be int32 [{size}] on tok's device, got "
                               f"{t.dtype} {tuple(t.shape)} on {t.device}")
    P = pair_a.numel()
    if tok.is_cuda:
        out = torch.empty(P, 4, dtype=torch.int32, device=tok.device)
        if prepass is None:
            prepass = P >= 2 * N
        ranks = torch.empty(N, L, 4, dtype=torch.int16, device=tok.device) if prepass else None
        C().ngram_matches(tok, length.contiguous(), pair_a.contiguous(), pair_b.contiguous(), out, ranks)
        return out
    return ngram_matches_torch(tok, length, pair_a, pair_b)
