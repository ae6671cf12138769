"""Character n-gram overlap (csrc/kernels/chrf.hip): chrF's clipped match
counts between pairs of rows of code points -- the GPU arm with its CPU arm."""
from __future__ import annotations

import torch

from tensorflow_distributed_on_gke_amd.ops._ext import C

CHRF_MAX_L = 2048
CHRF_ORDERS = 6


def char_ngram_matches_torch(chr, length, pair_a, pair_b, chunk_elems: int = 1 << 24):
    """`char_ngram_matches` as a composition of torch ops, on the tensors'
    device: `ngram_matches_torch`'s broadcast formulation (per pair an
    equality tensor [L, L] of x against y and of x against itself, ANDs of its
    diagonal shifts, m_n = sum_i [r_n(i) < c_n(i)]) over six orders,
    `chunk_elems` elements of such a tensor at a time. The CPU arm, and the
    composition the kernel is measured against."""
    N, L = chr.shape
    P = pair_a.numel()
    dev = chr.device
    out = torch.full((P, CHRF_ORDERS), -1, dtype=torch.int32, device=dev)
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
    res = torch.zeros(P, CHRF_ORDERS, dtype=torch.int32, device=dev)
    for p0 in range(0, P, step):
        ia, ib = a[p0:p0 + step], b[p0:p0 + step]
        # a character is its low 21 bits, the kernel's field
        X, Y = ((chr[i, :Lm] & 0x1FFFFF).clamp(max=0x1FFFFE) for i in (ia, ib))
        lx, ly = ln[ia].view(-1, 1), ln[ib].view(-1, 1)
        exy = X.unsqueeze(2) == Y.unsqueeze(1)  # [p, i, j]
        exx = X.unsqueeze(2) == X.unsqueeze(1)
        gxy, gxx = exy, exx
        for n in range(1, CHRF_ORDERS + 1):
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


def char_ngram_matches(chr, length, pair_a, pair_b):
    """Clipped character n-gram match counts between pairs of rows, n = 1..6.

    chr int32 [N, L] of Unicode code points (1 <= L <= 2048, any row stride
    >= L), length int32 [N], pair_a / pair_b int32 [P] -> int32 [P, 6]. With x
    = chr[pair_a[p], :length[pair_a[p]]] and y likewise of pair_b[p], column
    n - 1 of row p is m_n = sum over the distinct n-grams g of x of
    min(count_x(g), count_y(g)): chrF's match count, symmetric in x and y; a
    row paired with itself gives max(len - n + 1, 0). Only positions below a
    row's length count (a length outside [0, L] is clamped into it). Code
    point 0 is an ordinary character. A value outside [0, 0x10FFFF] is the
    caller's error: its low 21 bits are taken (and 0x1FFFFF as 0x1FFFFE).
    A pair with an index outside [0, N) gets -1 in all six columns. Exact
    integers, no atomics: the result does not depend on the order or number
    of pairs. GPU: every row's n-gram keys are sorted once, then a wave per
    pair searches (csrc/kernels/chrf.hip); the scratch for the sorted keys
    and their ranks, 32 bytes per character, is allocated here. CPU:
    `char_ngram_matches_torch`."""
    if chr.dim() != 2 or chr.dtype != torch.int32:
        raise RuntimeError(f"char_ngram_matches: chr must be int32 [N, L], got {chr.dtype} {tuple(chr.shape)}")
    N, L = chr.shape
    if not 1 <= L <= CHRF_MAX_L:
        raise RuntimeError(f"char_ngram_matches: L {L} outside [1, {CHRF_MAX_L}]")
    for name, t, size in (("length", length, N), ("pair_a", pair_a, pair_a.numel()),
                          ("pair_b", pair_b, pair_a.numel())):
        if t.dim() != 1 or t.numel() != size or t.dtype != torch.int32 or t.device != chr.device:
            raise RuntimeError(f"char_ngram_matches: {name} must be int32 [{size}] on chr's device, got "
                               f"{t.dtype} {tuple(t.shape)} on {t.device}")
    P = pair_a.numel()
    if chr.is_cuda:
        out = torch.empty(P, CHRF_ORDERS, dtype=torch.int32, device=chr.device)
        keys = torch.empty(N, L, 2, dtype=torch.int64, device=chr.device)
        ranks = torch.empty(N, L, 8, dtype=torch.int16, device=chr.device)
        C().char_ngram_matches(chr, length.contiguous(), pair_a.contiguous(), pair_b.contiguous(), out,
                               keys, ranks)
        return out
    return char_ngram_matches_torch(chr, length, pair_a, pair_b)
