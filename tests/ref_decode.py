"""Case tables and float64 references of the decoding ops (decode_attn,
beam_topk), shared by the CPU and the GPU tests: the CPU file proves every
case reachable by the reference, the GPU file holds the kernels to it.

Inputs are bf16-valued; a case is built once per process and never modified
(tests clone what a call writes)."""
import functools
import itertools
import math

import torch

START, END, PAD = 2, 3, 0  # infer/tokenizer.py
SENTINEL = 7.0

# ---------------------------------------------------------------- decode_attn
KV_LENS = (1, 2, 63, 64, 65, 130)  # and Lk itself: chunk edges of both head dims
ATTN_SHAPES = [(hd, H, R, Lk) for hd, H, R, Lk in
               itertools.product((16, 64), (1, 8), (1, 5, 12), (1, 65, 257))] + [(64, 8, 5, 1000)]
ATTN_VARIANTS = ("identity", "row_map", "anc")
GROUP = 4  # rows per sentence of the ancestry variant


def _bf(x):
    return x.to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def attn_case(hd, H, R, Lk, variant):
    """dict of CPU tensors: q [R, H, hd], k / v cache views, kv_len, anc /
    row_map (or None), scale, vmax = max |V|. Keys no row uses are NaN."""
    g = torch.Generator().manual_seed(1000 * hd + 100 * H + 10 * R + Lk + len(variant))
    d = H * hd
    lens = [n for n in KV_LENS if n <= Lk] + [Lk]
    kv_len = torch.tensor([lens[int(torch.randint(len(lens), (1,), generator=g))] for _ in range(R)],
                          dtype=torch.int32)
    q = _bf(torch.randn(R, H, hd, generator=g))
    anc = row_map = None
    if variant == "row_map":
        n_src = (R + 2) // 3
        big = _bf(torch.randn(n_src, Lk, 4 * d, generator=g))
        k = big[:, :, d:2 * d].unflatten(-1, (H, hd))
        v = big[:, :, 3 * d:].unflatten(-1, (H, hd))
        row_map = (torch.arange(R) // 3).to(torch.int32)
        src = row_map.long().view(R, 1).expand(R, Lk)
    else:
        n_src = R
        k = _bf(torch.randn(R, Lk, H, hd, generator=g))
        v = _bf(torch.randn(R, Lk, H, hd, generator=g))
        src = torch.arange(R).view(R, 1).expand(R, Lk)
        if variant == "anc":
            base = torch.arange(R) // GROUP * GROUP
            size = torch.minimum(torch.full((R,), GROUP), R - base)
            draw = torch.randint(1 << 20, (R, Lk), generator=g)
            src = base.view(R, 1) + draw % size.view(R, 1)
            src[torch.arange(R), kv_len.long() - 1] = torch.arange(R)
            anc = src.to(torch.int32)
    vmax = float(v.float().abs().max())
    used = torch.zeros(n_src, Lk, dtype=torch.bool)
    for r in range(R):
        n = int(kv_len[r])
        used[src[r, :n], torch.arange(n)] = True
    nan = torch.tensor(float("nan"), dtype=torch.bfloat16)
    k.masked_fill_(~used.view(n_src, Lk, 1, 1), nan)
    v.masked_fill_(~used.view(n_src, Lk, 1, 1), nan)
    return dict(q=q, k=k, v=v, kv_len=kv_len, anc=anc, row_map=row_map, src=src,
                scale=1.0 / math.sqrt(hd), vmax=vmax)


def attn_ref(c):
    """float64 softmax attention of a case -> [R, H, hd]."""
    q, k, v = c["q"].double(), c["k"].double(), c["v"].double()
    R = q.shape[0]
    out = torch.zeros_like(q)
    for r in range(R):
        n = int(c["kv_len"][r])
        js = torch.arange(n)
        kr, vr = k[c["src"][r, :n], js], v[c["src"][r, :n], js]  # [n, H, hd]
        p = torch.softmax(torch.einsum("hd,nhd->hn", q[r], kr) * c["scale"], dim=-1)
        out[r] = torch.einsum("hn,nhd->hd", p, vr)
    assert torch.isfinite(out).all()
    return out


def attn_bound(ref, vmax):
    """|out - ref| <= 2^-8 |ref| + 1e-4 max|V|: one bf16 ulp of the output
    rounding; f32 accumulation and the exponent approximation."""
    return 2.0 ** -8 * ref.abs() + 1e-4 * vmax


@functools.lru_cache(maxsize=None)
def fused_case(hd, H, R, Lk, with_anc):
    """The fused append: every row at the same step t = n - 1. `k` / `v` hold
    SENTINEL from position t on, `k_ready` / `v_ready` are the same caches with
    k_new / v_new at [r, t]."""
    g = torch.Generator().manual_seed(7 + 1000 * hd + 100 * H + 10 * R + Lk)
    n = max(1, Lk - R % 3)
    t = n - 1
    q, k_new, v_new = (_bf(torch.randn(R, H, hd, generator=g)) for _ in range(3))
    k = _bf(torch.randn(R, Lk, H, hd, generator=g))
    v = _bf(torch.randn(R, Lk, H, hd, generator=g))
    k[:, t:] = SENTINEL
    v[:, t:] = SENTINEL
    k_ready, v_ready = k.clone(), v.clone()
    k_ready[:, t], v_ready[:, t] = k_new, v_new
    anc = None
    if with_anc:
        base = torch.arange(R) // GROUP * GROUP
        size = torch.minimum(torch.full((R,), GROUP), R - base)
        anc = base.view(R, 1) + torch.randint(1 << 20, (R, Lk), generator=g) % size.view(R, 1)
        anc[:, t] = torch.arange(R)
        anc = anc.to(torch.int32)
    return dict(q=q, k=k, v=v, k_new=k_new, v_new=v_new, k_ready=k_ready, v_ready=v_ready, anc=anc,
                kv_len=torch.full((R,), n, dtype=torch.int32), scale=1.0 / math.sqrt(hd), t=t)


# ---------------------------------------------------------------- beam_topk
TOPK_SHAPES = [(V, ldl, beam, B) for (V, ldl), beam, B in
               itertools.product(((7, 8), (300, 304), (7010, 7040)), (1, 3, 4, 8), (1, 3))]
TOPK_KINDS = ("random", "initial", "all_finished", "ties")
GAP = 1e-3


def topk_ref(logits, V, score, fin, beam):
    """float64 reference of one selection step. Returns (score, parent, token,
    fin) per slot and, per sentence, the sorted candidate values (for the gap
    checks). Dead slots: score -inf, token PAD, fin 1, parent = first row."""
    R = logits.shape[0]
    B = R // beam
    x = logits[:, :V].double()
    logp = x - torch.logsumexp(x, dim=-1, keepdim=True)
    o_score = torch.full((R,), float("-inf"), dtype=torch.float64)
    o_parent = torch.zeros(R, dtype=torch.int64)
    o_token = torch.full((R,), PAD, dtype=torch.int64)
    o_fin = torch.ones(R, dtype=torch.int64)
    sorted_vals = []
    for s in range(B):
        flat = torch.full((beam, V), float("-inf"), dtype=torch.float64)  # -inf: no candidate
        for b in range(beam):
            r = s * beam + b
            sc = float(score[r])
            if sc == float("-inf"):
                continue
            if int(fin[r]):
                flat[b, PAD] = sc
            else:
                flat[b] = sc + logp[r]
        # by value, ties by the lower flat index (a stable sort)
        neg, order = torch.sort(-flat.view(-1), stable=True)
        keep = int((neg < float("inf")).sum())
        cands = list(zip(neg[: min(keep, beam + 1)].tolist(), order[: beam + 1].tolist()))
        sorted_vals.append([-c[0] for c in cands[: beam + 1]])
        for kslot in range(beam):
            r = s * beam + kslot
            o_parent[r] = s * beam
            if kslot < len(cands):
                val, idx = -cands[kslot][0], cands[kslot][1]
                b, tok = divmod(idx, V)
                o_score[r], o_parent[r], o_token[r] = val, s * beam + b, tok
                o_fin[r] = int(bool(int(fin[s * beam + b])) or tok == END)
    return o_score, o_parent, o_token, o_fin, sorted_vals


def gaps_ok(sorted_vals, planted_ties):
    """Every pair of neighbours among the best beam + 1 candidates of each
    sentence (the order of the slots and the cut) is more than GAP apart --
    or, where ties are planted, exactly equal."""
    for vals in sorted_vals:
        for a, b in zip(vals, vals[1:]):
            if not (a - b > GAP or (planted_ties and a == b)):
                return False
    return True


@functools.lru_cache(maxsize=None)
def topk_case(V, ldl, beam, B, kind):
    """Inputs of one case (CPU): logits bf16 [R, ldl] with +1e4 in the padding
    columns, score f32 [R], fin int32 [R]; plus the f64 reference. The seed is
    the first whose reference keeps the gaps (checked again by the tests)."""
    R = B * beam
    for attempt in range(200):
        g = torch.Generator().manual_seed(attempt * 7919 + V + 10 * beam + B + len(kind))
        logits = torch.full((R, ldl), 1e4).to(torch.bfloat16)
        logits[:, :V] = _bf(torch.randn(R, V, generator=g) * 3.0)
        score = -5.0 * torch.rand(R, generator=g)
        fin = torch.zeros(R, dtype=torch.int32)
        if kind == "random":
            fin[torch.rand(R, generator=g) < 0.3] = 1
            if beam > 1:
                score[1] = float("-inf")  # a dead slot among live ones
        elif kind == "initial":
            score = torch.full((B, beam), float("-inf"))
            score[:, 0] = 0.0
            score = score.reshape(R)
        elif kind == "all_finished":
            fin[(B - 1) * beam:] = 1  # the last sentence has ended altogether
        elif kind == "ties":
            # the best logit of row 0 twice in that row; rows 0 and 1 alike, with
            # equal scores: every best candidate exists 2 (beam 1) or 4 times
            top = int(logits[0, :V].float().argmax())
            logits[0, (top + 3) % V] = logits[0, top]
            if beam > 1:
                logits[1] = logits[0]
                score[1] = score[0]
                score[2:beam] -= 20.0  # the other rows stay out of the way
        ref = topk_ref(logits, V, score, fin, beam)
        if gaps_ok(ref[4], kind == "ties"):
            return dict(logits=logits, score=score.float(), fin=fin, ref=ref)
    raise AssertionError("no seed keeps the reference's gaps")
