"""Decoding steps (csrc/kernels/decode.hip): single-query attention, beam
selection, sampling, the ensemble mixture and teacher-forced scoring under it
-- each GPU arm with its CPU arm."""
from __future__ import annotations

import math

import torch

from tensorflow_distributed_on_gke_amd.ops._ext import C
from tensorflow_distributed_on_gke_amd.ops.kernels.attention import _ref_attn_fwd
from tensorflow_distributed_on_gke_amd.ops.mixture import normalised_weights


def decode_attn(q, k, v, kv_len, scale: float, anc=None, row_map=None, k_new=None, v_new=None):
    """Single-query attention, one query per (row, head): q [R, H, hd], k / v
    cache views [rows, Lk, H, hd] (any row / key / head strides) -> [R, H, hd].

    Key j < kv_len[r] (int32 [R], >= 1) of row r is read from cache row
    anc[r, j] (int32 [R, >= Lk]) when `anc` is given, else from row_map[r]
    (int32 [R]), else from row r. With k_new / v_new ([R, H, hd]) the new key
    is first stored to position kv_len[r] - 1 of cache row r (in place) and
    used as that key. GPU: bf16, hd 16 or 64 (csrc/kernels/decode.hip); CPU:
    the same in f32 through attention._ref_attn_fwd."""
    R, H, hd = q.shape
    if q.is_cuda:
        out = torch.empty(R, H, hd, dtype=torch.bfloat16, device=q.device)
        C().decode_attn(q, k, v, out, kv_len, scale, anc, row_map, k_new, v_new)
        return out
    n = kv_len.long().clamp(max=k.shape[1])
    rows = torch.arange(R)
    if k_new is not None:
        k[rows, n - 1] = k_new.to(k.dtype)
        v[rows, n - 1] = v_new.to(v.dtype)
    L = int(n.max())
    keys = torch.arange(L)
    if anc is not None:
        src = anc[:, :L].long()
        if k_new is not None:  # the new key is row r's own, whatever anc says
            src = src.clone()
            src[rows, n - 1] = rows
    else:
        src = (row_map.long() if row_map is not None else rows).view(R, 1).expand(R, L)
    src = src.clamp(0, k.shape[0] - 1)
    used = (keys.view(1, L) < n.view(R, 1)).view(R, L, 1, 1)
    zero = torch.zeros((), dtype=torch.float32)
    kg = torch.where(used, k[src, keys.view(1, L)].float(), zero)  # unused keys are never read
    vg = torch.where(used, v[src, keys.view(1, L)].float(), zero)
    out = _ref_attn_fwd(q.float().view(R, 1, H, hd), kg, vg, n.to(torch.int32), False, scale)[0]
    return out.view(R, H, hd).to(q.dtype)


def beam_topk(logits, V: int, score, fin, beam: int, end_id: int, pad_id: int, anc=None, t: int = 0,
              anc_out=None):
    """One beam-search selection step for rows r = sentence * beam + slot.

    logits [R, >= V] (only the first V columns count), score f32 [R], fin
    int32 [R]. Candidate (r, v) scores score[r] + log_softmax(logits[r])[v] in
    f32; an ended row offers only (r, pad_id) with its score unchanged, a row
    of score -inf nothing. Per sentence the best `beam` candidates, ties to
    the lower flat index slot * V + v, by descending score; a slot left
    without a candidate gets score -inf, token pad_id, fin 1 and the
    sentence's first row as parent. Returns (score f32, parent int32 (global
    row), token int32, fin int32, anc'), anc' being the ancestry table
    advanced from `anc` (int32 [R, > t + 1]): anc'[r, :t+1] =
    anc[parent[r], :t+1], anc'[r, t+1] = r (None without `anc`), written into
    `anc_out` (a second table, never `anc` itself) when given; later columns
    are not defined. 1 <= beam <= 8, V <= 65536."""
    R = logits.shape[0]
    if not 1 <= beam <= 8 or not 1 <= V <= 65536:
        raise RuntimeError(f"beam_topk: beam {beam} outside [1, 8] or V {V} outside [1, 65536]")
    dev = logits.device
    if logits.is_cuda:
        score_out = torch.empty(R, dtype=torch.float32, device=dev)
        parent, token, fin_out = (torch.empty(R, dtype=torch.int32, device=dev) for _ in range(3))
        if anc is not None and anc_out is None:
            anc_out = torch.zeros_like(anc)
        C().beam_topk(logits, V, score, fin, beam, end_id, pad_id, score_out, parent, token, fin_out,
                      anc, anc_out, t)
        return score_out, parent, token, fin_out, anc_out
    B = R // beam
    x = logits[:, :V].float()
    logp = x - torch.logsumexp(x, dim=-1, keepdim=True)
    cand = score.float().view(R, 1) + logp
    ended = fin.view(R, 1) != 0
    only_pad = torch.full_like(cand, float("-inf"))
    only_pad[:, pad_id] = score.float()
    cand = torch.where(ended, only_pad, cand)
    cand = torch.where(torch.isnan(cand) | ~(score.float() > float("-inf")).view(R, 1),
                       torch.full_like(cand, float("-inf")), cand)
    flat = cand.view(B, beam * V)
    order = torch.sort(-flat, dim=-1, stable=True).indices[:, :beam]  # ties: lower flat index
    val = torch.gather(flat, 1, order)
    dead = ~(val > float("-inf"))
    base = (torch.arange(B) * beam).view(B, 1)
    parent = torch.where(dead, base.expand(B, beam), base + order // V)
    token = torch.where(dead, torch.full_like(order, pad_id), order % V)
    fin_out = dead | (fin.view(R)[parent.view(R)].view(B, beam) != 0) | (token == end_id)
    score_out = torch.where(dead, torch.full_like(val, float("-inf")), val)
    parent = parent.reshape(R).to(torch.int32)
    if anc is not None:
        if anc_out is None:
            anc_out = torch.zeros_like(anc)
        anc_out[:, : t + 1] = anc[parent.long(), : t + 1]
        anc_out[:, t + 1] = torch.arange(R, dtype=anc.dtype)
    return (score_out.reshape(R), parent, token.reshape(R).to(torch.int32),
            fin_out.reshape(R).to(torch.int32), anc_out)


def sample_uniforms(seed: int, step: int, row_id, V: int) -> torch.Tensor:
    """f64 [R, V]: the uniforms of sample_token, exactly. u[r, v] = ((w >> 9) +
    0.5) * 2**-23 with w = word v & 3 of Philox(seed, offset=step, idx =
    row_id[r] << 32 | v >> 2); 23 bits, so the value is exact in f32 too."""
    from tensorflow_distributed_on_gke_amd.ops import philox

    row_id = row_id.to(torch.int64).cpu()
    R, G = row_id.numel(), (V + 3) // 4
    idx = (row_id.view(R, 1) << 32) | torch.arange(G, dtype=torch.int64).view(1, G)
    words = torch.stack(philox.philox4x32(seed, step, idx), dim=2).view(R, 4 * G)[:, :V]
    return ((words >> 9).double() + 0.5) * 2.0 ** -23


def sample_token(logits, V: int, score, fin, end_id: int, pad_id: int, temperature: float = 1.0,
                 top_k: int = 0, top_p: float = 1.0, seed: int = 0, step: int = 0, row_id=None):
    """One sampling step per row: temperature, then top-k, then top-p, then a
    Gumbel-max draw. Returns (score f32, token int32, fin int32).

    logits [R, >= V] (only the first V columns count; finite or -inf), score
    f32 [R] (running sum of log-probabilities), fin int32 [R], row_id int32 [R]
    (the row's identity in the random stream; None = its index).
    K = {v: x_v >= the top_k-th largest logit} (ties all kept; all finite
    logits with top_k = 0 or beyond their number); S = {v in K: x_v >= t}, t
    the largest value whose mass sum_{v in K, x_v >= t} exp((x_v - max x) / T)
    reaches top_p of K's (top_p = 1: S = K). token = argmax over S of x_v / T -
    log(-log u_v), ties to the lower v, u as in `sample_uniforms`: a draw from
    softmax(x / T) restricted to S, the same on the CPU and the GPU wherever
    the two best keys are not within rounding. score += log_softmax(x)[token]
    (T = 1, unfiltered: what beam_topk accumulates), fin = token == end_id. An
    ended row: pad_id, score unchanged, fin 1; a row of score -inf / NaN or
    without a finite logit: pad_id, -inf, fin 1. GPU: csrc/kernels/decode.hip;
    CPU: the same definition in f32."""
    R = logits.shape[0]
    if not 1 <= V <= 65536:
        raise RuntimeError(f"sample_token: V {V} outside [1, 65536]")
    if not (0.0 < temperature < float("inf")) or not 0.0 < top_p <= 1.0 or top_k < 0:
        raise RuntimeError(f"sample_token: temperature {temperature} must be finite and > 0, "
                           f"top_p {top_p} in (0, 1], top_k {top_k} >= 0")
    if not (0 <= pad_id < V and 0 <= end_id < V):
        raise RuntimeError("sample_token: pad / end id outside [0, V)")
    dev = logits.device
    seed, step = seed & (2 ** 64 - 1), step & (2 ** 64 - 1)
    if logits.is_cuda:
        score_out = torch.empty(R, dtype=torch.float32, device=dev)
        token, fin_out = (torch.empty(R, dtype=torch.int32, device=dev) for _ in range(2))
        s64 = lambda x: x - 2 ** 64 if x >= 2 ** 63 else x  # the same 64 bits, signed
        C().sample_token(logits, V, score, fin, end_id, pad_id, temperature, top_k, top_p, s64(seed),
                         s64(step), row_id, score_out, token, fin_out)
        return score_out, token, fin_out
    ninf = float("-inf")
    x = logits[:, :V].float()
    score = score.float()
    valid = x > ninf
    nfin = valid.sum(dim=1)
    ended = fin.view(R) != 0
    dead = ~ended & (~(score > ninf) | (nfin == 0))
    xs = torch.sort(torch.where(valid, x, torch.full_like(x, ninf)), dim=1, descending=True).values
    kth = torch.full_like(nfin, top_k - 1) if top_k > 0 else nfin - 1
    kth = torch.where(kth < nfin, kth, nfin - 1).clamp(min=0)
    tau = xs.gather(1, kth.view(R, 1))
    keep = valid & (x >= tau)
    T = torch.tensor(temperature, dtype=torch.float32)
    if top_p < 1.0:
        mx = torch.where(nfin > 0, xs[:, 0], torch.zeros(R)).view(R, 1)
        ws = torch.where((xs > ninf) & (xs >= tau), torch.exp((xs - mx) / T), torch.zeros(()))
        cum = torch.cumsum(ws, dim=1)
        # mass of {x >= xs[j]}: the running sum where xs[j]'s run of equal values ends
        last = torch.ones_like(xs, dtype=torch.bool)
        last[:, :-1] = xs[:, :-1] != xs[:, 1:]
        ends = torch.where(last, cum, torch.full_like(cum, float("inf")))
        mass = torch.flip(torch.cummin(torch.flip(ends, [1]), dim=1).values, [1])
        ok = mass >= torch.tensor(top_p, dtype=torch.float32) * cum[:, -1:]
        first = ok.to(torch.int32).argmax(dim=1)
        keep &= x >= xs.gather(1, first.view(R, 1))
    rid = torch.arange(R) if row_id is None else row_id
    u = sample_uniforms(seed, step, rid, V).float()
    key = torch.where(keep, x / T - torch.log(-torch.log(u)), torch.full_like(x, ninf))
    token = key.argmax(dim=1)  # the first of equal maxima
    lse = torch.logsumexp(torch.where(valid, x, torch.full_like(x, ninf)), dim=1)
    out = score + (x.gather(1, token.view(R, 1)).view(R) - lse)
    off = ended | dead
    token = torch.where(off, torch.full_like(token, pad_id), token)
    out = torch.where(ended, score, torch.where(dead, torch.full_like(out, ninf), out))
    return out, token.to(torch.int32), (off | (token == end_id)).to(torch.int32)


ENSEMBLE_MAX = 8


def _mixture_args(who: str, logits_list, V: int, weights):
    """The member count and vocabulary size in range, or RuntimeError; the
    weights, normalised."""
    M = len(logits_list)
    if not 1 <= M <= ENSEMBLE_MAX:
        raise RuntimeError(f"{who}: {M} members outside [1, {ENSEMBLE_MAX}]")
    if not 1 <= V <= 65536:
        raise RuntimeError(f"{who}: V {V} outside [1, 65536]")
    return normalised_weights(M, weights, f"{who}: needs {M} finite weights > 0")


def _mixture(logits_list, V: int, w) -> torch.Tensor:
    """The CPU definition of the mixture, f32 [R, V] (`ensemble_logprobs`)."""
    ninf = float("-inf")
    rows = []
    for x, wm in zip(logits_list, w):
        x = x[:, :V].float()
        x = torch.where(x > ninf, x, torch.full_like(x, ninf))  # NaN too
        lse = torch.logsumexp(x, dim=1, keepdim=True)
        rows.append(torch.where(lse > ninf, x - lse + math.log(wm), torch.full_like(x, ninf)))
    return torch.logsumexp(torch.stack(rows), dim=0)


def ensemble_logprobs(logits_list, V: int, weights=None, out=None):
    """The log of the weighted mean of M members' next-token probabilities.

    logits_list: 1 to 8 tensors [R, >= V] (only the first V columns count; a
    NaN or -inf logit has probability 0), weights: one positive number per
    member (default uniform), normalised here to sum 1. With lse_m[r] =
    logsumexp_v x_m[r, v] and a_m = x_m - lse_m + log w_m (-inf throughout a
    member's row without a finite logit), out[r, v] = logsumexp_m a_m[r, v]; a
    row no member has a finite logit in is all -inf, as are the columns from
    V on. Returns `out`, [R, multiple of 8 >= V] (default: V rounded up).
    GPU: bf16 members, each with its own row stride (a multiple of 8, rows
    16-byte aligned), f32 arithmetic, bf16 output: the rounded mixture, which
    the selection kernels renormalise (csrc/kernels/decode.hip). CPU: the same
    definition in f32, unrounded."""
    w = _mixture_args("ensemble_logprobs", logits_list, V, weights)
    first = logits_list[0]
    R = first.shape[0]
    if first.is_cuda:
        if out is None:
            out = torch.empty(R, (V + 7) // 8 * 8, dtype=torch.bfloat16, device=first.device)
        C().ensemble_logprobs(list(logits_list), V, w, out)
        return out
    ninf = float("-inf")
    mix = _mixture(logits_list, V, w)
    if out is None:
        out = torch.empty(R, (V + 7) // 8 * 8, dtype=torch.float32)
    if out.shape[0] != R or out.shape[1] < V:
        raise RuntimeError(f"ensemble_logprobs: out {tuple(out.shape)} too small for [{R}, {V}]")
    out[:, :V] = mix
    out[:, V:] = ninf
    return out


def score_tokens(logits_list, V: int, labels, weights=None, pad_id: int = 0, want_top: bool = False):
    """Teacher-forced scores of one label per row under the mixture of
    `ensemble_logprobs`, without the [R, V] mixture ever being stored.

    logits_list, V, weights: as `ensemble_logprobs`; labels: int32 or int64
    [R]. With mix = the mixture defined there, tok_lp[r] = mix[r, labels[r]]
    (-inf for a label outside [0, V) or a column of probability 0) and
    top_lp[r] = max_v mix[r, v]; a row whose label is pad_id is ignored: both
    are 0 and its logits are not read. Returns (tok_lp f32 [R], top_lp f32 [R]
    or None without `want_top`). The label's column goes through the same
    arithmetic as every other, so tok_lp >= top_lp says exactly whether the
    label is a most probable token. GPU: bf16 members as for
    `ensemble_logprobs`, f32 arithmetic and outputs (csrc/kernels/decode.hip
    score_tokens); CPU: the same definition in f32."""
    w = _mixture_args("score_tokens", logits_list, V, weights)
    first = logits_list[0]
    R = first.shape[0]
    if labels.dim() != 1 or labels.numel() != R or labels.dtype not in (torch.int32, torch.int64):
        raise RuntimeError(f"score_tokens: labels must be int32 or int64 [{R}], got {labels.dtype} "
                           f"{tuple(labels.shape)}")
    if first.is_cuda:
        tok_lp = torch.empty(R, dtype=torch.float32, device=first.device)
        top_lp = torch.empty(R, dtype=torch.float32, device=first.device) if want_top else None
        C().score_tokens(list(logits_list), V, w, labels, pad_id, tok_lp, top_lp)
        return tok_lp, top_lp
    ninf = float("-inf")
    mix = _mixture(logits_list, V, w)
    lab = labels.long()
    ignored = lab == pad_id
    inside = (lab >= 0) & (lab < V)
    zero = torch.zeros(R, dtype=torch.float32)
    tok_lp = mix.gather(1, lab.clamp(0, V - 1).view(R, 1)).view(R)
    tok_lp = torch.where(inside, tok_lp, torch.full_like(tok_lp, ninf))
    tok_lp = torch.where(ignored, zero, tok_lp)
    top_lp = torch.where(ignored, zero, mix.max(dim=1).values) if want_top else None
    return tok_lp, top_lp
