"""Beam-search decoding on the single-query KV-cache attention kernel.

Each of the B sentences keeps `beam` hypotheses, so the decoder runs on
R = B * beam rows, one new token per row and step. Three things keep a step
free of copies (csrc/kernels/decode.hip, docs/ARCHITECTURE.md "Inference"):

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

from typing import Tuple

import torch

from tensorflow_distributed_on_gke_amd.infer.greedy import _add_ln, _linear
from tensorflow_distributed_on_gke_amd.models.layers import CrossKVFn, KVGrad, RunCtx
from tensorflow_distributed_on_gke_amd.models.transformer import PAD_ID, Transformer, seq_lengths
from tensorflow_distributed_on_gke_amd.ops import kernels as K


def length_penalty(length: torch.Tensor, alpha: float) -> torch.Tensor:
    """((5 + len) / 6) ** alpha, the GNMT length normalisation."""
    return ((5.0 + length.float()) / 6.0) ** alpha


@torch.no_grad()
def beam_search(model: Transformer, src: torch.Tensor, start: int, end: int, beam: int = 4,
                max_length: int = 20, alpha: float = 0.6, reorder: str = "index"
                ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """src int64 [B, S] -> (tokens int64 [B, 1 + n], scores f32 [B],
    all_tokens int64 [B, beam, 1 + n], all_scores f32 [B, beam]).

    Scores are sums of f32 log-probabilities (an ended hypothesis keeps its
    score and is padded with PAD); `all_*` list every sentence's hypotheses by
    descending score, -inf marking a slot that never held one. `tokens` /
    `scores` are the hypothesis that maximises score / ((5 + len) / 6) **
    alpha, len counting the generated tokens including [END]; ended or not,
    all are ranked alike."""
    if reorder not in ("index", "copy"):
        raise ValueError(f"reorder must be 'index' or 'copy', got {reorder!r}")
    if not 1 <= beam <= 8:
        raise ValueError(f"beam must be in [1, 8], got {beam}")
    m = model
    cfg = m.cfg
    dev = m.device
    src = src.to(dev)
    B = src.shape[0]
    R = B * beam
    d, H = cfg.d_model, cfg.heads
    hd = d // H
    V = cfg.tgt_vocab
    scale = 1.0 / (hd ** 0.5)
    if max_length + 1 > cfg.max_tgt_len:
        raise ValueError(f"max_length {max_length} + 1 > positional table {cfg.max_tgt_len}")
    rt = RunCtx(training=False, store=None)
    src_len = seq_lengths(src)
    enc = m.encode(src, src_len, rt)
    S = enc.shape[1]
    kv_all = CrossKVFn.apply(enc, m.cross_kv.w, m.cross_kv.b, KVGrad(), rt).contiguous()
    act = m.act_dtype
    Tm = max_length + 1
    kcache = [torch.zeros(R, Tm, H, hd, dtype=act, device=dev) for _ in m.dec_layers]
    vcache = [torch.zeros(R, Tm, H, hd, dtype=act, device=dev) for _ in m.dec_layers]
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
        if dev.type == "cuda":
            x2 = K.embed_fwd(tok.view(R, 1).contiguous(), m.dec_emb.compute, m.pe_tgt[t:], d ** 0.5,
                             0.0, 0, None, 0).view(R, d)
        else:
            x2 = m.dec_emb.master[tok] * (d ** 0.5) + m.pe_tgt[t].view(1, d)
        klen = torch.full((R,), t + 1, dtype=torch.int32, device=dev)
        for li, layer in enumerate(m.dec_layers):
            qkv = _linear(x2, layer.qkv1).view(R, 3, H, hd)
            o = K.decode_attn(qkv[:, 0], kcache[li], vcache[li], klen, scale, anc=anc,
                              k_new=qkv[:, 1], v_new=qkv[:, 2])
            y = _add_ln(x2, _linear(o.reshape(R, d), layer.o1), layer.ln1)
            q2 = _linear(y, layer.q2).view(R, H, hd)
            kv5 = kv_all[:, :, li * 2 * d:(li + 1) * 2 * d].view(B, S, 2, H, hd)
            o2 = K.decode_attn(q2, kv5[:, :, 0], kv5[:, :, 1], cross_len, scale, row_map=row_map)
            y2 = _add_ln(y, _linear(o2.reshape(R, d), layer.o2), layer.ln2)
            f = _linear(_linear(y2, layer.ff1, relu=True), layer.ff2)
            x2 = _add_ln(y2, f, layer.ln3)
        lg = m.project(x2.view(R, 1, d))
        score, parent, token, fin_new, new_anc = K.beam_topk(lg, V, score, fin, beam, end, PAD_ID,
                                                             anc=anc, t=t, anc_out=nxt_anc)
        par = parent.long()
        if index:
            anc, nxt_anc = new_anc, anc
        elif t + 1 < max_length:
            for li in range(len(m.dec_layers)):
                kcache[li] = kcache[li].index_select(0, par)
                vcache[li] = vcache[li].index_select(0, par)
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
