"""Word alignment from cross-attention: which source token each token of a
translation attends to.

One teacher-forced forward (no K/V cache: the target exists), with a request
in `RunCtx.align` for the cross-attention block of ONE decoder layer; that
block calls `ops.kernels.attention.attn_align` (csrc/kernels/attn_align.hip)
on its bf16 Q and K: the mean over heads of the softmax rows and its arg-max
per target position, one launch, no per-head [B, H, Lq, Lk] tensor. The
default layer is the second to last, max(1, layers - 1): among the layers of a
plain Transformer the penultimate one's head mean aligns best (Garg et al.
2019, "Jointly Learning to Align and Translate with Transformer Models").

Positions. The source row is [START] x_0 .. x_{m-1} [END]; the kernel is told
k_lo = 1, k_trim = 1, so the two special tokens keep their share of the softmax
but are never the answer, and source index = key - 1. Decoder position t
(input tgt[t], label tgt[t + 1]) stands for target token y_t = tgt[t + 1]; the
position whose label is [END] is left out (q_len = the number of real target
tokens). Of an `Ensemble` only the first member is read: the mean of several
models' attention is not an alignment any of them made.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple, Union

import torch

from tensorflow_distributed_on_gke_amd.infer.ensemble import Ensemble, members
from tensorflow_distributed_on_gke_amd.infer.score import mask_after_end
from tensorflow_distributed_on_gke_amd.infer.tokenizer import END
from tensorflow_distributed_on_gke_amd.models.layers import RunCtx
from tensorflow_distributed_on_gke_amd.models.transformer import PAD_ID, Transformer

Links = List[Tuple[int, int, float]]  # (target token, source token, conf), ascending target


def default_layer(layers: int) -> int:
    return max(1, layers - 1)


@torch.no_grad()
def align_pairs(model: Union[Transformer, Ensemble], src: torch.Tensor, tgt: torch.Tensor,
                layer: Optional[int] = None, want_soft: bool = False, end: int = END):
    """src int64 [B, S] ([START] .. [END], right-padded), tgt int64 [B, 1 + T]
    with [START] first -> per pair its `Links`: for every real target token t
    (0-based, special tokens stripped) the source token s (0-based, likewise)
    with the largest head-mean attention at decoder layer `layer` (1-based;
    default `default_layer`) and that probability. A target token whose source
    has no real token gets no link. want_soft: also, per pair, the f32 [n_tgt,
    n_src] head-mean attention over the real tokens (its rows sum to 1 minus
    the share of [START] and [END])."""
    m = members(model)[0][0]
    layer = default_layer(m.cfg.layers) if layer is None else layer
    if not 1 <= layer <= m.cfg.layers:
        raise ValueError(f"layer must be in 1..{m.cfg.layers}, got {layer}")
    dev = m.device
    src, tgt = src.to(dev), tgt.to(dev)
    B = src.shape[0]
    if tgt.shape[1] < 2:  # nothing to feed the decoder
        return ([[] for _ in range(B)], [torch.zeros(0, 0)] * B) if want_soft else [[] for _ in range(B)]
    labels = mask_after_end(tgt[:, 1:], end)
    q_len = ((labels != PAD_ID) & (labels != end)).sum(dim=1, dtype=torch.int32)
    site = m.dec_layers[layer - 1].site2
    rt = RunCtx(training=False, store=None,
                align={site: dict(q_len=q_len, k_lo=1, k_trim=1, want_soft=want_soft)})
    m.features(src, tgt[:, :-1].contiguous(), rt)
    hard, conf, soft = rt.align[site]
    hard, conf, n_tgt = hard.tolist(), conf.tolist(), q_len.tolist()
    links = [[(t, hard[b][t] - 1, conf[b][t]) for t in range(n_tgt[b]) if hard[b][t] >= 0]
             for b in range(B)]
    if not want_soft:
        return links
    n_src = ((src != PAD_ID).sum(dim=1) - 2).clamp_min(0).cpu().tolist()
    soft = soft.cpu()
    return links, [soft[b, :n_tgt[b], 1:1 + n_src[b]].clone() for b in range(B)]


def project_words(links: Links, tgt_words: Sequence[int], src_words: Sequence[int]) -> Links:
    """Token links -> word links. tgt_words / src_words: the word index of
    every token (infer/tokenizer.word_ids; -1: part of no word). Target word u
    aligns to the source word that holds the arg-max source token of u's most
    confident token (the first such token on ties); tokens outside words and
    links into a token outside words are left out."""
    best: dict = {}
    for t, s, c in links:
        u, v = tgt_words[t], src_words[s]
        if u >= 0 and v >= 0 and (u not in best or c > best[u][1]):
            best[u] = (v, c)
    return [(u, v, c) for u, (v, c) in sorted(best.items())]


def pharaoh(links: Links, min_conf: float = 0.0) -> str:
    """`s-t` pairs ascending by t, links below min_conf dropped."""
    return " ".join(f"{s}-{t}" for t, s, c in links if c >= min_conf)
