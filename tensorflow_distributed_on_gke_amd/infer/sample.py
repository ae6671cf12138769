"""Sampled decoding (temperature, top-k, top-p) on the single-query KV-cache
attention kernel.

Each of the B sentences draws `n` translations, so the decoder runs on
R = B * n rows (r = sentence * n + sample), one new token per row and step.
The loop is beam search's (infer/beam.py) without the ancestry table: a
sample never changes rows, so the self-attention runs on identity rows with
the K / V append fused into the launch, and the cross-attention reads the
encoder K / V of sentence r // n through a row map. The selection step is
`ops.kernels.sample_token` (csrc/kernels/decode.hip): row r draws from the
Philox stream of (seed, step t, row_id0 + r), so a row's translation depends
on its identity, not on what else is in the batch.
"""
from __future__ import annotations

import torch

from tensorflow_distributed_on_gke_amd.infer.greedy import _add_ln, _linear
from tensorflow_distributed_on_gke_amd.models.layers import CrossKVFn, KVGrad, RunCtx
from tensorflow_distributed_on_gke_amd.models.transformer import PAD_ID, Transformer, seq_lengths
from tensorflow_distributed_on_gke_amd.ops import kernels as K


@torch.no_grad()
def sample_search(model: Transformer, src: torch.Tensor, start: int, end: int, n: int = 1,
                  max_length: int = 20, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0,
                  seed: int = 0, row_id0: int = 0, return_steps: bool = False):
    """src int64 [B, S] -> (tokens int64 [B, n, 1 + len], scores f32 [B, n]).

    Scores are sums of the model's own f32 log-probabilities (T = 1,
    unfiltered: comparable with beam search's); an ended row keeps its score
    and is padded with PAD. Row r's identity in the random stream is
    row_id0 + r, or, with one `row_id0` per sentence, row_id0[r // n] + r % n.
    With `return_steps` a third value lists, per step,
    the (logits [R, >= V], token int32 [R], fin int32 [R]) the step saw and
    gave."""
    if n < 1:
        raise ValueError(f"n must be at least 1, got {n}")
    m = model
    cfg = m.cfg
    dev = m.device
    src = src.to(dev)
    B = src.shape[0]
    R = B * n
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
    row_map = torch.div(rows, n, rounding_mode="floor").to(torch.int32)
    if isinstance(row_id0, int):
        row_id = rows.long() + row_id0
    else:  # one base per sentence: its samples are base .. base + n - 1
        base = torch.as_tensor(row_id0, dtype=torch.int64).to(dev)
        if base.shape != (B,):
            raise ValueError(f"row_id0 must be an int or one int per sentence, got shape {tuple(base.shape)}")
        row_id = base[row_map.long()] + rows.long() % n
    row_id = row_id & 0xFFFFFFFF  # 32 bits of identity, as int32
    row_id = torch.where(row_id >= 2 ** 31, row_id - 2 ** 32, row_id).to(torch.int32)
    cross_len = src_len[row_map.long()].to(torch.int32).contiguous()
    score = torch.zeros(R, dtype=torch.float32, device=dev)
    fin = torch.zeros(R, dtype=torch.int32, device=dev)
    hist = [torch.full((R,), start, dtype=torch.int64, device=dev)]
    steps = []
    for t in range(max_length):
        tok = hist[-1]
        if dev.type == "cuda":
            x2 = K.embed_fwd(tok.view(R, 1).contiguous(), m.dec_emb.compute, m.pe_tgt[t:], d ** 0.5,
                             0.0, 0, None, 0).view(R, d)
        else:
            x2 = m.dec_emb.master[tok] * (d ** 0.5) + m.pe_tgt[t].view(1, d)
        klen = torch.full((R,), t + 1, dtype=torch.int32, device=dev)
        for li, layer in enumerate(m.dec_layers):
            qkv = _linear(x2, layer.qkv1).view(R, 3, H, hd)
            o = K.decode_attn(qkv[:, 0], kcache[li], vcache[li], klen, scale, k_new=qkv[:, 1],
                              v_new=qkv[:, 2])
            y = _add_ln(x2, _linear(o.reshape(R, d), layer.o1), layer.ln1)
            q2 = _linear(y, layer.q2).view(R, H, hd)
            kv5 = kv_all[:, :, li * 2 * d:(li + 1) * 2 * d].view(B, S, 2, H, hd)
            o2 = K.decode_attn(q2, kv5[:, :, 0], kv5[:, :, 1], cross_len, scale, row_map=row_map)
            y2 = _add_ln(y, _linear(o2.reshape(R, d), layer.o2), layer.ln2)
            f = _linear(_linear(y2, layer.ff1, relu=True), layer.ff2)
            x2 = _add_ln(y2, f, layer.ln3)
        lg = m.project(x2.view(R, 1, d))
        score, token, fin = K.sample_token(lg, V, score, fin, end, PAD_ID, temperature=temperature,
                                           top_k=top_k, top_p=top_p, seed=seed, step=t, row_id=row_id)
        if return_steps:
            steps.append((lg, token, fin))
        hist.append(token.long())
        if bool(fin.all()):
            break
    tokens = torch.stack(hist, dim=1).view(B, n, len(hist))
    if return_steps:
        return tokens, score.view(B, n), steps
    return tokens, score.view(B, n)
