"""One decoder step on a K/V cache: what the decoding loops hold per model.

`DecoderStep` owns, for one `Transformer` and one batch of source sentences,
the encoder output, the stacked cross-attention K / V, the self-attention K / V
caches of R rows, and the pass embed -> decoder layers -> `project` for one new
token per row. The greedy, beam-search and sampling loops (infer/greedy.py,
infer/beam.py, infer/sample.py) run it once per step; an ensemble
(infer/ensemble.py) holds one per member and runs them on the same rows. What
belongs to the hypotheses rather than to a model (the ancestry table, the row
map, the key counts, scores, history) stays with the loop and is passed in.
"""
from __future__ import annotations

from typing import Optional

import torch

from tensorflow_distributed_on_gke_amd.models.layers import LN_EPS, CrossKVFn, KVGrad, RunCtx
from tensorflow_distributed_on_gke_amd.models.transformer import Transformer
from tensorflow_distributed_on_gke_amd.ops import kernels as K
from tensorflow_distributed_on_gke_amd.ops.kernels.attention import _ref_attn_fwd


# --------------------------------------------------------------- single-token ops (GPU kernels / CPU f32)
def _linear(x2, dense, relu=False):
    if x2.is_cuda:
        return K.linear_fwd(x2.contiguous(), dense.w.compute, dense.b.master, relu=relu)
    y = x2 @ dense.w.master.t() + dense.b.master
    return torch.relu(y) if relu else y


def _add_ln(x, s, ln):
    if x.is_cuda:
        return K.ln_fwd(x.contiguous(), s.contiguous(), ln.gamma.master, ln.beta.master, 0.0, 0, None, 0,
                        save=False)[0]
    return torch.nn.functional.layer_norm(x + s, (x.shape[-1],), ln.gamma.master, ln.beta.master, LN_EPS)


def _attend(q, k, v, kv_len, scale):
    if q.is_cuda:
        return K.attn_fwd(q, k, v, kv_len, scale, False)[0]
    return _ref_attn_fwd(q, k, v, kv_len, False, scale)[0]


class DecoderStep:
    """The per-model state of a decoding loop over R rows, and its step.

    `src` int64 [B, S] (on the model's device) with lengths `src_len` is encoded
    once; the caches hold `max_length` + 1 positions of R rows. `single_query`
    chooses the attention of the step: the decoding kernel
    (ops.kernels.decode_attn: indexed keys, the K / V append fused into the
    launch), or, for the greedy loop, the training attention kernel on a cache
    the step writes first, rows and sentences then being the same."""

    def __init__(self, model: Transformer, src: torch.Tensor, src_len: torch.Tensor, R: int,
                 max_length: int, single_query: bool = True):
        m = model
        cfg = m.cfg
        self.model = m
        self.R = R
        self.single_query = single_query
        d, H = cfg.d_model, cfg.heads
        hd = d // H
        self.scale = 1.0 / (hd ** 0.5)
        rt = RunCtx(training=False, store=None)
        enc = m.encode(src, src_len, rt)
        self.S = enc.shape[1]
        self.kv_all = CrossKVFn.apply(enc, m.cross_kv.w, m.cross_kv.b, KVGrad(), rt).contiguous()
        Tm = max_length + 1
        self.kcache = [torch.zeros(R, Tm, H, hd, dtype=m.act_dtype, device=m.device) for _ in m.dec_layers]
        self.vcache = [torch.zeros(R, Tm, H, hd, dtype=m.act_dtype, device=m.device) for _ in m.dec_layers]

    def logits(self, tok: torch.Tensor, t: int, klen: torch.Tensor, cross_len: torch.Tensor,
               row_map: Optional[torch.Tensor] = None, anc: Optional[torch.Tensor] = None
               ) -> torch.Tensor:
        """The step at position t: tok int64 [R] -> logits [R, >= V] (`project`'s
        layout), the rows' K / V appended to the caches at t. klen int32 [R] is
        t + 1 per row, cross_len int32 [R] the source length of the row's
        sentence, row_map int32 [R] that sentence (None: row r is sentence r),
        anc the ancestry table (None: row r reads its own cache row)."""
        m, R = self.model, self.R
        d, H = m.cfg.d_model, m.cfg.heads
        hd = d // H
        scale = self.scale
        B, S = self.kv_all.shape[0], self.S
        if m.device.type == "cuda":
            x2 = K.embed_fwd(tok.view(R, 1).contiguous(), m.dec_emb.compute, m.pe_tgt[t:], d ** 0.5,
                             0.0, 0, None, 0).view(R, d)
        else:
            x2 = m.dec_emb.master[tok] * (d ** 0.5) + m.pe_tgt[t].view(1, d)
        for li, layer in enumerate(m.dec_layers):
            kc, vc = self.kcache[li], self.vcache[li]
            kv5 = self.kv_all[:, :, li * 2 * d:(li + 1) * 2 * d].view(B, S, 2, H, hd)
            if self.single_query:
                qkv = _linear(x2, layer.qkv1).view(R, 3, H, hd)
                o = K.decode_attn(qkv[:, 0], kc, vc, klen, scale, anc=anc, k_new=qkv[:, 1],
                                  v_new=qkv[:, 2])
            else:
                qkv = _linear(x2, layer.qkv1).view(R, 1, 3, H, hd)
                kc[:, t] = qkv[:, 0, 1]
                vc[:, t] = qkv[:, 0, 2]
                o = _attend(qkv[:, :, 0], kc[:, : t + 1], vc[:, : t + 1], klen, scale)
            y = _add_ln(x2, _linear(o.reshape(R, d), layer.o1), layer.ln1)
            if self.single_query:
                q2 = _linear(y, layer.q2).view(R, H, hd)
                o2 = K.decode_attn(q2, kv5[:, :, 0], kv5[:, :, 1], cross_len, scale, row_map=row_map)
            else:
                q2 = _linear(y, layer.q2).view(R, 1, H, hd)
                o2 = _attend(q2, kv5[:, :, 0], kv5[:, :, 1], cross_len, scale)
            y2 = _add_ln(y, _linear(o2.reshape(R, d), layer.o2), layer.ln2)
            f = _linear(_linear(y2, layer.ff1, relu=True), layer.ff2)
            x2 = _add_ln(y2, f, layer.ln3)
        return m.project(x2.view(R, 1, d))

    def gather(self, parent: torch.Tensor) -> None:
        """Row r's caches become those of row parent[r] (int64 [R]): the
        copying alternative to an ancestry table."""
        for li in range(len(self.kcache)):
            self.kcache[li] = self.kcache[li].index_select(0, parent)
            self.vcache[li] = self.vcache[li].index_select(0, parent)
