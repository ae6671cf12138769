"""Fused block-level autograd ops of the encoder-decoder Transformer.

Every post-LN sublayer of the reference is ONE `torch.autograd.Function` with a
hand-written backward that sequences the gfx950 kernels and writes parameter
gradients straight into the flat f32 gradient buffer, notifying the
data-parallel engine as each becomes final (its bucket's all-reduce can start
while backward continues):

  SelfAttnBlockFn : y = LN(x + dropout(MHA(x, x, x)))          (encoder / decoder block 1)
  CrossAttnBlockFn: y = LN(x + dropout(MHA(enc, enc, x)))      (decoder block 2)
  FFNBlockFn      : y = LN(x + dropout(W2 relu(W1 x + b1) + b2))
  CrossKVFn       : K|V projections of the encoder output for ALL decoder
                    layers as one GEMM (N = layers*2*d)
  EmbedFn         : dropout(emb[tok] * sqrt(d) + PE)

The two attention blocks are one core, _attn_block_fwd / _attn_block_bwd: the
only place that chooses between the attention kernels (forward: fused
projection + attention, bf16, e4m3; backward: fused dO, bf16, e5m2-emitting,
fp8) and that orders the block's weight-gradient, bias-fold and grad-ready
calls, on GPU and in the CPU reference. The Functions differ in where K, V and
their gradients live: slots 1 and 2 of the block's own [M, 3d] projection, or
(_ExtKV) a layer's slice of the batched cross K|V buffers and of KVGrad's; they
keep their argument lists, the checks and lazy allocations of those buffers,
and what they hand back to autograd.

Fusions this buys over per-op autograd: the residual gradient is added inside
the dgrad GEMM epilogue (beta = 1 onto the LayerNorm input gradient) instead
of an autograd add; the sublayer's output-bias gradient comes out of the
LayerNorm backward's column reduction; ReLU backward is the dgrad epilogue of
the second FFN GEMM; the encoder-output gradient of all cross attentions is
produced by one dgrad GEMM.

On CPU tensors the same ops run a plain-PyTorch f32 reference with identical
semantics (including the Philox dropout masks): the CPU test path and the
BASELINE "tiny on CPU" configuration. On GPU tensors only the HIP kernels run.

Reference semantics (distributed_training_transformer/transformer_model.py):
  MultiHeadAttention :112-166  (separate Q/K/V Dense; here fused [3d,d] / [L*2d,d])
  FFN                :169-175  (Dense(ff, relu) -> Dense(d))
  post-LN sublayer   :187-204, :219-248  (LN(x + dropout(sublayer(x))), eps 1e-6)
  embedding          :270-279, :301-308  (emb * sqrt(d) + PE, dropout)
"""
from __future__ import annotations

import math
import os
from collections import namedtuple
from dataclasses import dataclass
from typing import Optional

import torch

from tensorflow_distributed_on_gke_amd.models.params import Param, ParamStore
from tensorflow_distributed_on_gke_amd.models.wgrad import (  # noqa: F401 (WgradQueue: re-exported)
    WgradQueue, _beta, _fold_bias_later, _fp8_grad_bias, _ready, _wgrad)
from tensorflow_distributed_on_gke_amd.ops import kernels as K
from tensorflow_distributed_on_gke_amd.ops import fp8, philox
from tensorflow_distributed_on_gke_amd.ops.kernels.attention import _ref_attn_fwd, attn_align, attn_keep_scale

LN_EPS = 1e-6


@dataclass
class RunCtx:
    """Per-forward runtime state shared by all layers."""

    training: bool = False
    dropout: float = 0.1
    seed: int = 0
    ctr: Optional[torch.Tensor] = None  # int64[1]: dropout stream counter (device-resident)
    accumulate: bool = False  # accumulate into existing grads (gradient accumulation)
    store: Optional[ParamStore] = None
    # inference probe: {site: [B,H,Lq,Lk] f32 attention weights} when set
    attn_maps: Optional[dict] = None
    # ops.fp8.Fp8State: FFN and attention-input forward GEMMs in e4m3 (BASELINE config 5)
    fp8: Optional[object] = None
    # WgradQueue: weight gradients deferred to the end of backward (grouped)
    wgrad: Optional["WgradQueue"] = None
    # {embedding site: ops.kernels.EmbCsr}: the token sorts of this forward's
    # embedding backwards (one launch for both tables, Transformer.features)
    emb_csr: Optional[dict] = None
    # dropout rate on the attention probabilities (training only; bf16)
    attn_dropout: float = 0.0
    # inference probe: {cross-attention site: keyword arguments of
    # ops.kernels.attention.attn_align (q_len, k_lo, k_trim, want_soft)}; the
    # block replaces a requested site's entry by its (hard, conf, soft)
    align: Optional[dict] = None

    @property
    def p(self) -> float:
        return self.dropout if self.training else 0.0

    @property
    def attn_p(self) -> float:
        return self.attn_dropout if self.training else 0.0

    def cpu_offset(self, site: int) -> int:
        if self.ctr is None:
            return site
        return philox.rng_offset(int(self.ctr.item()), site)


@dataclass
class KVGrad:
    """Side channel collecting every decoder layer's d(K|V) into one buffer so
    the cross-K/V projection backward is a single GEMM pair. With the fp8
    attention backward on every decoder layer (`f8b`, decided by the forward
    of CrossKVFn), the layers write the e5m2 d(K|V) straight into `buf8` and
    their bias-gradient column sums into `part` ([B, layers * 2d]), and the
    bf16 K|V / d(K|V) are never materialised."""

    buf: Optional[torch.Tensor] = None
    dec_len: int = 0  # decoder sequence length of this forward (Transformer.decode)
    heads: int = 0
    f8b: bool = False
    buf8: Optional[torch.Tensor] = None
    part: Optional[torch.Tensor] = None
    wkv: Optional["Param"] = None  # the batched K|V projection (its e5m2 gradient slot)


def _dgrad_res(dy2: torch.Tensor, w: Param, N: int, dres: Optional[torch.Tensor]) -> torch.Tensor:
    """A block's input gradient dx = dy2 @ w (+ dres, the residual gradient
    already in dx: accumulated by the GEMM's beta = 1 epilogue)."""
    if dres is None:
        return K.linear_dgrad(dy2, w.compute, N)
    return _dgrad_into(dy2, w, N, dres)


def _keep_scale(rt: RunCtx, site: int, shape, device) -> Optional[torch.Tensor]:
    """CPU reference dropout multiplier (keep/(1-p)) drawn from the device RNG stream."""
    p = rt.p
    if p <= 0:
        return None
    n = math.prod(shape)
    keep = philox.keep_mask(rt.seed, rt.cpu_offset(site), n, p).view(shape)
    return keep.to(torch.float32).to(device) / (1.0 - p)


def _write_grad(p: Param, g: torch.Tensor, rt: RunCtx) -> None:
    if rt.accumulate:
        p.grad.add_(g.to(p.grad.dtype))
    else:
        p.grad.copy_(g.to(p.grad.dtype))


def _attn_lean(rt: RunCtx, M: int, w_in: Param, w_out: Optional[Param], d: int) -> bool:
    """Attention block with fp8 projections in forward and backward (fp8
    state with ATTN_PROJ_FP8; weight gradients through the deferred queue)."""
    st = rt.fp8
    return (st is not None and rt.training and rt.wgrad is not None and fp8.ATTN_PROJ_FP8
            and id(w_in) in st.proj_bwd and (w_out is None or id(w_out) in st.attn_out)
            and fp8.wgrad_fp8_ok(M, d, d))


def _fp8_dgrad(g8, g_slot: int, w: Param, out, rt: RunCtx, beta: float = 0.0, out8_slot=None):
    """out (=|+= beta) dequant(g8 (e5m2) @ w) against w's e4m3 copy (read
    N-contiguous by the kernel, fp8.DGRAD_PLAIN_W; else its transposed copy).
    out None, out8_slot: returns its e5m2 copy only (no bf16 output) in that
    gradient slot (amax recorded): the fp8 attention backward's dO."""
    st = rt.fp8
    wt8, swt = st.weights.get(w, transposed=not fp8.DGRAD_PLAIN_W)
    return fp8.gemm_bf8_dgrad(g8, st.gmeta, g_slot, wt8, st.meta, swt, out, beta=beta,
                              out8_slot=out8_slot, w_plain=fp8.DGRAD_PLAIN_W)


def _f8_bwd_planned(rt: RunCtx, lean: bool, Lq: int, Lk: int, hd: int) -> bool:
    """Forward-time decision: will this (e4m3-forward) attention block's
    backward run on the fp8 kernel? Then the bf16 copies of its projection
    outputs are never read and not written. (Not with attention maps: they
    read the bf16 Q / K; nor with an alignment request.)"""
    return (lean and fp8.ATTN_BWD_F8 and rt.attn_maps is None and rt.align is None
            and K.attn_bwd_f8_ok(Lq, Lk, hd))


# =============================================================================== LN helpers
def _proj_ln_fwd(a2, w: Param, b: Param, x, gamma: Param, beta: Param, site: int, rt: RunCtx):
    """GPU block tail y = LN(x + dropout(a2 @ w^T + b)) -> (y, saved): the
    output-projection GEMM (bias fused) then the fused dropout + residual +
    LayerNorm kernel. (GEMM + LayerNorm in one launch measured slower on
    MI355X, both as full-row tiles -- every workgroup streams all of W --
    and as 128-column tiles exchanging row partials across workgroups; that
    path is gone from the tree, its numbers are in
    profiles/r5/ln_fused_ab.txt.)"""
    s = K.linear_fwd(a2, w.compute, b.master)
    return _ln_fwd(x, s.view(x.shape), gamma, beta, site, rt)


# the training forward's LayerNorms save their dropout keep bits (1 bit per
# element) for the backward, which reads them instead of regenerating the
# Philox mask (ln_bwd kbits)
LN_KEEP_BITS = os.environ.get("TDG_LN_KEEP_BITS", "1") != "0"


def _kbits(rt: RunCtx, x: torch.Tensor) -> Optional[torch.Tensor]:
    """Keep-bit bitmap [M, D / 8] of a training LayerNorm with dropout."""
    D = x.shape[-1]
    if LN_KEEP_BITS and x.is_cuda and rt.training and rt.p > 0 and D % 512 == 0:
        return torch.empty(x.numel() // D, D // 8, dtype=torch.uint8, device=x.device)
    return None


def _ln_fwd(x, s, gamma: Param, beta: Param, site: int, rt: RunCtx):
    """Returns (y, saved) for y = LN(x + dropout(s)); saved = (h, mean, rstd,
    CPU keep scale, GPU keep bits)."""
    if x.is_cuda:
        y8 = s8 = a8 = None
        slot = rt.fp8.ln_slots.get(id(gamma)) if rt.fp8 is not None else None
        if slot is not None:  # this LN feeds an fp8 GEMM: emit its e4m3 copy too
            y8 = torch.empty(x.shape, dtype=fp8.FP8, device=x.device)
            s8, a8 = rt.fp8.meta.s(slot), rt.fp8.meta.a(slot)
            rt.fp8.stash[slot] = y8
        kbits = _kbits(rt, x)
        y, h, mean, rstd = K.ln_fwd(x.contiguous(), s.contiguous(), gamma.master, beta.master,
                                    rt.p, rt.seed, rt.ctr, site, y8=y8, s8=s8, amax8=a8, kbits=kbits)
        return y, (h, mean, rstd, None, kbits)
    ks = _keep_scale(rt, site, s.shape, s.device)
    h = x + (s * ks if ks is not None else s)
    mean = h.mean(-1, keepdim=True)
    rstd = torch.rsqrt(((h - mean) ** 2).mean(-1, keepdim=True) + LN_EPS)
    return (h - mean) * rstd * gamma.master + beta.master, (h, mean, rstd, ks, None)


def _ln_bwd(dy, saved, gamma: Param, beta: Param, sub_bias: Param, site: int, rt: RunCtx,
            ds8_slot: Optional[int] = None):
    """Returns (dh, ds): dh = dL/d(residual input) (fresh, writable), ds =
    dL/d(sublayer output). Also writes dgamma, dbeta and the sublayer's output
    bias gradient (sum of ds over rows). ds8_slot (GPU, fp8 backward): ds is
    returned as its e5m2 copy only (scale slot ds8_slot of rt.fp8.gmeta,
    amax recorded), the bf16 ds is not written."""
    h, mean, rstd, ks = saved[:4]
    if dy.is_cuda:
        q = rt.wgrad
        ds8 = s8 = a8 = None
        if ds8_slot is not None:
            gm = rt.fp8.gmeta
            ds8 = torch.empty(dy.shape, dtype=gm.dtype, device=dy.device)
            s8, a8 = gm.s(ds8_slot), gm.a(ds8_slot)
        folds = [] if q is not None else None
        dh, ds = K.ln_bwd(dy.contiguous(), h, mean, rstd, gamma.master, gamma.grad, beta.grad,
                          sub_bias.grad, rt.p, rt.seed, rt.ctr, site, want_ds=ds8 is None,
                          accumulate=rt.accumulate, defer=folds,
                          ds8=ds8, s8=s8, amax8=a8, kbits=saved[4])
        if ds8 is not None:
            ds = ds8
        if q is not None:  # folded (and reported ready) with the next wgrad flush
            q.defer_fold(folds, (gamma, beta, sub_bias), rt)
            return dh, ds
    else:
        xhat = (h - mean) * rstd
        D = h.shape[-1]
        g = dy * gamma.master
        dh = rstd * (g - g.mean(-1, keepdim=True) - xhat * (g * xhat).mean(-1, keepdim=True))
        ds = dh * ks if ks is not None else dh
        _write_grad(gamma, (dy * xhat).reshape(-1, D).sum(0), rt)
        _write_grad(beta, dy.reshape(-1, D).sum(0), rt)
        _write_grad(sub_bias, ds.reshape(-1, D).sum(0), rt)
    _ready(rt, gamma, beta, sub_bias)
    return dh, ds


def _dgrad_into(dy2: torch.Tensor, w: Param, N: int, dx: torch.Tensor) -> torch.Tensor:
    """dx += dy2 @ w (the residual gradient already sits in dx)."""
    if dy2.is_cuda:
        return K.linear_dgrad(dy2, w.compute, N, out=dx.view(dy2.shape[0], -1), beta=1.0)
    dx.view(dy2.shape[0], -1).add_(dy2 @ w.master)
    return dx


# =============================================================================== embedding
class EmbedFn(torch.autograd.Function):
    NO_GRAD_ARGS = 6  # forward arguments that get no gradient from backward: all of them
    @staticmethod
    def forward(ctx, anchor, tok, table: Param, pe: torch.Tensor, site: int, rt: RunCtx):
        d = table.shape[1]
        scale = math.sqrt(d)
        ctx.table, ctx.site, ctx.rt, ctx.scale = table, site, rt, scale
        ctx.save_for_backward(tok)
        if tok.is_cuda:
            # training with dropout: the keep bits for the CSR backward
            ctx.kbits = None
            ctx.csr = rt.emb_csr.get(site) if rt.emb_csr else None
            if ctx.csr is not None and rt.p > 0 and d % 512 == 0:
                ctx.kbits = torch.empty(tok.numel(), d // 8, dtype=torch.uint8, device=tok.device)
            return K.embed_fwd(tok, table.compute, pe, scale, rt.p, rt.seed, rt.ctr, site,
                               kbits=ctx.kbits)
        B, L = tok.shape
        x = table.master[tok] * scale + pe[:L].unsqueeze(0)
        ks = _keep_scale(rt, site, x.shape, x.device)
        ctx.ks = ks
        return x * ks if ks is not None else x

    @staticmethod
    def backward(ctx, dout):
        (tok,) = ctx.saved_tensors
        table, rt = ctx.table, ctx.rt
        if dout.is_cuda:
            dc = dout.contiguous()
            K.embed_bwd(tok, dc, table.grad, ctx.scale, rt.p, rt.seed, rt.ctr, ctx.site,
                        accumulate=rt.accumulate, kbits=ctx.kbits, csr=ctx.csr)
        else:
            g = dout * ctx.ks if ctx.ks is not None else dout
            g = (g * ctx.scale).reshape(-1, table.shape[1])
            table.grad.index_add_(0, tok.reshape(-1), g.to(table.grad.dtype))
        _ready(rt, table)
        return (None,) * EmbedFn.NO_GRAD_ARGS


# =============================================================================== attention (CPU reference core)
# (the forward, _ref_attn_fwd, lives next to the kernel it stands in for: ops/kernels/attention.py)
def _ref_attn_bwd(q, k, v, p, dout, scale, keep_scale=None):
    """keep_scale: the forward's attention-dropout multiplier (p stays the
    undropped softmax): dV from p * keep_scale, dP masked and scaled alike."""
    ks = 1.0 if keep_scale is None else keep_scale.to(p.dtype)
    dv = torch.einsum("bhqk,bqhd->bkhd", p * ks, dout)
    dp = torch.einsum("bqhd,bkhd->bhqk", dout, v) * ks
    ds = p * (dp - (dp * p).sum(-1, keepdim=True))
    dq = torch.einsum("bhqk,bkhd->bqhd", ds, k) * scale
    dk = torch.einsum("bhqk,bqhd->bkhd", ds, q) * scale
    return dq, dk, dv


def attention_probs(q, k, kv_len, causal: bool, scale: float) -> torch.Tensor:
    """Attention weights [B,H,Lq,Lk] (f32), the maps the reference returns."""
    if q.is_cuda:
        return K.attn_probs(q, k, kv_len, scale, causal)
    return _ref_attn_fwd(q, k, k, kv_len, causal, scale)[1]


def _attn_out_ln_fwd(ctx, o, x, wo: Param, bo: Param, gamma: Param, beta: Param, site: int,
                     rt: RunCtx, kx, o8e):
    """An attention block's forward ending y = LN(x + dropout(o @ Wo^T + bo)); sets ctx.ln and
    ctx.f8a. kx, o8e: the lean block's kept e4m3 input and the e4m3 O its attention epilogue
    emitted."""
    M, d = x.numel() // x.shape[-1], x.shape[-1]
    ctx.f8a = None
    if ctx.lean:  # e4m3 output projection; keep the e4m3 operands for the backward
        s, o8 = rt.fp8.out_proj(o.view(M, d), wo, bo, o8e[0] if o8e else None)
        ctx.f8a = (kx[0], kx[1], o8)
    elif x.is_cuda:  # projection fused with the LayerNorm
        y, ctx.ln = _proj_ln_fwd(o.view(M, d), wo, bo, x, gamma, beta, site, rt)
        return y
    else:
        s = o.reshape(M, d) @ wo.master.t() + bo.master
    y, ctx.ln = _ln_fwd(x, s.view(x.shape), gamma, beta, site, rt)
    return y


_LeanBwd = namedtuple("_LeanBwd", "dh ds8 go os_ gq x8 xs o8")


def _lean_bwd_begin(ctx, dy, w_in: Param, site: int, rt: RunCtx) -> _LeanBwd:
    """Start of a lean fp8 attention backward (ctx.p = (w_in, b_in, wo, bo, gamma, beta)): the
    LayerNorm backward -> dh and ds [M, d] as e5m2 only (gradient slot go); gq: w_in's gradient
    slot; x8 (slot xs), o8 (slot os_): the forward's e4m3 block input and attention output."""
    wo, bo, gamma, beta = ctx.p[2:]
    st = rt.fp8
    x8, xs, o8 = ctx.f8a
    os_, go = st.attn_out[id(wo)]
    dh, ds8 = _ln_bwd(dy, ctx.ln, gamma, beta, bo, site, rt, ds8_slot=go)
    return _LeanBwd(dh, ds8.view(-1, dy.shape[-1]), go, os_, st.proj_bwd[id(w_in)], x8, xs, o8)


def _lean_bwd_end(lb: _LeanBwd, g8, w_in: Param, wo: Param, rt: RunCtx) -> None:
    """input-projection dgrad of e5m2 g8 into the residual gradient, both weight gradients in fp8"""
    st, bt = rt.fp8, _beta(rt)
    _fp8_dgrad(g8, lb.gq, w_in, lb.dh.view(lb.ds8.shape), rt, 1.0)
    rt.wgrad.add_fp8(lb.ds8, st.gmeta.s(lb.go), lb.o8, st.meta.s(lb.os_), wo, bt, rt)
    rt.wgrad.add_fp8(g8, st.gmeta.s(lb.gq), lb.x8, st.meta.s(lb.xs), w_in, bt, rt)


# =============================================================================== attention block core
# Cross-attention's K and V lie outside the block, in buffers batched over the decoder layers.
# Each of kv, kv8, g, g8 is this layer's (K, V) pair of [B, S, H, hd] views (_layer_kv), or
# (None, None): kv the bf16 K|V, kv8 the e4m3 K|V (scale slot kvs); for the backward g the bf16
# d(K|V), or g8 the e5m2 d(K|V) in their own gradient slot gk, with their bias-gradient column
# sums in part ([B, layers * 2d]) at columns cs_k / cs_v.
_ExtKV = namedtuple("_ExtKV", "kv kv8 kvs g g8 gk part cs_k cs_v",
                    defaults=((None, None), (None, None), None, None, 0, 0))

# an attention block's dropout on its probabilities draws from a site of its own: this plus the
# block's LayerNorm site (Transformer's sites stay below 64; rng_offset has 4096 per counter step)
ATTN_DROP_SITE = 2048


def _layer_kv(t, layer: int, d: int, heads: int):
    """Decoder layer `layer`'s (K, V) [B, S, H, hd] views of a batched [B, S, layers * 2d]
    tensor (the cross K|V or their gradient); (None, None) without one."""
    if t is None:
        return None, None
    B, S = t.shape[:2]
    return t[:, :, layer * 2 * d:(layer + 1) * 2 * d].view(B, S, 2, heads, d // heads).unbind(2)


def _qkv(t, kv, B: int, heads: int, hd: int):
    """(q, k, v) [B, L, H, hd] views of an input-projection output, or of its gradient, t: the
    three column slots of t [M, 3d] (self-attention: kv None), or t [M, d] as q and the pair kv
    from outside the block (cross-attention). t None: None in its places."""
    if kv is None:
        return t.view(B, -1, 3, heads, hd).unbind(2) if t is not None else (None, None, None)
    return (t.view(B, -1, heads, hd) if t is not None else None,) + tuple(kv)


def _attn_block_fwd(ctx, x, w_in: Param, b_in: Param, wo: Param, bo: Param, gamma: Param,
                    beta: Param, heads: int, kv_len, causal: bool, site: int, rt: RunCtx,
                    ext: Optional[_ExtKV] = None):
    """Forward of an attention block y = LN(x + dropout(MHA(..) @ Wo^T + bo)), the one place that
    chooses between the attention forward kernels. Q|K|V = x @ w_in^T + b_in are the column slots
    of one [M, 3d] projection (self-attention); with `ext` (cross-attention) the projection is Q
    alone and K, V come from outside. Sets ctx.p, meta, lean, f8b (the fp8 backward is planned),
    q8 (the e4m3 projection output and its scale slot, where the e4m3 attention read it) and
    what _attn_out_ln_fwd sets. Returns (y, x2, proj, o, aux); proj None: only its e4m3 copy
    was written."""
    B, L, d = x.shape
    hd = d // heads
    scale = 1.0 / math.sqrt(hd)
    ctx.p = (w_in, b_in, wo, bo, gamma, beta)
    ctx.meta = (heads, causal, scale, site, rt)
    x2 = x.reshape(B * L, d)
    ctx.lean = lean = x.is_cuda and _attn_lean(rt, B * L, w_in, wo, d)
    kx = [] if lean else None
    ctx.q8 = o8e = None
    kv, kv8 = (ext.kv, ext.kv8) if ext is not None else (None, None)
    # attention dropout (training, bf16): the register-staged attention kernels' DROP variants,
    # so no fused projection + attention; the backward regenerates the mask from ctx.drop
    ctx.drop = drop = ((rt.attn_p, rt.seed, rt.ctr, ATTN_DROP_SITE + site) if rt.attn_p > 0 else None)
    ctx.attn_ks = None
    if drop is not None and rt.fp8 is not None:
        raise RuntimeError("attention dropout with fp8 is not supported: the fp8 attention kernels "
                           "have no dropout variant")
    if x.is_cuda:
        Lk = L if ext is None else (kv8 if kv[0] is None else kv)[0].shape[1]
        f8 = (rt.fp8 is not None and (ext is None or kv8[0] is not None)
              and K.attn_fwd_fp8_ok(L, Lk, hd))
        # the fp8 backward reads only the e4m3 Q|K|V: no bf16 copy then
        ctx.f8b = f8b = f8 and _f8_bwd_planned(rt, lean, L, Lk, hd)
        if ext is not None and kv[0] is None and not f8b:
            raise RuntimeError("cross-attention: the batched K|V were produced for the fp8 "
                               "backward (no bf16 copy) but this layer does not run it")
        r = (rt.fp8.linear(x2, w_in, b_in, want8=f8, keep_x8=kx, want_y=not f8b)
             if rt.fp8 is not None else None)
        proj, proj8 = (r[0], r[1]) if f8 and r is not None else (r, None)
        fused = None
        if (proj is None and not f8b and rt.fp8 is None and rt.attn_maps is None and drop is None
                and not (rt.align and site in rt.align)):
            # projection + attention forward in one launch (<= 128 tokens)
            fused = K.qkv_attn_fwd(x2, w_in.compute, b_in.master, B, heads, kv_len, scale, causal,
                                   *(kv or ()))
            if fused is not None:
                proj = fused[0]
        if proj is None and not f8b:
            proj = K.linear_fwd(x2, w_in.compute, b_in.master)  # [M, 3d] / [M, d]
        q, k, v = _qkv(proj, kv, B, heads, hd)
        if fused is not None:
            o, aux = fused[1], fused[2]
        elif proj8 is not None:  # e4m3 attention on the projection's e4m3 output (and, for
            # cross-attention, the batched e4m3 K|V)
            sq = rt.fp8.meta.s(r[2])
            skv = sq if ext is None else rt.fp8.meta.s(ext.kvs)
            ctx.q8 = (proj8, r[2])  # (the fp8 attention backward's operands)
            # (lean: the epilogue also emits the e4m3 O of the output projection)
            o8e = rt.fp8.o8_for(wo, (B, L, heads, hd), x.device) if lean else None
            o, aux = K.attn_fwd_fp8(*_qkv(proj8, kv8, B, heads, hd), sq, skv, skv, kv_len, scale,
                                    causal, *(o8e or ()))
        else:
            o, aux = K.attn_fwd(q, k, v, kv_len, scale, causal, drop=drop)
    else:
        proj = x2 @ w_in.master.t() + b_in.master
        q, k, v = _qkv(proj, kv, B, heads, hd)
        if drop is not None:  # (CPU reference: the same mask, kept for the backward)
            ctx.attn_ks = attn_keep_scale(drop[0], rt.seed, rt.cpu_offset(drop[3]), B, heads, L,
                                          k.shape[1])
        o, aux = _ref_attn_fwd(q, k, v, kv_len, causal, scale, ctx.attn_ks)
    if rt.attn_maps is not None:  # (_f8_bwd_planned: the bf16 q, k exist when maps are asked for)
        rt.attn_maps[site] = attention_probs(q, k, kv_len, causal, scale)
    if rt.align and site in rt.align:  # (as the maps: off the fused launch, bf16 q and k exist)
        klen = kv_len if kv_len is not None else torch.full((B,), k.shape[1], dtype=torch.int32,
                                                            device=x.device)
        rt.align[site] = attn_align(q, k, klen, scale, **rt.align[site])
    y = _attn_out_ln_fwd(ctx, o, x, wo, bo, gamma, beta, site, rt, kx, o8e)
    return y, x2, proj, o, aux


def _attn_block_bwd(ctx, dy, x2, proj, o, aux, kv_len, ext: Optional[_ExtKV] = None):
    """Backward of _attn_block_fwd -> dx [B, L, d], the one place that chooses between the
    attention backward kernels. Writes the block's parameter gradients and, with `ext`, this
    layer's d(K|V) into ext.g / ext.g8. Lean fp8 blocks: e5m2 ds from the LayerNorm backward ->
    O-proj dgrad (e5m2 x e4m3 Wo^T) -> attention backward -> e5m2 dQ|dK|dV -> input-projection
    dgrad (into the residual gradient); both weight gradients in fp8 from the saved e4m3
    operands."""
    w_in, b_in, wo, bo, gamma, beta = ctx.p
    heads, causal, scale, site, rt = ctx.meta
    B, L, d = dy.shape
    M, hd, N = B * L, d // heads, w_in.shape[0]
    kv, kv8, gkv, gkv8 = (ext.kv, ext.kv8, ext.g, ext.g8) if ext is not None else (None,) * 4
    cs_k, cs_v = (ext.cs_k, ext.cs_v) if ext is not None else (d, 2 * d)
    tag = f"{'qkv' if ext is None else 'q'}{site}"  # (workspaces: one per site and purpose)
    q, k, v = _qkv(proj, kv, B, heads, hd)
    if ctx.lean:
        st = rt.fp8
        lb = _lean_bwd_begin(ctx, dy, w_in, site, rt)
        sg, ag = st.gmeta.s(lb.gq), st.gmeta.a(lb.gq)
        if ctx.f8b and ctx.q8 is not None:  # (planned by the forward, which kept the e4m3 operands)
            # fp8 attention backward: e5m2 dO straight from the output projection's dgrad, e4m3
            # Q/K/V of the forward -> e5m2 dQ|dK|dV (+ amax, bias sums). Cross-attention: dK / dV
            # as e5m2 straight into the batched buffer (the cross K|V projection's gradient
            # slot, bias sums into its own part), or bf16 into the batched cross K|V gradient
            gdo, gds = st.attn_bwd8[id(wo)]
            do8 = _fp8_dgrad(lb.ds8, lb.go, wo, None, rt, out8_slot=gdo)
            proj8, qs = ctx.q8
            sq = st.meta.s(qs)
            skv = sq if ext is None else st.meta.s(ext.kvs)
            g8 = torch.empty(M, N, dtype=st.gmeta.dtype, device=dy.device)
            dq8, dk8, dv8 = _qkv(g8, gkv8, B, heads, hd)
            dk, dv = gkv or (None, None)
            part = K.workspace(f"f8cs_{tag}", B * N, dy.device)
            own = {}
            if ext is not None and ext.part is not None:
                own = dict(sgkv8=st.gmeta.s(ext.gk), amaxgkv8=st.gmeta.a(ext.gk),
                           cs_part2=ext.part, cs_ld2=ext.part.shape[1])
            nparts = K.attn_bwd_f8(*_qkv(proj8, kv8, B, heads, hd), sq, skv, skv, o,
                                   do8.view(B, L, heads, hd), st.gmeta.s(gdo), aux, kv_len, scale,
                                   causal, st.gmeta.s(gds), st.gmeta.a(gds), dk=dk, dv=dv, dq8=dq8,
                                   dk8=dk8, dv8=dv8, sg8=sg, amaxg8=ag, cs_part=part, cs_ld=N,
                                   cs_q=0, cs_k=cs_k, cs_v=cs_v, **own)
            _fold_bias_later(rt, part[: nparts * N], nparts, N, b_in)
        else:
            do = torch.empty(M, d, dtype=torch.bfloat16, device=dy.device)
            _fp8_dgrad(lb.ds8, lb.go, wo, do, rt, 0.0)
            g = torch.empty(M, N, dtype=torch.bfloat16, device=dy.device)
            dq, dk, dv = _qkv(g, gkv, B, heads, hd)
            if fp8.ATTN_BWD_G8 and K.attn_bwd_g8_ok(L, k.shape[1], hd):
                # the attention backward emits e5m2 dQ|dK|dV, their amax and the bias-gradient
                # partials itself (no bf16 dQ|dK|dV pass). Cross-attention: of dQ alone; dK / dV
                # stay bf16 (summed over the layers into the batched cross K|V gradient), so
                # the bf16 writes are not skipped
                g8 = torch.empty(M, N, dtype=st.gmeta.dtype, device=dy.device)
                dq8, dk8, dv8 = _qkv(g8, gkv8, B, heads, hd)
                part = K.workspace(f"qcs_{tag}", B * -(-L // 128) * N, dy.device)
                nparts = K.attn_bwd_g8(q, k, v, o, do.view(B, L, heads, hd), aux, dq, dk, dv,
                                       kv_len, scale, causal, dq8, dk8, dv8, sg, ag, part, N, 0,
                                       cs_k, cs_v, skip_bf16=ext is None)
                _fold_bias_later(rt, part[: nparts * N], nparts, N, b_in)
            else:
                K.attn_bwd(q, k, v, o, do.view(B, L, heads, hd), aux, dq, dk, dv, kv_len, scale,
                           causal)
                g8 = _fp8_grad_bias(g, lb.gq, b_in, rt, tag)
        _lean_bwd_end(lb, g8, w_in, wo, rt)
        return lb.dh.view(B, L, d)
    dh, ds = _ln_bwd(dy, ctx.ln, gamma, beta, bo, site, rt)
    ds2 = ds.reshape(M, d)
    if dy.is_cuda:
        _wgrad(rt, ds2, o.view(M, d), d, wo)
        g = torch.empty(M, N, dtype=torch.bfloat16, device=dy.device)
        dq, dk, dv = _qkv(g, gkv, B, heads, hd)
        # (<= 128 tokens: the output projection's dgrad dO = ds @ Wo inside the attention
        # backward)
        if not K.attn_bwd_fdo(q, k, v, o, ds2, wo.compute, aux, dq, dk, dv, kv_len, scale, causal,
                              drop=ctx.drop):
            do = K.linear_dgrad(ds2, wo.compute, d)
            K.attn_bwd(q, k, v, o, do.view(B, L, heads, hd), aux, dq, dk, dv, kv_len, scale, causal,
                       drop=ctx.drop)
        _wgrad(rt, g, x2, N, w_in, b_in)
    else:
        _write_grad(wo, ds2.t() @ o.reshape(M, d), rt)
        _ready(rt, wo)
        do = (ds2 @ wo.master).view(B, L, heads, hd)
        g = torch.empty(M, N, dtype=ds2.dtype)
        for dst, src in zip(_qkv(g, gkv, B, heads, hd),
                            _ref_attn_bwd(q, k, v, aux, do, scale, ctx.attn_ks)):
            dst.copy_(src)
        _write_grad(w_in, g.t() @ x2, rt)
        _write_grad(b_in, g.sum(0), rt)
        _ready(rt, w_in, b_in)  # (GPU: reported by _wgrad / the deferred flush)
    return _dgrad_into(g, w_in, N, dh).view(B, L, d)


# =============================================================================== self-attention block
class SelfAttnBlockFn(torch.autograd.Function):
    NO_GRAD_ARGS = 11  # forward arguments after x
    @staticmethod
    def forward(ctx, x, wqkv: Param, bqkv: Param, wo: Param, bo: Param, gamma: Param,
                beta: Param, heads: int, kv_len, causal: bool, site: int, rt: RunCtx):
        y, x2, qkv, o, aux = _attn_block_fwd(ctx, x, wqkv, bqkv, wo, bo, gamma, beta, heads, kv_len,
                                             causal, site, rt)
        ctx.save_for_backward(x2, qkv, o, aux, kv_len)
        return y

    @staticmethod
    def backward(ctx, dy):
        dx = _attn_block_bwd(ctx, dy, *ctx.saved_tensors)
        rt = ctx.meta[-1]
        if dy.is_cuda and rt.wgrad is not None:
            rt.wgrad.layer_end()  # self-attention is a layer's first block
        return (dx,) + (None,) * SelfAttnBlockFn.NO_GRAD_ARGS


# =============================================================================== cross-attention
def _take_dkv(dkv_in, kvh: KVGrad, rows: int) -> torch.Tensor:
    """The batched d(K|V) [rows, layers * 2d] the decoder layers filled (layer
    0 also hands it to autograd, which delivers it as dkv_in)."""
    dkv = (dkv_in if dkv_in is not None else kvh.buf).reshape(rows, -1)
    kvh.buf = None
    return dkv


class CrossKVFn(torch.autograd.Function):
    """kv_all[B, S, layers*2*d] = enc @ Wkv_all^T + b: the K and V projections
    of the encoder output for every decoder layer in one GEMM."""

    NO_GRAD_ARGS = 4  # forward arguments after enc
    @staticmethod
    def forward(ctx, enc, wkv: Param, bkv: Param, kvh: KVGrad, rt: RunCtx):
        B, S, d = enc.shape
        e2 = enc.reshape(B * S, d)
        ctx.p = (wkv, bkv)
        ctx.kvh, ctx.rt, ctx.shape = kvh, rt, (B, S, d)
        ctx.save_for_backward(e2)
        ctx.lean = lean = enc.is_cuda and _attn_lean(rt, B * S, wkv, None, d)
        kx = [] if lean else None
        ctx.f8a = None
        T = kvh.dec_len
        hd = d // kvh.heads if kvh.heads else 0
        # every decoder layer's cross-attention runs e4m3 forward + fp8
        # backward: the bf16 K|V are never read (and d(K|V) come as e5m2)
        kvh.f8b = bool(lean and enc.is_cuda and T and K.attn_fwd_fp8_ok(T, S, hd)
                       and fp8.wgrad_fp8_ok(B * T, d, d) and _f8_bwd_planned(rt, True, T, S, hd))
        if enc.is_cuda:
            kv = None
            if rt.fp8 is not None:
                r = rt.fp8.linear(e2.contiguous(), wkv, bkv, want8=True, keep_x8=kx, want_y=not kvh.f8b)
                if lean and r is not None:
                    ctx.f8a = tuple(kx)
                if r is not None:  # its e4m3 copy feeds the decoders' e4m3 attention
                    kv = r[0]
                    rt.fp8.kv8 = (r[1].view(B, S, -1), r[2])
                    if kvh.f8b:  # (autograd needs an output of this shape; nothing reads
                        # it: a zero-stride placeholder, not a bf16 K|V image)
                        kv = torch.zeros(1, dtype=torch.bfloat16, device=enc.device).expand(
                            B * S, r[1].shape[1])
            if kv is None:
                kv = K.linear_fwd(e2.contiguous(), wkv.compute, bkv.master)
        else:
            kv = e2 @ wkv.master.t() + bkv.master
        return kv.view(B, S, -1)

    @staticmethod
    def backward(ctx, dkv_in):
        wkv, bkv = ctx.p
        rt = ctx.rt
        B, S, d = ctx.shape
        (e2,) = ctx.saved_tensors
        # filled slice-by-slice by every CrossAttnBlockFn.backward (layer 0
        # also hands it to autograd, which delivers it here as dkv_in)
        kvh = ctx.kvh
        N = wkv.shape[0]
        bt = _beta(rt)
        if e2.is_cuda and ctx.f8a is not None:
            # lean fp8: e5m2 dK|dV of every decoder layer -> one dgrad + fp8
            # weight gradient against the encoder output's e4m3 copy
            st = rt.fp8
            x8, xs = ctx.f8a
            gk = st.proj_bwd[id(wkv)]
            if kvh.f8b:  # written by the layers' fp8 attention backward (e5m2 + bias sums;
                # dkv_in is the layers' zero-stride placeholder)
                dkv8 = kvh.buf8.reshape(B * S, -1)
                _fold_bias_later(rt, kvh.part, B, N, bkv)
                kvh.buf8 = kvh.part = None
            else:
                dkv8 = _fp8_grad_bias(_take_dkv(dkv_in, kvh, B * S).contiguous(), gk, bkv, rt, "kv")
            rt.wgrad.add_fp8(dkv8, st.gmeta.s(gk), x8, st.meta.s(xs), wkv, bt, rt)
            rt.wgrad.boundary()
            denc = torch.empty(B * S, d, dtype=torch.bfloat16, device=e2.device)
            _fp8_dgrad(dkv8, gk, wkv, denc, rt, 0.0)
            if rt.store is not None:
                rt.store.release_point()
            return (denc.view(B, S, d),) + (None,) * CrossKVFn.NO_GRAD_ARGS
        dkv = _take_dkv(dkv_in, kvh, B * S)
        if e2.is_cuda:
            _wgrad(rt, dkv, e2, N, wkv, bkv)
            if rt.wgrad is not None:
                rt.wgrad.boundary()  # every decoder layer's backward is done
            denc = _dgrad_res(dkv, wkv, N, None)
        else:
            _write_grad(wkv, dkv.t() @ e2, rt)
            _write_grad(bkv, dkv.sum(0), rt)
            _ready(rt, wkv, bkv)
            denc = dkv @ wkv.master
        if rt.store is not None:
            # the rest of backward (encoder) reads no decoder-side weight: the
            # data-parallel optimizer may update those buckets from here on
            rt.store.release_point()
        return (denc.view(B, S, d),) + (None,) * CrossKVFn.NO_GRAD_ARGS


class CrossAttnBlockFn(torch.autograd.Function):
    """Decoder block 2: Q from the decoder stream, K = V = encoder output
    (reference call order mha2(enc, enc, out1) -> values, keys, query)."""

    NO_GRAD_ARGS = 12  # forward arguments after x and kv_all
    @staticmethod
    def forward(ctx, x, kv_all, layer: int, kvh: KVGrad, wq: Param, bq: Param, wo: Param,
                bo: Param, gamma: Param, beta: Param, heads: int, kv_len, site: int, rt: RunCtx):
        d = x.shape[-1]
        # (kvh.f8b: kv_all is a placeholder, the e4m3 K|V are read)
        if not kvh.f8b and not kv_all.is_contiguous():
            raise ValueError("kv_all must be contiguous")
        kv8, kvs = (None, None), None
        if x.is_cuda and rt.fp8 is not None and rt.fp8.kv8 is not None:
            t8, kvs = rt.fp8.kv8  # the batched e4m3 K|V
            if t8.shape != kv_all.shape:
                raise RuntimeError(f"fp8 cross K|V {tuple(t8.shape)} is not this forward's "
                                   f"{tuple(kv_all.shape)}")
            kv8 = _layer_kv(t8, layer, d, heads)
        ext = _ExtKV(_layer_kv(None if kvh.f8b else kv_all, layer, d, heads), kv8, kvs)
        y, x2, q, o, aux = _attn_block_fwd(ctx, x, wq, bq, wo, bo, gamma, beta, heads, kv_len, False,
                                           site, rt, ext)
        ctx.layer, ctx.kvh = layer, kvh
        # (kept for the fp8 attention backward, with ctx.q8, only where the e4m3 attention ran)
        ctx.kv8 = (kv8, kvs) if ctx.q8 is not None else ((None, None), None)
        ctx.save_for_backward(x2, kv_all, q, o, aux, kv_len)
        return y

    @staticmethod
    def backward(ctx, dy):
        heads, rt = ctx.meta[0], ctx.meta[-1]
        layer, kvh = ctx.layer, ctx.kvh
        x2, kv_all, q, o, aux, kv_len = ctx.saved_tensors
        B, S, NKV = kv_all.shape
        d = dy.shape[-1]
        kv = dkv_all = gk = None
        cs_k = cs_v = 0
        if kvh.f8b:
            # every layer's d(K|V) goes to kvh.buf8 as e5m2 (the cross K|V projection's
            # gradient slot), their bias sums to kvh.part: no bf16 buffer
            if kvh.buf8 is None:
                kvh.buf8 = torch.empty(B, S, NKV, dtype=rt.fp8.gmeta.dtype, device=dy.device)
                kvh.part = torch.empty(B, NKV, dtype=torch.float32, device=dy.device)
            gk = rt.fp8.proj_bwd[id(kvh.wkv)]
            cs_k, cs_v = layer * 2 * d, layer * 2 * d + d
        else:
            if kvh.buf is None:
                kvh.buf = torch.empty(B * S, NKV, dtype=kv_all.dtype, device=dy.device)
            kv, dkv_all = kv_all, kvh.buf.view(B, S, -1)
        ext = _ExtKV(_layer_kv(kv, layer, d, heads), *ctx.kv8, _layer_kv(dkv_all, layer, d, heads),
                     _layer_kv(kvh.buf8, layer, d, heads), gk, kvh.part, cs_k, cs_v)
        dx = _attn_block_bwd(ctx, dy, x2, q, o, aux, kv_len, ext)
        # Only layer 0 hands the (by then complete) shared buffer to autograd;
        # the other layers contribute through the side channel, so no adds.
        dkv_ret = None
        if layer == 0:  # (kvh.f8b: autograd gets a zero-stride placeholder of the right shape)
            dkv_ret = dkv_all if dkv_all is not None else torch.zeros(
                1, dtype=kv_all.dtype, device=dy.device).expand(kv_all.shape)
        return (dx, dkv_ret) + (None,) * CrossAttnBlockFn.NO_GRAD_ARGS


# =============================================================================== feed-forward block
# the bf16 training forward's FFN1 GEMM also writes its ReLU mask as a bitmap
# (1 bit per hidden element); the ReLU-backward dgrad reads that, prefetched
# before its main loop, instead of the bf16 hidden activation (0: the bf16 mask)
RELU_BITS = os.environ.get("TDG_RELU_BITS", "1") != "0"


class FFNBlockFn(torch.autograd.Function):
    """y = LN(x + dropout(Dense(d)(Dense(ff, relu)(x))))."""

    NO_GRAD_ARGS = 8  # forward arguments after x
    @staticmethod
    def forward(ctx, x, w1: Param, b1: Param, w2: Param, b2: Param, gamma: Param, beta: Param,
                site: int, rt: RunCtx):
        B, L, d = x.shape
        x2 = x.reshape(B * L, d)
        ctx.p = (w1, b1, w2, b2, gamma, beta)
        ctx.meta = (site, rt)
        ctx.f8 = None
        ctx.lean = False
        ctx.hbits = None
        if x.is_cuda and rt.fp8 is not None:
            st = rt.fp8
            xs, hs = st.ffn_slots[id(w1)]
            w1_8, s1 = st.weights.get(w1)
            w2_8, s2 = st.weights.get(w2)
            x8 = st.stash.pop(xs, None)  # fused into the producing LayerNorm
            if x8 is None:
                x8 = fp8.quantize(x2, st.meta, xs)
            x8 = x8.view(x2.shape)
            # lean: the backward runs entirely on the e4m3 copies (fp8 weight
            # gradients, ReLU mask from h8), so the bf16 hidden is not written
            lean = (rt.training and rt.wgrad is not None and fp8.WGRAD_FP8
                    and st.ffn_bwd_slots.get(id(w1)) is not None
                    and fp8.wgrad_fp8_ok(B * L, d, w1.shape[0]))
            h, h8 = fp8.gemm_fp8(x8, w1_8, b1.master, st.meta, xs, s1, relu=True, out8_slot=hs,
                                 want_y=not lean)
            f, _ = fp8.gemm_fp8(h8, w2_8, b2.master, st.meta, hs, s2)
            # the e4m3 copies feed the fp8 weight gradients of the backward
            ctx.f8 = (x8, h8) if rt.training else None
            ctx.lean = lean
        elif x.is_cuda:
            ff = w1.shape[0]
            hbits = None
            if RELU_BITS and rt.training and ff % 8 == 0:
                hbits = torch.empty(B * L, ff // 8, dtype=torch.uint8, device=x.device)
            h = K.linear_fwd(x2, w1.compute, b1.master, relu=True, relu_bits=hbits)
            ctx.hbits = hbits
            f = None  # second projection fused with the LayerNorm below
        else:
            h = torch.relu(x2 @ w1.master.t() + b1.master)
            f = h @ w2.master.t() + b2.master
        if f is None:
            y, ctx.ln = _proj_ln_fwd(h, w2, b2, x, gamma, beta, site, rt)
        else:
            y, ctx.ln = _ln_fwd(x, f.view(B, L, d), gamma, beta, site, rt)
        ctx.save_for_backward(x2, h if h is not None else x2)  # (lean: h unused)
        return y

    @staticmethod
    def backward(ctx, dy):
        w1, b1, w2, b2, gamma, beta = ctx.p
        site, rt = ctx.meta
        x2, h = ctx.saved_tensors
        B, L, d = dy.shape
        ff = w1.shape[0]
        bt = _beta(rt)
        f8w = ctx.lean
        bw = rt.fp8.ffn_bwd_slots.get(id(w1)) if (dy.is_cuda and rt.fp8 is not None) else None
        # lean fp8 backward: the LayerNorm backward emits ds directly in e5m2
        dh, ds = _ln_bwd(dy, ctx.ln, gamma, beta, b2, site, rt, ds8_slot=bw[0] if f8w else None)
        ds2 = ds.reshape(B * L, d)
        if dy.is_cuda:
            if not f8w:
                _wgrad(rt, ds2, h, d, w2)
            if bw is not None:
                # fp8 backward: e5m2 gradients x e4m3 weights on the
                # block-scaled MFMA; the ReLU-backward dgrad also emits the e5m2
                # copy of its output for the next dgrad, which accumulates the
                # residual gradient already in dh
                st = rt.fp8
                gs, gh = bw
                M = B * L
                ds8 = ds2 if f8w else fp8.quantize(ds2, st.gmeta, gs)
                wp = fp8.DGRAD_PLAIN_W  # plain e4m3 weights read N-contiguous
                w2t8, s2t = st.weights.get(w2, transposed=not wp)
                w1t8, s1t = st.weights.get(w1, transposed=not wp)
                if f8w:
                    # lean fp8 backward: the ReLU-backward dgrad writes only
                    # the e5m2 dpre8 and, from its epilogue, b1's gradient
                    # (column sums); the mask is the forward's e4m3 hidden h8;
                    # weight gradients: e5m2 gradients x the forward's e4m3
                    # inputs (FFN1 input x8, hidden h8), token-major
                    x8, h8 = ctx.f8
                    xs, hs = st.ffn_slots[id(w1)]
                    q, folds = rt.wgrad, []
                    # (b1's column-sum fold deferred to the wgrad flush with
                    # the LayerNorm folds: one launch instead of one per layer)
                    dpre8 = fp8.gemm_bf8_dgrad(ds8, st.gmeta, gs, w2t8, st.meta, s2t, None,
                                               relu_aux8=h8.view(M, ff), out8_slot=gh,
                                               colsum_out=b1.grad, colsum_beta=bt, w_plain=wp,
                                               defer=folds)
                    q.defer_fold(folds, (b1,), rt)
                    q.add_fp8(ds8.view(M, d), st.gmeta.s(gs), h8.view(M, ff), st.meta.s(hs), w2, bt, rt)
                    q.add_fp8(dpre8.view(M, ff), st.gmeta.s(gh), x8.view(M, d), st.meta.s(xs), w1, bt, rt)
                else:
                    dpre = torch.empty(M, ff, dtype=ds2.dtype, device=ds2.device)
                    dpre8 = fp8.gemm_bf8_dgrad(ds8, st.gmeta, gs, w2t8, st.meta, s2t, dpre, relu_aux=h,
                                               out8_slot=gh, w_plain=wp)
                    _wgrad(rt, dpre, x2, ff, w1, b1)
                fp8.gemm_bf8_dgrad(dpre8, st.gmeta, gh, w1t8, st.meta, s1t, dh.view(M, d), beta=1.0,
                                   w_plain=wp)
                return (dh.view(B, L, d),) + (None,) * FFNBlockFn.NO_GRAD_ARGS
            # ReLU mask: the forward's bitmap if it wrote one (h is still saved:
            # the W2 weight gradient reads it)
            mask = dict(relu_bits=ctx.hbits) if ctx.hbits is not None else dict(relu_aux=h)
            if w2.compute_t is not None and not w2.compute_t_stale:
                # NT layout against W2^T (ParamStore.add_transposed; stale while
                # an fp8 backward had the re-transposes paused: NN below)
                dpre = K.linear_dgrad_t(ds2, w2.compute_t, **mask)
            else:
                dpre = K.linear_dgrad(ds2, w2.compute, d, **mask)
            _wgrad(rt, dpre, x2, ff, w1, b1)
        else:
            _write_grad(w2, ds2.t() @ h, rt)
            _ready(rt, w2)
            dpre = (ds2 @ w2.master) * (h > 0).to(ds2.dtype)
            _write_grad(w1, dpre.t() @ x2, rt)
            _write_grad(b1, dpre.sum(0), rt)
            _ready(rt, w1, b1)  # (GPU: reported by _wgrad / the deferred flush)
        dx = _dgrad_into(dpre, w1, ff, dh)
        return (dx.view(B, L, d),) + (None,) * FFNBlockFn.NO_GRAD_ARGS
