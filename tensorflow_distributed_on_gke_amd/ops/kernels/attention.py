"""Attention family (csrc/kernels/attention.hip): bf16 / fp8 forward and
backward, the fused Q|K|V forward, and the CPU reference forward."""
from __future__ import annotations

import os
from typing import Optional

import torch

from tensorflow_distributed_on_gke_amd.ops._ext import C
from tensorflow_distributed_on_gke_amd.ops.kernels.workspace import workspace


def _ref_attn_fwd(q, k, v, kv_len, causal, scale):
    """q [B,Lq,H,hd] ... -> out [B,Lq,H,hd], probs [B,H,Lq,Lk]. Masked logits
    get -1e9 added exactly as the reference does (transformer_model.py:101-102)."""
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) * scale
    B, H, Lq, Lk = s.shape
    mask = torch.zeros(B, 1, Lq, Lk, dtype=s.dtype, device=s.device)
    keys = torch.arange(Lk, device=s.device)
    if kv_len is not None:
        mask = mask + (keys.view(1, 1, 1, Lk) >= kv_len.view(B, 1, 1, 1).to(keys.device)).to(s.dtype)
    if causal:
        qs = torch.arange(Lq, device=s.device)
        mask = torch.maximum(mask, (keys.view(1, Lk) > qs.view(Lq, 1)).to(s.dtype).view(1, 1, Lq, Lk))
    p = torch.softmax(s + mask * -1e9, dim=-1)
    out = torch.einsum("bhqk,bkhd->bqhd", p, v)
    return out, p


def attn_fwd(q, k, v, kv_len, scale: float, causal: bool):
    B, Lq, H, hd = q.shape
    out = torch.empty(B, Lq, H, hd, dtype=torch.bfloat16, device=q.device)
    lse = torch.empty(B, H, Lq, dtype=torch.float32, device=q.device)
    C().attn_fwd(q, k, v, out, lse, kv_len, scale, causal)
    return out, lse


# self-attention of <= 128 tokens: the Q|K|V projection and the attention
# forward in one launch (attn_qkv.h qkv_attn_fwd_kernel)
QKV_ATTN = os.environ.get("TDG_QKV_ATTN", "1") != "0"


def qkv_attn_fwd(x2, w, bias, B: int, heads: int, kv_len, scale: float, causal: bool,
                 k=None, v=None):
    """(qkv [M, 3d], out [B, L, H, hd], lse [B, H, L]) of the self-attention
    over qkv = x2 @ w^T + bias, one launch; None when the shape is not covered
    (L > 128, hd != 64). k / v ([B, Lk, H, 64] views): the cross-attention
    form -- w / bias the Q projection's, the first result q [M, d]."""
    M, d = x2.shape
    L, hd = M // B, d // heads
    if not QKV_ATTN or L > 128 or hd != 64 or (k is not None and k.shape[1] > 128):
        return None
    np_ = 1 if k is not None else 3
    qkv = torch.empty(M, np_ * d, dtype=torch.bfloat16, device=x2.device)
    out = torch.empty(B, L, heads, hd, dtype=torch.bfloat16, device=x2.device)
    lse = torch.empty(B, heads, L, dtype=torch.float32, device=x2.device)
    if not C().qkv_attn_fwd(x2, w, bias, qkv, out, lse, kv_len, scale, causal, B, heads, k, v):
        return None
    return qkv, out, lse


def attn_fwd_fp8_ok(Lq: int, Lk: int, hd: int) -> bool:
    """Shapes the e4m3 attention forward covers (attn_f8.h
    attn_fwd_fp8_kernel): hd 64, the long-sequence path."""
    return hd == 64 and Lq > 128


def attn_fwd_fp8(q8, k8, v8, sq, sk, sv, kv_len, scale: float, causal: bool, o8=None, so8=None,
                 amax8=None):
    """Attention forward on e4m3 copies q8 = e4m3(q * sq) etc. (per-tensor
    scales, one-element device tensors): O (bf16) and the log2-domain LSE, as
    attn_fwd. o8 ([B, Lq, H, hd] e4m3, with its scale so8 and amax slot
    amax8): also O's e4m3 copy from the epilogue (= quantising the bf16 O)."""
    B, Lq, H, hd = q8.shape
    out = torch.empty(B, Lq, H, hd, dtype=torch.bfloat16, device=q8.device)
    lse = torch.empty(B, H, Lq, dtype=torch.float32, device=q8.device)
    C().attn_fwd_fp8(q8, k8, v8, out, lse, kv_len, sq, sk, sv, scale, causal, o8, so8, amax8)
    return out, lse


def attn_bwd(q, k, v, o, dout, lse, dq, dk, dv, kv_len, scale: float, causal: bool):
    delta = workspace("attn_delta", lse.numel(), q.device)[: lse.numel()]
    C().attn_bwd(q, k, v, o, dout, lse, delta, dq, dk, dv, kv_len, scale, causal)


# the fused backward of <= 128-token attention computes dO = dY @ Wo[:, head]
# itself (the output projection's dgrad, never written to memory)
ATTN_BWD_FDO = os.environ.get("TDG_ATTN_BWD_FDO", "1") != "0"


def attn_bwd_fdo(q, k, v, o, dy2, wo, lse, dq, dk, dv, kv_len, scale: float, causal: bool) -> bool:
    """attn_bwd with dout = (dy2 @ wo).view(q.shape) computed in-kernel; False
    (nothing launched) when not covered (Lq / Lk > 128, hd != 64)."""
    if not ATTN_BWD_FDO:
        return False
    delta = workspace("attn_delta", lse.numel(), q.device)[: lse.numel()]
    return C().attn_bwd_fdo(q, k, v, o, dy2, wo, lse, delta, dq, dk, dv, kv_len, scale, causal)


def attn_bwd_g8_ok(Lq: int, Lk: int, hd: int) -> bool:
    """Shapes whose attention backward can emit e5m2 gradients (the hd-64
    pipelined kernels, attn_bwd.h attn_emit_g8)."""
    return hd == 64 and (Lq > 128 or Lk > 128)


def attn_bwd_g8(q, k, v, o, dout, lse, dq, dk, dv, kv_len, scale: float, causal: bool, dq8,
                dk8, dv8, sg8, amax8, cs_part, cs_ld: int, cs_q: int, cs_k: int, cs_v: int,
                skip_bf16: Optional[bool] = None) -> int:
    """attn_bwd that also writes e5m2 copies dq8 (dk8 / dv8 optional, same
    layout as dq / dk / dv) = e5m2(bf16(grad) * sg8), their amax into the
    slot amax8, and the bias-gradient column-sum partials cs_part[B *
    nblocks, cs_ld] (columns cs_q / cs_k / cs_v + head * 64 + j). skip_bf16:
    the bf16 dq / dk / dv are not written (default: when the e5m2 dk8 / dv8
    are requested -- without them the bf16 dK / dV are the output and must be
    written). Returns the partial row count."""
    if skip_bf16 is None:
        skip_bf16 = dk8 is not None
    B, Lq = q.shape[0], q.shape[1]
    np_ = -(-Lq // 128)
    delta = workspace("attn_delta", lse.numel(), q.device)[: lse.numel()]
    C().attn_bwd_g8(q, k, v, o, dout, lse, delta, dq, dk, dv, kv_len, scale, causal, dq8, dk8, dv8,
                    sg8, amax8, cs_part, np_, cs_ld, cs_q, cs_k, cs_v, skip_bf16)
    return B * np_


def attn_bwd_f8_ok(Lq: int, Lk: int, hd: int) -> bool:
    """Shapes the fp8 attention backward covers (attn_f8.h
    attn_bwd_f8_kernel: every key of a (batch, head) in one workgroup)."""
    return hd == 64 and 128 < Lq <= 512 and Lk <= 512


def attn_bwd_f8(q8, k8, v8, sq, sk, sv, o, do8, sdo, lse, kv_len, scale: float, causal: bool,
                sds, amaxds, dq=None, dk=None, dv=None, dq8=None, dk8=None, dv8=None, sg8=None,
                amaxg8=None, cs_part=None, cs_ld: int = 0, cs_q: int = 0, cs_k: int = 0,
                cs_v: int = 0, sgkv8=None, amaxgkv8=None, cs_part2=None, cs_ld2: int = 0) -> int:
    """Attention backward on fp8 MFMAs: the forward's e4m3 q8 / k8 / v8
    (scales sq / sk / sv), the e5m2 do8 (scale sdo), bf16 o and the forward's
    lse; dS in e5m2 with scale sds (its amax into the slot amaxds). Writes each
    given output: bf16 dq / dk / dv, e5m2 dq8 / dk8 / dv8 = e5m2(bf16(grad) *
    sg8) (amax into amaxg8) and the bias-gradient column sums of the e5m2
    outputs, one row per batch element: cs_part[b, cs_{q,k,v} + head * 64 + j].
    sgkv8 / amaxgkv8: dk8 / dv8 in their own e5m2 slot (the batched cross
    K|V gradient); cs_part2 / cs_ld2: their column sums in a buffer of their
    own. Returns the partial row count (B)."""
    C().attn_bwd_f8(q8, k8, v8, sq, sk, sv, o, do8, sdo, lse, kv_len, scale, causal, sds, amaxds,
                    dq, dk, dv, dq8, dk8, dv8, sg8, amaxg8, cs_part, cs_ld, cs_q, cs_k, cs_v, sgkv8,
                    amaxgkv8, cs_part2, cs_ld2)
    return q8.shape[0]


def attn_probs(q, k, kv_len, scale: float, causal: bool) -> torch.Tensor:
    B, Lq, H, hd = q.shape
    Lk = k.shape[1]
    probs = torch.empty(B, H, Lq, Lk, dtype=torch.float32, device=q.device)
    C().attn_probs(q, k, probs, kv_len, scale, causal)
    return probs
