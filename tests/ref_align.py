"""Float64 reference of attn_align (csrc/kernels/attn_align.hip) and the
comparison both of its test files use. No GPU needed.

  P_h = softmax_j(scale q_h k_h^T) over j < kv_len[b];  A = mean_h P_h
  hard = argmax_j A over k_lo <= j < kv_len[b] - k_trim (lowest j on ties, -1
  if empty), conf = A[hard]; rows >= q_len[b]: hard -1, conf 0, soft 0.
"""
import ref_attn as A
import torch

F64 = torch.float64
# The bound of the float64 test of attn_probs (ref_attn.E32["attn_probs"] with
# the table's margin), taken as an absolute error of a probability: the same
# exponent and normaliser, plus a mean over <= 16 heads. Measured on the
# MI355X over the cases of test_gpu_attn_align.py: profiles/align_cost.txt.
TOL = A.R.tol("attn_probs")


def bf(x):
    return x.to(torch.bfloat16)


def reference(q, k, kv_len, scale, q_len=None, k_lo=0, k_trim=0):
    """(A [B, Lq, Lk] f64, hard [B, Lq], conf [B, Lq], gap [B, Lq]): gap = best
    minus second best of A in the arg-max range (inf with fewer than two keys)."""
    B, Lq, H, _ = q.shape
    Lk = k.shape[1]
    kvl = kv_len.long().clamp(0, Lk)
    ql = q_len.long().clamp(0, Lq) if q_len is not None else torch.full((B,), Lq)
    s = torch.einsum("bqhd,bkhd->bhqk", q.to(F64), k.to(F64)) * scale
    keys = torch.arange(Lk)
    att = keys.view(1, Lk) < kvl.view(B, 1)
    p = torch.softmax(s.masked_fill(~att.view(B, 1, 1, Lk), -float("inf")), -1)
    p = torch.where(att.view(B, 1, 1, Lk), p, torch.zeros_like(p))  # (kv_len 0: NaN -> 0)
    rows = torch.arange(Lq).view(1, Lq) < ql.view(B, 1)
    a = p.mean(1) * rows.unsqueeze(-1)
    rng = (keys.view(1, Lk) >= k_lo) & (keys.view(1, Lk) < (kvl - k_trim).view(B, 1))
    m = torch.where(rng.view(B, 1, Lk), a, torch.full_like(a, -1.0))
    top = m.topk(min(2, Lk), -1).values
    ok = rows & (top[..., 0] >= 0)
    first = (m == top[..., :1]).long().argmax(-1)
    hard = torch.where(ok, first, torch.full_like(first, -1))
    conf = torch.where(ok, top[..., 0], torch.zeros_like(top[..., 0]))
    gap = top[..., 0] - top[..., 1] if Lk > 1 else torch.full_like(conf, float("inf"))
    gap = torch.where(top[..., -1] < 0, torch.full_like(gap, float("inf")), gap)  # one key in range
    return a, hard, conf, gap


def check(got, ref, kv_len, q_len, what):
    """got = (hard, conf, soft) of the code under test (CPU tensors). Returns
    the worst absolute error of soft / conf."""
    hard, conf, soft = got
    a, rhard, rconf, gap = ref
    B, Lq, Lk = a.shape
    assert soft.shape == (B, Lq, -(-Lk // 8) * 8), what
    err = max(float((soft[..., :Lk].to(F64) - a).abs().max()), float((conf.to(F64) - rconf).abs().max()))
    print(f"{what}: max abs err {err:.3e} (tol {TOL:.3e})")
    assert err <= TOL, f"{what}: soft / conf off by {err:.3e} > {TOL:.3e}"
    ql = q_len.long() if q_len is not None else torch.full((B,), Lq)
    outside = ((torch.arange(soft.shape[-1]).view(1, 1, -1) >= kv_len.long().view(B, 1, 1)) |
               (torch.arange(Lq).view(1, Lq, 1) >= ql.view(B, 1, 1)))
    assert bool((soft[outside.expand_as(soft)] == 0).all()), f"{what}: soft outside q_len / kv_len not exactly 0"
    valid = rhard >= 0
    assert bool((hard[~valid] == -1).all()) and bool((conf[~valid] == 0).all()), f"{what}: invalid rows"
    sure = valid & (gap > 2 * TOL)
    assert int((valid & ~sure).sum()) <= 0.05 * int(valid.sum()), f"{what}: too many near-ties in the reference"
    assert torch.equal(hard[sure].long(), rhard[sure]), f"{what}: hard differs where the reference is decided"
    picked = soft.gather(-1, hard.clamp_min(0).long().unsqueeze(-1)).squeeze(-1)
    assert torch.equal(conf[valid], picked[valid]), f"{what}: conf is not soft[hard]"
    return err
