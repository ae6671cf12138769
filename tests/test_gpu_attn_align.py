"""attn_align_kernel (csrc/kernels/attn_align.hip) on the MI355X against the
float64 reference of tests/ref_align.py, evaluated on the bf16-rounded inputs.

Shapes: one key; a partial key block; a block edge; all four waves with
unequal block counts (130 keys: 3, 2, 2, 2 blocks); the longest row (1000
keys, NKB 16). Each case has a batch row with every key, one with kv_len 1,
one whose arg-max range is empty under k_lo = k_trim = 1 (kv_len 2), and a
ragged one. Measured worst |soft - ref| and |conf - ref| over these cases:
7.7e-8 (profiles/align_cost.txt); the bound is ref_align.TOL = 6.96e-6,
attn_probs' own.
"""
import pytest
import torch

import ref_align as RA
from tensorflow_distributed_on_gke_amd.ops.kernels import attention as KA

pytestmark = pytest.mark.gpu
DEV = "cuda"

#        hd  H   Lq   Lk  q_len  strided
CASES = [(16, 1, 1, 1, False, False),
         (32, 5, 17, 15, True, False),
         (64, 8, 16, 17, False, True),
         (128, 5, 40, 130, True, False),
         (64, 8, 33, 1000, False, False),
         (16, 8, 40, 130, False, True),
         (32, 1, 33, 1000, True, True),
         (128, 8, 17, 15, False, False)]


def _views(B, Lq, Lk, H, hd, strided, gen):
    """bf16 (q [B, Lq, H, hd], k [B, Lk, H, hd]) on the CPU and the same views
    on the GPU; strided: q cut from a packed [M, 3d] projection, k from the
    stacked K|V [B, Lk, 2, H, hd]."""
    d = H * hd
    if not strided:
        q, k = RA.bf(torch.randn(B, Lq, H, hd, generator=gen)), RA.bf(torch.randn(B, Lk, H, hd, generator=gen))
        return (q, k), (q.to(DEV), k.to(DEV))
    qkv = RA.bf(torch.randn(B * Lq, 3 * d, generator=gen))
    kv = RA.bf(torch.randn(B, Lk, 2 * d, generator=gen))
    cut = lambda x, y: (x[:, :d].view(B, Lq, H, hd), y.view(B, Lk, 2, H, hd)[:, :, 0])  # noqa: E731
    return cut(qkv, kv), cut(qkv.to(DEV), kv.to(DEV))


def _run(qk_dev, kv_len, scale, q_len, k_lo, k_trim, want_soft=True):
    out = KA.attn_align(*qk_dev, kv_len.to(DEV), scale, None if q_len is None else q_len.to(DEV),
                        k_lo, k_trim, want_soft=want_soft)
    torch.cuda.synchronize()
    return tuple(t if t is None else t.cpu() for t in out)


@pytest.mark.parametrize("hd,H,Lq,Lk,with_qlen,strided", CASES)
def test_against_float64(hd, H, Lq, Lk, with_qlen, strided):
    B = 4
    gen = torch.Generator().manual_seed(hd * 1000 + Lk)
    (q, k), dev = _views(B, Lq, Lk, H, hd, strided, gen)
    kv_len = torch.tensor([Lk, 1, 2, (Lk * 2) // 3 + 1], dtype=torch.int32).clamp(max=Lk)
    q_len = torch.tensor([Lq, 0, 1, Lq // 2 + 1], dtype=torch.int32) if with_qlen else None
    scale = hd ** -0.5
    got = _run(dev, kv_len, scale, q_len, 1, 1)
    RA.check(got, RA.reference(q, k, kv_len, scale, q_len, 1, 1), kv_len, q_len,
             f"hd{hd} H{H} {Lq}x{Lk}")
    again = _run(dev, kv_len, scale, q_len, 1, 1)  # fixed reduction order: bitwise the same
    assert all(torch.equal(x, y) for x, y in zip(got, again))
    h2, c2, s2 = _run(dev, kv_len, scale, q_len, 1, 1, want_soft=False)
    assert s2 is None and torch.equal(h2, got[0]) and torch.equal(c2, got[1])


@pytest.mark.parametrize("hd,H,L", [(16, 5, 40), (64, 8, 130)])
def test_planted_keys_and_exact_ties(hd, H, L):
    """k[perm[i]] = 2 q[i] in every head (q rows of one norm, so a row's own
    key has the largest logit in every head): hard is the permutation. Then
    every planted key twice: the two copies tie bitwise, the lower index wins
    and conf equals both copies' soft."""
    gen = torch.Generator().manual_seed(L)
    q = torch.randn(1, L, H, hd, generator=gen)
    q = RA.bf(q / q.norm(dim=-1, keepdim=True) * hd ** 0.5)
    perm = torch.randperm(L, generator=gen)
    k = torch.empty_like(q)
    k[0, perm] = q[0] * 2
    kv_len = torch.tensor([L], dtype=torch.int32)
    hard, _, _ = _run((q.to(DEV), k.to(DEV)), kv_len, hd ** -0.5, None, 0, 0)
    assert torch.equal(hard[0].long(), perm)
    slots = torch.randperm(2 * L + 3, generator=gen)
    a, b = slots[:L], slots[L:2 * L]
    k2 = RA.bf(torch.randn(1, 2 * L + 3, H, hd, generator=gen))
    k2[0, a] = q[0] * 2
    k2[0, b] = q[0] * 2
    hard, conf, soft = _run((q.to(DEV), k2.to(DEV)), torch.tensor([2 * L + 3], dtype=torch.int32),
                            hd ** -0.5, None, 0, 0)
    assert torch.equal(hard[0].long(), torch.minimum(a, b))
    rows = torch.arange(L)
    assert torch.equal(conf[0], soft[0, rows, a]) and torch.equal(conf[0], soft[0, rows, b])


def test_too_many_keys_raises():
    q = torch.zeros(1, 1, 1, 16, dtype=torch.bfloat16, device=DEV)
    k = torch.zeros(1, KA.ALIGN_MAX_LK + 1, 1, 16, dtype=torch.bfloat16, device=DEV)
    with pytest.raises((ValueError, RuntimeError)):
        KA.attn_align(q, k, torch.ones(1, dtype=torch.int32, device=DEV), 1.0)
