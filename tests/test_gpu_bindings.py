"""Host-side validation of the `_C` bindings: malformed operands must raise
RuntimeError before anything is launched, and the same call well-formed must
still compute attention. Shapes are the smallest the kernels take (B 1, L 16,
H 1, head dim 64)."""
import math

import pytest
import torch

from tensorflow_distributed_on_gke_amd.ops._ext import C

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, L, H, HD = 1, 16, 1, 64
SCALE = 1 / math.sqrt(HD)
SENTINEL = 7.0


@pytest.fixture(scope="module")
def ops():
    """q / k / v (bf16 on the GPU) and the fp32 softmax-attention reference."""
    g = torch.Generator().manual_seed(0)
    q, k, v = (torch.randn(B, L, H, HD, generator=g).to(torch.bfloat16) for _ in range(3))
    s = torch.einsum("bqhd,bkhd->bhqk", q.float(), k.float()) * SCALE
    ref = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, -1), v.float())
    return q.to(DEV), k.to(DEV), v.to(DEV), ref


def _outputs():
    out = torch.full((B, L, H, HD), SENTINEL, dtype=torch.bfloat16, device=DEV)
    lse = torch.full((B, H, L), SENTINEL, dtype=torch.float32, device=DEV)
    return out, lse


def _untouched(*tensors):
    torch.cuda.synchronize()
    for t in tensors:
        assert (t.float() == SENTINEL).all().item(), "a rejected call wrote to its output"


def test_attn_fwd_well_formed(ops):
    q, k, v, ref = ops
    out, lse = _outputs()
    C().attn_fwd(q, k, v, out, lse, None, SCALE, False)
    err = (out.float().cpu() - ref).abs().max().item()
    bound = 2e-2 * (ref.abs().max().item() + 1e-6)  # test_gpu_kernels.py attention forward
    assert err <= bound, f"attn fwd: max err {err:.3e} > {bound:.3e}"


def test_attn_fwd_misaligned_q(ops):
    q, k, v, _ = ops
    flat = torch.zeros(q.numel() + 8, dtype=torch.bfloat16, device=DEV)
    q1 = flat[1:1 + q.numel()].view(B, L, H, HD)  # one element (2 bytes) off a 16-byte boundary
    q1.copy_(q)
    out, lse = _outputs()
    with pytest.raises(RuntimeError):
        C().attn_fwd(q1, k, v, out, lse, None, SCALE, False)
    _untouched(out, lse)


def test_attn_fwd_int64_kv_len(ops):
    q, k, v, _ = ops
    out, lse = _outputs()
    kv_len = torch.full((B,), L, dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError):
        C().attn_fwd(q, k, v, out, lse, kv_len, SCALE, False)
    _untouched(out, lse)


def test_attn_bwd_short_lse(ops):
    q, k, v, _ = ops
    o = torch.zeros_like(q)
    dout = torch.zeros_like(q)
    lse = torch.zeros(B * H * L - 1, dtype=torch.float32, device=DEV)
    delta = torch.zeros(B * H * L, dtype=torch.float32, device=DEV)
    dq, dk, dv = (torch.full_like(q, SENTINEL) for _ in range(3))
    with pytest.raises(RuntimeError):
        C().attn_bwd(q, k, v, o, dout, lse, delta, dq, dk, dv, None, SCALE, False)
    _untouched(dq, dk, dv)


def test_attn_fwd_fp8_bf16_q(ops):
    q, k, v, _ = ops
    k8, v8 = k.to(torch.float8_e4m3fn), v.to(torch.float8_e4m3fn)
    one = torch.ones(1, dtype=torch.float32, device=DEV)
    out, lse = _outputs()
    with pytest.raises(RuntimeError):
        C().attn_fwd_fp8(q, k8, v8, out, lse, None, one, one, one, SCALE, False, None, None, None)
    _untouched(out, lse)


def test_ln_fwd_kbits_wrong_length():
    M, D = L, 512  # kbits need D >= 512: only the length is wrong here
    x = torch.zeros(M, D, dtype=torch.bfloat16, device=DEV)
    s = torch.zeros_like(x)
    gamma = torch.ones(D, dtype=torch.float32, device=DEV)
    beta = torch.zeros(D, dtype=torch.float32, device=DEV)
    y = torch.full_like(x, SENTINEL)
    kbits = torch.zeros(M * D // 8 - 1, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError):
        C().ln_fwd(x, s, gamma, beta, y, None, None, None, 0.1, 1, None, 0, 1e-6, None, None, None,
                   kbits)
    _untouched(y)


def test_gemm_lda_not_multiple_of_8():
    M, N, K, lda = 16, 16, 64, 68
    a = torch.zeros(M, lda, dtype=torch.bfloat16, device=DEV)
    b = torch.zeros(N, K, dtype=torch.bfloat16, device=DEV)
    c = torch.full((M, N), SENTINEL, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError):
        C().gemm(a, b, c, None, None, M, N, K, lda, K, N, 0, True, True, 0, 1.0, 0.0, 0, 1, None)
    _untouched(c)
