"""Long sequences on the GPU: the attention kernels and the training step past
512 keys.

The reference filters nothing by length (english_portugese_dataset.py:34-47)
and sizes its positional-encoding table for 1000 positions
(__main__.py:82-83, transformer_model.py:29-53), so sequences up to 1000 are
part of its workload; SURVEY §5 asks for 512..8k. Covered here:

* bf16 attention forward + backward (the streaming multi-tile kernels:
  attn_fwd.h attn_fwd_pipe_kernel, attn_bwd.h attn_bwd_dq_pipe_kernel /
  attn_bwd_dkdv_pipe_kernel for hd 64, the register-staged kernels for hd 16)
  at Lq = Lk in {1000, 2048, 4096} with padding and look-ahead masks, against
  fp32 autograd of the same attention (computed on the GPU in fp32: the CPU
  would need minutes at 4096);
* the e4m3 forward (attn_fwd_fp8_kernel) at 1000 and 2048 against fp32
  attention of the dequantised inputs;
* the backward the fp8 step takes above 512 keys (the fp8 kernel keeps every
  key of a (batch, head) in one workgroup and stops at 512; longer sequences
  run the bf16 backward with e5m2 outputs, attn_bwd_g8), against the plain
  bf16 backward;
* a whole Transformer-base training step at 1000 source and target tokens,
  bf16 and fp8: the HIP-graph replay equals the eager step bitwise.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ref_attn(q, k, v, kv_len, causal, scale):
    """fp32 attention on the GPU (torch ops; the reference, not the path under test)."""
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) * scale
    B, H, Lq, Lk = s.shape
    keys = torch.arange(Lk, device=q.device)
    mask = (keys.view(1, 1, 1, Lk) >= kv_len.view(B, 1, 1, 1).long())
    if causal:
        mask = mask | (keys.view(1, Lk) > torch.arange(Lq, device=q.device).view(Lq, 1)).view(1, 1, Lq, Lk)
    s = s.masked_fill(mask, float("-inf"))
    p = torch.softmax(s, -1)
    return torch.einsum("bhqk,bkhd->bqhd", p, v)


def _close(a, b, tol, what):
    err = (a.float() - b.float()).abs().max().item()
    ref = b.float().abs().max().item() + 1e-6
    assert err <= tol * ref, f"{what}: max err {err:.3e} vs max |ref| {ref:.3e}"


@pytest.mark.parametrize("L", [1000, 2048, 4096])
@pytest.mark.parametrize("hd", [16, 64])
@pytest.mark.parametrize("mask", ["pad", "causal"])
def test_attention_long_bf16_fwd_bwd(L, hd, mask):
    from tensorflow_distributed_on_gke_amd.ops import kernels as kk
    torch.manual_seed(L + hd)
    B, H = 2, 2
    causal = mask == "causal"
    q, k, v = (torch.randn(B, L, H, hd, device=DEV).bfloat16() for _ in range(3))
    # padding: one full row and one cut mid-sequence (not at a tile boundary)
    kv_len = torch.tensor([L, L - 389 if not causal else L], dtype=torch.int32, device=DEV)
    scale = 1 / math.sqrt(hd)
    out, lse = kk.attn_fwd(q, k, v, kv_len, scale, causal)
    qr, kr, vr = (t.float().requires_grad_() for t in (q, k, v))
    ref = _ref_attn(qr, kr, vr, kv_len, causal, scale)
    _close(out, ref.detach(), 2e-2, f"attn fwd L={L} hd={hd} {mask}")
    dout = torch.randn(B, L, H, hd, device=DEV).bfloat16()
    ref.backward(dout.float())
    dq, dk, dv = (torch.empty_like(t) for t in (q, k, v))
    kk.attn_bwd(q, k, v, out, dout, lse, dq, dk, dv, kv_len, scale, causal)
    torch.cuda.synchronize()
    _close(dv, vr.grad, 3e-2, f"attn dv L={L}")
    _close(dk, kr.grad, 3e-2, f"attn dk L={L}")
    _close(dq, qr.grad, 3e-2, f"attn dq L={L}")
    # keys past kv_len get no gradient
    if not causal:
        n = int(kv_len[1])
        assert dk[1, n:].float().abs().max().item() == 0.0
        assert dv[1, n:].float().abs().max().item() == 0.0


@pytest.mark.parametrize("L", [1000, 2048])
@pytest.mark.parametrize("causal", [False, True])
def test_attention_long_fp8_forward(L, causal):
    from tensorflow_distributed_on_gke_amd.ops import kernels as kk
    torch.manual_seed(11)
    B, H, hd = 2, 2, 64
    q, k, v = (torch.randn(B, L, H, hd, device=DEV).bfloat16() for _ in range(3))
    kv_len = torch.tensor([L, L - 389 if not causal else L], dtype=torch.int32, device=DEV)
    sc = [torch.tensor([448.0 / t.float().abs().max().item()], device=DEV) for t in (q, k, v)]
    q8, k8, v8 = ((t.float() * s).clamp(-448, 448).to(torch.float8_e4m3fn) for t, s in zip((q, k, v), sc))
    scale = hd ** -0.5
    out, lse = kk.attn_fwd_fp8(q8, k8, v8, sc[0], sc[1], sc[2], kv_len, scale, causal)
    qd, kd, vd = (t8.float() / s for t8, s in zip((q8, k8, v8), sc))
    ref = _ref_attn(qd, kd, vd, kv_len, causal, scale)
    err = (out.float() - ref).abs().max().item() / ref.abs().max().item()
    assert err < 4e-2, err
    # the log2-domain LSE of the fp32 logits
    s = torch.einsum("bqhd,bkhd->bhqk", qd, kd) * scale
    keys = torch.arange(L, device=DEV)
    m = (keys.view(1, 1, 1, L) >= kv_len.view(B, 1, 1, 1).long())
    if causal:
        m = m | (keys.view(1, L) > keys.view(L, 1)).view(1, 1, L, L)
    lref = torch.logsumexp(s.masked_fill(m, float("-inf")), -1) / math.log(2.0)
    assert (lse - lref).abs().max().item() < 2e-2


@pytest.mark.parametrize("L", [1000, 2048])
def test_fp8_step_backward_past_512_keys(L):
    """What the fp8 step's attention backward runs above 512 keys: the bf16
    pipelined backward that also emits the e5m2 dQ|dK|dV (attn_bwd_g8) --
    its bf16 outputs are bitwise the plain backward's, its e5m2 copies the
    quantised bf16 ones."""
    from tensorflow_distributed_on_gke_amd.ops import fp8 as F
    from tensorflow_distributed_on_gke_amd.ops import kernels as kk
    assert not kk.attn_bwd_f8_ok(L, L, 64) and kk.attn_bwd_g8_ok(L, L, 64)
    torch.manual_seed(3)
    B, H, hd = 2, 2, 64
    q, k, v = (torch.randn(B, L, H, hd, device=DEV).bfloat16() for _ in range(3))
    kv_len = torch.tensor([L, L - 100], dtype=torch.int32, device=DEV)
    scale = hd ** -0.5
    out, lse = kk.attn_fwd(q, k, v, kv_len, scale, True)
    dout = (torch.randn(B, L, H, hd, device=DEV) * 0.1).bfloat16()
    ref = [torch.empty_like(t) for t in (q, k, v)]
    kk.attn_bwd(q, k, v, out, dout, lse, *ref, kv_len, scale, True)
    gm = F.Fp8Meta(DEV, fmt=1)
    ig = gm.slot("g")
    gm.scale[ig] = 256.0
    got = [torch.empty_like(t) for t in (q, k, v)]
    g8 = [torch.empty(t.shape, dtype=gm.dtype, device=DEV) for t in (q, k, v)]
    part = torch.zeros(B * -(-L // 128), 3 * H * hd, device=DEV)
    kk.attn_bwd_g8(q, k, v, out, dout, lse, *got, kv_len, scale, True, g8[0], g8[1], g8[2],
                   gm.s(ig), gm.a(ig), part, 3 * H * hd, 0, H * hd, 2 * H * hd, skip_bf16=False)
    torch.cuda.synchronize()
    for a, b, a8 in zip(got, ref, g8):
        assert torch.equal(a, b)
        want = (b.float() * 256.0).clamp(-57344, 57344).to(gm.dtype)
        assert torch.equal(a8.view(torch.uint8), want.view(torch.uint8))


def _long_batches(dev, B, S, T, n):
    g = torch.Generator().manual_seed(5)
    out = []
    for i in range(n):
        src = torch.randint(4, 7000, (B, S), generator=g)
        tgt = torch.randint(4, 7000, (B, T + 1), generator=g)
        src[1, S - 137 - i:] = 0  # padded rows, cut mid-tile
        tgt[1, T - 201 - 3 * i:] = 0
        out.append((src.to(dev), tgt.to(dev)))
    return out


def _train(graph, fp8, steps=2, B=4, L=1000):
    from tensorflow_distributed_on_gke_amd.models.transformer import Transformer, model_config
    from tensorflow_distributed_on_gke_amd.ops import tuning
    from tensorflow_distributed_on_gke_amd.train.optim import Adam
    from tensorflow_distributed_on_gke_amd.train.step import TrainStep

    tuning.AUTOTUNE = False  # identical GEMM configs in both runs
    cfg = model_config("base")
    m = Transformer(cfg).build(DEV, seed=2)
    opt = Adam(m.store, cfg.d_model)
    st = None
    if fp8:
        from tensorflow_distributed_on_gke_amd.ops.fp8 import Fp8State
        st = Fp8State(m)
    step = TrainStep(m, opt, None, workers=1, seed=3, fp8_state=st)
    bs = _long_batches(DEV, B, L, L, steps)
    if graph:
        assert step.capture(*bs[0], warmup=2)
        assert step.graph is not None and opt.iterations == 0
    losses = [step(*b).clone() for b in bs]
    torch.cuda.synchronize()
    return m.store.flat.clone(), torch.stack(losses)


@pytest.mark.parametrize("fp8", [False, True])
def test_train_step_seq1000_graph_matches_eager(fp8):
    """Transformer-base at 1000 source / target tokens (the reference's
    positional-encoding limit): the captured step replays bitwise like the
    eager one, the loss is finite (fp8: e4m3 attention forward, the bf16
    attention backward with e5m2 outputs, fp8 GEMMs)."""
    f_e, l_e = _train(False, fp8)
    f_g, l_g = _train(True, fp8)
    assert torch.isfinite(l_e).all() and (l_e[:, 0] > 0).all(), l_e
    assert torch.equal(l_e, l_g), (l_e, l_g)
    assert torch.equal(f_e, f_g)
