"""Attention dropout on the CPU: the setting's check, the reference backward
against float64 autograd of the reference forward under one mask, and the CPU
model with and without it."""
import pytest
import torch

from tensorflow_distributed_on_gke_amd.config import Settings, check_attention_dropout, load_settings
from tensorflow_distributed_on_gke_amd.models.layers import RunCtx, _ref_attn_bwd
from tensorflow_distributed_on_gke_amd.models.transformer import Transformer, model_config
from tensorflow_distributed_on_gke_amd.ops.kernels.attention import _ref_attn_fwd, attn_keep_scale


def test_check_attention_dropout():
    assert Settings().attention_dropout == 0.0 and model_config("tiny").attention_dropout == 0.0
    assert check_attention_dropout(0) == 0.0 and check_attention_dropout(0.0, "fp8") == 0.0
    assert load_settings(None, ["attention_dropout=0.1"]).attention_dropout == 0.1
    for bad in (-0.1, 1.0, float("nan"), float("inf"), "0.1", True, None):
        with pytest.raises(ValueError, match="attention_dropout"):
            check_attention_dropout(bad)
    with pytest.raises(ValueError, match="dtype=fp8"):
        load_settings(None, ["attention_dropout=0.1", "dtype=fp8"])


def test_ref_backward_is_autograd_of_ref_forward():
    B, H, Lq, Lk, hd, p = 2, 3, 5, 11, 8, 0.3
    g = torch.Generator().manual_seed(0)
    q, k, v, do = (torch.randn(B, L, H, hd, generator=g, dtype=torch.float64, requires_grad=True)
                   for L in (Lq, Lk, Lk, Lq))
    ks = attn_keep_scale(p, 7, 4096 * 2 + 2049, B, H, Lq, Lk)
    assert ks.shape == (B, H, Lq, Lk) and 0 < int((ks == 0).sum()) < ks.numel() // 2
    kv_len = torch.tensor([Lk, 6], dtype=torch.int32)
    out, probs = _ref_attn_fwd(q, k, v, kv_len, False, 0.5, ks)
    (out * do.detach()).sum().backward()
    with torch.no_grad():
        got = _ref_attn_bwd(q, k, v, probs, do, 0.5, ks)
    for a, b in zip(got, (q.grad, k.grad, v.grad)):
        assert float((a - b).abs().max()) < 1e-12


def test_cpu_model_drops_only_when_asked():
    cfg = model_config("tiny", src_vocab=60, tgt_vocab=50, dropout=0.0)
    m = Transformer(cfg).build("cpu", seed=3)
    g = torch.Generator().manual_seed(1)
    src, tgt = torch.randint(4, 50, (3, 9), generator=g), torch.randint(4, 50, (3, 8), generator=g)

    def run(**kw):
        m.store.zero_grad()  # (the CPU embedding backward adds into its table's gradient)
        out = m.loss_and_backward(src, tgt, RunCtx(training=True, dropout=0.0, seed=5, store=m.store, **kw),
                                  workers=1.0)
        return out.clone(), torch.cat([p.grad.reshape(-1) for p in m.store.params])

    plain, zero, half = run(), run(attn_dropout=0.0), run(attn_dropout=0.5)
    assert torch.equal(plain[0], zero[0]) and torch.equal(plain[1], zero[1])
    assert plain[0][0] != half[0][0] and not torch.equal(plain[1], half[1])
