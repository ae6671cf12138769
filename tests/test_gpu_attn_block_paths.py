"""Which kernels an attention block runs, per configuration: the sequence of
`ops.kernels` launch wrappers one `loss_and_backward` goes through (forward,
backward, deferred weight gradients) is pinned as a literal list per case, and
the result is bitwise reproducible, so two trees that record the same sequence
can be compared with `torch.equal`.

The lists were recorded on the tree before the self- and cross-attention
blocks shared one core (models/layers.py `_attn_block_fwd` / `_attn_block_bwd`)
and hold unchanged on it.

Cases (tiny preset; 2 heads = head dim 64 unless stated): batch 2 for the bf16
cases. The lean fp8 blocks need a token count that is a multiple of 128
(`fp8.wgrad_fp8_ok`), which batch 2 cannot give at these lengths, so the
`Fp8State` cases use batch 8 as `test_fp8_attention_backward_grads_match_bf16_backward`
does; `fp8_batch2` keeps the batch-2 form, where the e4m3 forward runs around
bf16 (not lean) projections and backward."""
import pytest
import torch

from tensorflow_distributed_on_gke_amd.models.layers import RunCtx, WgradQueue
from tensorflow_distributed_on_gke_amd.models.transformer import Transformer, model_config
from tensorflow_distributed_on_gke_amd.ops import fp8 as F
from tensorflow_distributed_on_gke_amd.ops import kernels as kk

pytestmark = pytest.mark.gpu

RECORDED = ("attn_", "qkv_attn", "linear_", "ln_", "wgrad_", "embed_")
V = 64

# src / tgt: padded lengths (the decoder sees tgt - 1); heads None: the preset's 8 (head dim 16);
# off: ops.fp8 switches turned off; maps: inference forward with the attention-map probe
CASES = {
    # <= 128 tokens: fused projection + attention forward, fused-dO backward, on every block
    "bf16_short": dict(src=40, tgt=33, dropout=0.1),
    # past the 128-token fused kernels: projection GEMM + attn_fwd, linear_dgrad + attn_bwd
    "bf16_long": dict(src=160, tgt=161, dropout=0.1),
    # head dim 16: the fused paths decline on hd
    "bf16_hd16": dict(src=40, tgt=33, dropout=0.1, heads=None),
    # the maps force the unfused forward; attn_probs per block
    "bf16_maps": dict(src=40, tgt=33, maps=True),
    # attn_fwd_fp8 + attn_bwd_f8 on self and cross blocks, e5m2 d(K|V) straight to kvh.buf8
    "fp8_f8": dict(src=160, tgt=161, fp8=True, batch=8),
    "fp8_g8": dict(src=160, tgt=161, fp8=True, batch=8, off=("ATTN_BWD_F8",)),
    "fp8_bf16_bwd": dict(src=160, tgt=161, fp8=True, batch=8, off=("ATTN_BWD_F8", "ATTN_BWD_G8")),
    # encoder self-attention inside the fp8 backward's range, cross-attention (Lq 32) not:
    # kvh.f8b false, bf16 d(K|V)
    "fp8_mixed": dict(src=160, tgt=33, fp8=True, batch=8),
    # short sequences under fp8: lean projections around the bf16 attention kernels
    "fp8_short": dict(src=40, tgt=33, fp8=True, batch=8),
    "fp8_batch2": dict(src=160, tgt=161, fp8=True),
}

# one line per layer: the encoder layers, the batched cross K|V projection and the decoder
# embedding, the decoder layers, the loss head, then the backward in reverse
_BF16_LONG = (
    "embed_csr_sort embed_fwd "
    "qkv_attn_fwd linear_fwd attn_fwd linear_fwd ln_fwd linear_fwd linear_fwd ln_fwd "
    "qkv_attn_fwd linear_fwd attn_fwd linear_fwd ln_fwd linear_fwd linear_fwd ln_fwd "
    "linear_fwd embed_fwd "
    "qkv_attn_fwd linear_fwd attn_fwd linear_fwd ln_fwd qkv_attn_fwd linear_fwd attn_fwd linear_fwd ln_fwd "
    "linear_fwd linear_fwd ln_fwd "
    "qkv_attn_fwd linear_fwd attn_fwd linear_fwd ln_fwd qkv_attn_fwd linear_fwd attn_fwd linear_fwd ln_fwd "
    "linear_fwd linear_fwd ln_fwd "
    "linear_fwd linear_wgrad linear_dgrad "
    "ln_bwd linear_wgrad linear_dgrad linear_wgrad linear_dgrad "
    "ln_bwd linear_wgrad attn_bwd_fdo linear_dgrad attn_bwd linear_wgrad linear_dgrad "
    "ln_bwd linear_wgrad attn_bwd_fdo linear_dgrad attn_bwd linear_wgrad linear_dgrad "
    "ln_bwd linear_wgrad linear_dgrad linear_wgrad linear_dgrad "
    "ln_bwd linear_wgrad attn_bwd_fdo linear_dgrad attn_bwd linear_wgrad linear_dgrad "
    "ln_bwd linear_wgrad attn_bwd_fdo linear_dgrad attn_bwd linear_wgrad linear_dgrad "
    "embed_bwd linear_wgrad linear_dgrad "
    "ln_bwd linear_wgrad linear_dgrad linear_wgrad linear_dgrad "
    "ln_bwd linear_wgrad attn_bwd_fdo linear_dgrad attn_bwd linear_wgrad linear_dgrad "
    "ln_bwd linear_wgrad linear_dgrad linear_wgrad linear_dgrad "
    "ln_bwd linear_wgrad attn_bwd_fdo linear_dgrad attn_bwd linear_wgrad linear_dgrad "
    "embed_bwd")

EXPECTED = {
    "bf16_short": (
        "embed_csr_sort embed_fwd "
        "qkv_attn_fwd linear_fwd ln_fwd linear_fwd linear_fwd ln_fwd "
        "qkv_attn_fwd linear_fwd ln_fwd linear_fwd linear_fwd ln_fwd "
        "linear_fwd embed_fwd "
        "qkv_attn_fwd linear_fwd ln_fwd qkv_attn_fwd linear_fwd ln_fwd linear_fwd linear_fwd ln_fwd "
        "qkv_attn_fwd linear_fwd ln_fwd qkv_attn_fwd linear_fwd ln_fwd linear_fwd linear_fwd ln_fwd "
        "linear_fwd linear_wgrad linear_dgrad "
        "ln_bwd linear_wgrad linear_dgrad linear_wgrad linear_dgrad "
        "ln_bwd linear_wgrad attn_bwd_fdo linear_wgrad linear_dgrad "
        "ln_bwd linear_wgrad attn_bwd_fdo linear_wgrad linear_dgrad "
        "ln_bwd linear_wgrad linear_dgrad linear_wgrad linear_dgrad "
        "ln_bwd linear_wgrad attn_bwd_fdo linear_wgrad linear_dgrad "
        "ln_bwd linear_wgrad attn_bwd_fdo linear_wgrad linear_dgrad "
        "embed_bwd linear_wgrad linear_dgrad "
        "ln_bwd linear_wgrad linear_dgrad linear_wgrad linear_dgrad "
        "ln_bwd linear_wgrad attn_bwd_fdo linear_wgrad linear_dgrad "
        "ln_bwd linear_wgrad linear_dgrad linear_wgrad linear_dgrad "
        "ln_bwd linear_wgrad attn_bwd_fdo linear_wgrad linear_dgrad "
        "embed_bwd"),
    # (qkv_attn_fwd and attn_bwd_fdo are asked and decline: nothing launched)
    "bf16_long": _BF16_LONG,
    "bf16_hd16": _BF16_LONG,
    "bf16_maps": (
        "embed_fwd "
        "linear_fwd attn_fwd attn_probs linear_fwd ln_fwd linear_fwd linear_fwd ln_fwd "
        "linear_fwd attn_fwd attn_probs linear_fwd ln_fwd linear_fwd linear_fwd ln_fwd "
        "linear_fwd embed_fwd "
        "linear_fwd attn_fwd attn_probs linear_fwd ln_fwd linear_fwd attn_fwd attn_probs linear_fwd ln_fwd "
        "linear_fwd linear_fwd ln_fwd "
        "linear_fwd attn_fwd attn_probs linear_fwd ln_fwd linear_fwd attn_fwd attn_probs linear_fwd ln_fwd "
        "linear_fwd linear_fwd ln_fwd"),
    # (the fp8 GEMMs are ops.fp8's, not recorded; the weight gradients one ragged launch)
    "fp8_f8": (
        "embed_csr_sort embed_fwd "
        "attn_fwd_fp8 ln_fwd ln_fwd "
        "attn_fwd_fp8 ln_fwd ln_fwd "
        "embed_fwd "
        "attn_fwd_fp8 ln_fwd attn_fwd_fp8 ln_fwd ln_fwd "
        "attn_fwd_fp8 ln_fwd attn_fwd_fp8 ln_fwd ln_fwd "
        "linear_fwd linear_dgrad "
        "ln_bwd ln_bwd attn_bwd_f8 ln_bwd attn_bwd_f8 "
        "ln_bwd ln_bwd attn_bwd_f8 ln_bwd attn_bwd_f8 "
        "embed_bwd "
        "ln_bwd ln_bwd attn_bwd_f8 "
        "ln_bwd ln_bwd attn_bwd_f8 "
        "embed_bwd wgrad_ragged"),
    "fp8_g8": (
        "embed_csr_sort embed_fwd "
        "attn_fwd_fp8 ln_fwd ln_fwd "
        "attn_fwd_fp8 ln_fwd ln_fwd "
        "embed_fwd "
        "attn_fwd_fp8 ln_fwd attn_fwd_fp8 ln_fwd ln_fwd "
        "attn_fwd_fp8 ln_fwd attn_fwd_fp8 ln_fwd ln_fwd "
        "linear_fwd linear_dgrad "
        "ln_bwd ln_bwd attn_bwd_g8 ln_bwd attn_bwd_g8 "
        "ln_bwd ln_bwd attn_bwd_g8 ln_bwd attn_bwd_g8 "
        "embed_bwd "
        "ln_bwd ln_bwd attn_bwd_g8 "
        "ln_bwd ln_bwd attn_bwd_g8 "
        "embed_bwd wgrad_ragged"),
    "fp8_bf16_bwd": (
        "embed_csr_sort embed_fwd "
        "attn_fwd_fp8 ln_fwd ln_fwd "
        "attn_fwd_fp8 ln_fwd ln_fwd "
        "embed_fwd "
        "attn_fwd_fp8 ln_fwd attn_fwd_fp8 ln_fwd ln_fwd "
        "attn_fwd_fp8 ln_fwd attn_fwd_fp8 ln_fwd ln_fwd "
        "linear_fwd linear_dgrad "
        "ln_bwd ln_bwd attn_bwd ln_bwd attn_bwd "
        "ln_bwd ln_bwd attn_bwd ln_bwd attn_bwd "
        "embed_bwd "
        "ln_bwd ln_bwd attn_bwd "
        "ln_bwd ln_bwd attn_bwd "
        "embed_bwd wgrad_ragged"),
    # (cross-attention, Lq 32 / Lk 160: the e5m2-emitting backward; decoder self-attention bf16)
    "fp8_mixed": (
        "embed_csr_sort embed_fwd "
        "attn_fwd_fp8 ln_fwd ln_fwd "
        "attn_fwd_fp8 ln_fwd ln_fwd "
        "embed_fwd "
        "attn_fwd ln_fwd attn_fwd ln_fwd ln_fwd "
        "attn_fwd ln_fwd attn_fwd ln_fwd ln_fwd "
        "linear_fwd linear_dgrad "
        "ln_bwd ln_bwd attn_bwd_g8 ln_bwd attn_bwd "
        "ln_bwd ln_bwd attn_bwd_g8 ln_bwd attn_bwd "
        "embed_bwd "
        "ln_bwd ln_bwd attn_bwd_f8 "
        "ln_bwd ln_bwd attn_bwd_f8 "
        "embed_bwd wgrad_ragged"),
    # (8 x 40 encoder tokens are no multiple of 128: the encoder blocks and the cross K|V
    # projection are not lean, the decoder's, 8 x 32 tokens, are)
    "fp8_short": (
        "embed_csr_sort embed_fwd "
        "attn_fwd linear_fwd ln_fwd ln_fwd "
        "attn_fwd linear_fwd ln_fwd ln_fwd "
        "embed_fwd "
        "attn_fwd ln_fwd attn_fwd ln_fwd ln_fwd "
        "attn_fwd ln_fwd attn_fwd ln_fwd ln_fwd "
        "linear_fwd linear_dgrad "
        "ln_bwd ln_bwd attn_bwd ln_bwd attn_bwd "
        "ln_bwd ln_bwd attn_bwd ln_bwd attn_bwd "
        "embed_bwd linear_dgrad "
        "ln_bwd ln_bwd attn_bwd_fdo linear_dgrad "
        "ln_bwd ln_bwd attn_bwd_fdo linear_dgrad "
        "embed_bwd wgrad_ragged wgrad_ragged"),
    "fp8_batch2": (
        "embed_csr_sort embed_fwd "
        "attn_fwd_fp8 linear_fwd ln_fwd ln_fwd "
        "attn_fwd_fp8 linear_fwd ln_fwd ln_fwd "
        "embed_fwd "
        "attn_fwd_fp8 linear_fwd ln_fwd attn_fwd_fp8 linear_fwd ln_fwd ln_fwd "
        "attn_fwd_fp8 linear_fwd ln_fwd attn_fwd_fp8 linear_fwd ln_fwd ln_fwd "
        "linear_fwd linear_dgrad "
        "ln_bwd ln_bwd attn_bwd_fdo linear_dgrad attn_bwd linear_dgrad "
        "ln_bwd attn_bwd_fdo linear_dgrad attn_bwd linear_dgrad "
        "ln_bwd ln_bwd attn_bwd_fdo linear_dgrad attn_bwd linear_dgrad "
        "ln_bwd attn_bwd_fdo linear_dgrad attn_bwd linear_dgrad "
        "embed_bwd linear_dgrad "
        "ln_bwd ln_bwd attn_bwd_fdo linear_dgrad attn_bwd linear_dgrad "
        "ln_bwd ln_bwd attn_bwd_fdo linear_dgrad attn_bwd linear_dgrad "
        "embed_bwd wgrad_ragged"),
}


def _batch(B, S, T, seed):
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(4, V, (B, S), generator=g)
    tgt = torch.randint(4, V, (B, T), generator=g)
    for b in range(1, B):  # (row 0 keeps the full length)
        src[b, int(torch.randint(S // 2, S + 1, (1,), generator=g)):] = 0
        tgt[b, int(torch.randint(T // 2, T + 1, (1,), generator=g)):] = 0
    return src.cuda(), tgt.cuda()


def record_kernels(setattr_):
    """Wrap the launch wrappers of the ops.kernels package (the names models/ reaches as
    K.<name>; not the `_ok` predicates, which launch nothing) with a recorder; returns the
    list the names are appended to. setattr_: monkeypatch.setattr."""
    calls = []

    def wrap(name, fn):
        def rec(*a, **k):
            calls.append(name)
            return fn(*a, **k)
        return rec

    for name in sorted(vars(kk)):
        fn = getattr(kk, name)
        if name.startswith(RECORDED) and callable(fn) and not name.endswith("_ok"):
            setattr_(kk, name, wrap(name, fn))
    return calls


def run_case(name, calls=None):
    """One case on a fresh model -> (loss/accuracy tensor or the decoder features, flat
    gradient or the attention maps); `calls` is cleared before the step that counts."""
    c = CASES[name]
    p = c.get("dropout", 0.0)
    heads = c.get("heads", 2)
    cfg = model_config("tiny", heads=heads, src_vocab=V, tgt_vocab=V, dropout=p)
    src, tgt = _batch(c.get("batch", 2), c["src"], c["tgt"], seed=7)
    old = {s: getattr(F, s) for s in c.get("off", ())}
    try:
        for s in old:
            setattr(F, s, False)
        m = Transformer(cfg).build("cuda", seed=1)
        ctr = torch.tensor([4], dtype=torch.int64, device="cuda")
        if c.get("maps"):
            rt = RunCtx(training=False, store=None, attn_maps={})
            if calls is not None:
                calls.clear()
            with torch.no_grad():
                dec = m.features(src, tgt[:, :-1].contiguous(), rt)
            torch.cuda.synchronize()
            return dec.clone(), torch.cat([rt.attn_maps[k].reshape(-1) for k in sorted(rt.attn_maps)])
        st = F.Fp8State(m) if c.get("fp8") else None
        rt = RunCtx(training=True, dropout=p, seed=3, store=m.store, fp8=st, ctr=ctr)
        if st is not None:
            rt.wgrad = WgradQueue()
            rt.wgrad.layers_per_step = 2 * cfg.layers
        # fp8: the second step runs on calibrated delayed scales (dO, dS, gradients)
        for _ in range(2 if st is not None else 1):
            m.store.zero_grad()
            if calls is not None:
                calls.clear()
            out = m.loss_and_backward(src, tgt, rt, 1.0)
            if st is not None:
                st.after_step()
        torch.cuda.synchronize()
        return out.clone(), m.store.flat_grad.clone()
    finally:
        for s, v in old.items():
            setattr(F, s, v)


_RESULTS = {}


@pytest.mark.parametrize("name", list(CASES))
def test_attention_block_kernel_sequence(name, monkeypatch):
    calls = record_kernels(monkeypatch.setattr)
    _RESULTS[name] = run_case(name, calls)
    print(name, " ".join(calls))
    assert calls == EXPECTED[name].split()


@pytest.mark.parametrize("name", ["bf16_short", "bf16_long", "fp8_f8", "fp8_mixed"])
def test_attention_block_step_is_bitwise_reproducible(name):
    """Same weights, batch, seed and counter -> the same loss and flat gradient, bit for bit
    (what makes a torch.equal comparison between two trees meaningful)."""
    a = _RESULTS.get(name) or run_case(name)
    b = run_case(name)
    assert torch.isfinite(a[1]).all()
    assert torch.equal(a[0], b[0])
    assert torch.equal(a[1], b[1])
