"""ReLU mask as a bitmap: the bias+ReLU GEMM epilogue writes one bit per
hidden element (bit e of byte c = column 8c + e), the ReLU-backward dgrad
epilogue reads those bits (prefetched before its main loop) instead of the
bf16 activation. Everything here is bitwise: the predicate (stored bf16 > 0)
is the one the bf16-mask epilogue applies."""
import math

import numpy as np
import pytest
import torch

from tensorflow_distributed_on_gke_amd.ops import kernels as kk

pytestmark = pytest.mark.gpu
DEV = "cuda"

FWD_CFGS = [0, 4, 5, 6, 9, 10, 12, 13, 14, 20, 21, 22]
DGRAD_CFGS = [0, 1, 2, 3, 4, 7, 8, 11, 12, 13, 20, 21, 22]


def _randn(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _packbits(mask: torch.Tensor) -> torch.Tensor:
    return torch.from_numpy(np.packbits(mask.cpu().numpy(), axis=1, bitorder="little"))


def _same(a: torch.Tensor, b: torch.Tensor) -> bool:
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


# ------------------------------------------------------------------ producer
_FWD_IN = {}


def _fwd_inputs(M, N, K):
    """N(0, 1) inputs, bias scale 0.5: 40-60 % of the outputs positive.
    Built once per shape."""
    key = (M, N, K)
    if key not in _FWD_IN:
        x = _randn(M, K, seed=11).bfloat16().to(DEV)
        w = _randn(N, K, scale=1.0 / math.sqrt(K), seed=12).bfloat16().to(DEV)
        b = _randn(N, scale=0.5, seed=13).to(DEV)
        _FWD_IN[key] = (x, w, b)
    return _FWD_IN[key]


@pytest.mark.parametrize("cfg", FWD_CFGS)
@pytest.mark.parametrize("shape", [(1000, 776, 512), (200, 264, 64), (256, 256, 192)])
def test_producer_bitmap(shape, cfg):
    """bias+ReLU forward with a bitmap: same bf16 output as without one, the
    bitmap = packbits(out > 0), nothing written outside [M, N / 8] of a wider
    sentinel-filled buffer. (Ragged M, N % 8 == 0 but no tile multiple; one
    tile exactly; one K tile.)"""
    M, N, K = shape
    x, w, b = _fwd_inputs(M, N, K)
    plain = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    kk.gemm(x, w, plain, M, N, K, K, K, N, True, True, kk.EPI_BIAS_RELU, bias=b, cfg=(cfg, 1))
    ldbits = N // 8 + 24
    buf = torch.full((M + 3, ldbits), 0xA5, dtype=torch.uint8, device=DEV)
    bits = buf[:M]
    out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    kk.gemm(x, w, out, M, N, K, K, K, N, True, True, kk.EPI_BIAS_RELU, bias=b, cfg=(cfg, 1),
            relu_bits=bits)
    assert bits.stride(0) == ldbits
    assert _same(out, plain), f"cfg{cfg}: output changed by the bitmap"
    got = buf.cpu()
    want = _packbits(out > 0)
    frac = (out > 0).float().mean().item()
    assert 0.4 < frac < 0.6, frac  # neither polarity can hide a stuck bit
    assert torch.equal(got[:M, :N // 8], want), f"cfg{cfg}: bitmap != packbits(out > 0)"
    assert (got[:M, N // 8:] == 0xA5).all() and (got[M:] == 0xA5).all(), \
        f"cfg{cfg}: bytes outside [M, N/8] written"


@pytest.mark.parametrize("cfg", [12, 4])
def test_degenerate_masks(cfg):
    """Pre-activations exactly 0 -> all bits 0 (a `>=` predicate would set
    them); a large positive bias -> all bits 1."""
    M, N, K = 256, 256, 64
    w = _randn(N, K, scale=0.1, seed=22).bfloat16().to(DEV)
    out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    bits = torch.full((M, N // 8), 0x5A, dtype=torch.uint8, device=DEV)
    x0 = torch.zeros(M, K, dtype=torch.bfloat16, device=DEV)
    kk.linear_fwd(x0, w, torch.zeros(N, device=DEV), relu=True, out=out, relu_bits=bits)
    # (linear_fwd picks its own tile: run the named config explicitly too)
    kk.gemm(x0, w, out, M, N, K, K, K, N, True, True, kk.EPI_BIAS_RELU,
            bias=torch.zeros(N, device=DEV), cfg=(cfg, 1), relu_bits=bits)
    assert (out == 0).all()
    assert (bits == 0).all()
    x = _randn(M, K, seed=21).bfloat16().to(DEV)
    kk.gemm(x, w, out, M, N, K, K, K, N, True, True, kk.EPI_BIAS_RELU,
            bias=torch.full((N,), 100.0, device=DEV), cfg=(cfg, 1), relu_bits=bits)
    assert (out > 0).all()
    assert (bits == 0xFF).all()


def test_producer_refusals():
    """relu_bits needs relu, N % 8 == 0 and no split-K: refused, not ignored."""
    M, N, K = 64, 204, 64
    x = _randn(M, K, seed=1).bfloat16().to(DEV)
    w = _randn(N, K, seed=2).bfloat16().to(DEV)
    b = torch.zeros(N, device=DEV)
    out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    bits = torch.zeros(M, 26, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError):
        kk.gemm(x, w, out, M, N, K, K, K, N, True, True, kk.EPI_BIAS_RELU, bias=b, cfg=(4, 1),
                relu_bits=bits)
    with pytest.raises(ValueError):
        kk.linear_fwd(x, w, b, relu=False, relu_bits=bits)
    N = 256
    w = _randn(N, K, seed=2).bfloat16().to(DEV)
    out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    bits = torch.zeros(M, N // 8, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError):  # split-K
        kk.gemm(x, w, out, M, N, K, K, K, N, True, True, kk.EPI_BIAS_RELU,
                bias=torch.zeros(N, device=DEV), cfg=(0, 2), relu_bits=bits)
    with pytest.raises(RuntimeError):  # one-wave-per-SIMD pipelined tiles: no bitmap path
        kk.gemm(x, w, out, M, N, K, K, K, N, True, True, kk.EPI_BIAS_RELU,
                bias=torch.zeros(N, device=DEV), cfg=(23, 1), relu_bits=bits)


# ------------------------------------------------------------------ consumer
_DG_IN = {}


def _dgrad_inputs(M, N, K):
    key = (M, N, K)
    if key not in _DG_IN:
        dy = _randn(M, K, seed=31).bfloat16().to(DEV)
        w = _randn(K, N, scale=1.0 / math.sqrt(K), seed=32).bfloat16().to(DEV)  # [K, N]: NN operand
        wt = w.t().contiguous()  # [N, K]: NT operand
        h = _randn(M, N, seed=33).bfloat16().to(DEV)
        bits = _packbits(h > 0).to(DEV)
        assert torch.equal(bits, kk.pack_relu_bits(h))
        _DG_IN[key] = (dy, w, wt, h, bits)
    return _DG_IN[key]


@pytest.mark.parametrize("cfg", DGRAD_CFGS)
@pytest.mark.parametrize("layout", ["nn", "nt"])
@pytest.mark.parametrize("shape", [(1000, 1024, 768), (300, 200, 136), (130, 2048, 512),
                                   (256, 256, 64)])
def test_consumer_bits_equal_aux(shape, layout, cfg):
    """ReLU-backward dgrad dx[M, N] = (dy[M, K] @ W) * (h > 0): the mask from
    the bitmap gives bitwise the output of the mask from the bf16 h, in the NN
    layout and in NT against the transposed weight, for every tile config."""
    M, N, K = shape
    dy, w, wt, h, bits = _dgrad_inputs(M, N, K)
    B, ldb, b_kc = (w, N, False) if layout == "nn" else (wt, K, True)
    ref = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    kk.gemm(dy, B, ref, M, N, K, K, ldb, N, True, b_kc, kk.EPI_DRELU, aux=h, ldaux=N, cfg=(cfg, 1))
    out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    kk.gemm(dy, B, out, M, N, K, K, ldb, N, True, b_kc, kk.EPI_DRELU, cfg=(cfg, 1), relu_bits=bits)
    assert _same(out, ref), f"{layout} cfg{cfg}: bitmap mask != bf16 mask"
    # a padded bitmap row stride, unaligned for the wide loads
    wide = torch.zeros(M, N // 8 + 3, dtype=torch.uint8, device=DEV)
    wide[:, :N // 8] = bits
    out.fill_(float("nan"))
    kk.gemm(dy, B, out, M, N, K, K, ldb, N, True, b_kc, kk.EPI_DRELU, cfg=(cfg, 1),
            relu_bits=wide[:, :N // 8])
    assert _same(out, ref), f"{layout} cfg{cfg}: strided bitmap"


def test_consumer_beta_and_wrappers():
    """linear_dgrad / linear_dgrad_t with relu_bits equal relu_aux, also with
    the beta = 1 accumulation."""
    M, N, K = 300, 200, 136
    dy, w, wt, h, bits = _dgrad_inputs(M, N, K)
    assert _same(kk.linear_dgrad(dy, w, K, relu_bits=bits), kk.linear_dgrad(dy, w, K, relu_aux=h))
    assert _same(kk.linear_dgrad_t(dy, wt, relu_bits=bits), kk.linear_dgrad_t(dy, wt, relu_aux=h))
    c0 = _randn(M, N, seed=34).bfloat16().to(DEV)
    a, b = c0.clone(), c0.clone()
    kk.linear_dgrad(dy, w, K, relu_aux=h, out=a, beta=1.0)
    kk.linear_dgrad(dy, w, K, relu_bits=bits, out=b, beta=1.0)
    assert _same(a, b)


def test_consumer_refuses_n_not_multiple_of_8():
    """N % 8 != 0 has no bitmap: the launch is refused (the caller keeps the
    bf16 mask for such shapes), never run with a wrong mask."""
    M, N, K = 64, 204, 64
    dy = _randn(M, K, seed=41).bfloat16().to(DEV)
    w = _randn(K, N, seed=42).bfloat16().to(DEV)
    wp = torch.zeros(K, 208, dtype=torch.bfloat16, device=DEV)  # ldb a multiple of 8
    wp[:, :N] = w
    bits = torch.zeros(M, 26, dtype=torch.uint8, device=DEV)
    out = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError):
        kk.gemm(dy, wp, out, M, N, K, K, 208, N, True, False, kk.EPI_DRELU, cfg=(4, 1),
                relu_bits=bits)
    assert (out == 0).all()
    # the bf16 mask path still takes the shape
    h = _randn(M, N, seed=43).bfloat16().to(DEV)
    kk.gemm(dy, wp, out, M, N, K, K, 208, N, True, False, kk.EPI_DRELU, aux=h, ldaux=N, cfg=(4, 1))
    ref = (dy.float() @ w.float()) * (h > 0)
    assert ((out.float() - ref).abs().max() / ref.abs().max()).item() < 1e-2


# ------------------------------------------------------------------ block level
def _ffn_block(d, ff, graph):
    """dx and the FFN parameter gradients of one FFNBlockFn forward + backward
    (B = 2, L = 128), bitmap on or off by the module switch."""
    from tensorflow_distributed_on_gke_amd.models import layers
    from tensorflow_distributed_on_gke_amd.models.layers import FFNBlockFn, RunCtx
    from tensorflow_distributed_on_gke_amd.models.transformer import Transformer, model_config

    cfg = model_config("tiny", layers=1, d_model=d, heads=8, d_ff=ff, src_vocab=64, tgt_vocab=64,
                       dropout=0.1)
    m = Transformer(cfg).build(DEV, seed=5)
    lay = m.enc_layers[0]
    ps = (lay.ff1.w, lay.ff1.b, lay.ff2.w, lay.ff2.b, lay.ln2.gamma, lay.ln2.beta)
    x = _randn(2, 128, d, seed=51).bfloat16().to(DEV)
    dy = _randn(2, 128, d, seed=52).bfloat16().to(DEV)
    ctr = torch.tensor([3], dtype=torch.int64, device=DEV)
    res = {}
    old = layers.RELU_BITS
    try:
        for on in (True, False):
            layers.RELU_BITS = on
            dx = torch.empty_like(x)

            def run():
                rt = RunCtx(training=True, dropout=0.1, seed=7, ctr=ctr, store=None)
                xin = x.clone().requires_grad_(True)
                y = FFNBlockFn.apply(xin, *ps, lay.site2, rt)
                y.backward(dy)
                dx.copy_(xin.grad)

            for p in ps:
                p.grad.fill_(float("nan"))
            run()  # eager (also the warm-up of the capture below)
            if graph:
                torch.cuda.synchronize()
                for p in ps:
                    p.grad.fill_(float("nan"))
                dx.fill_(float("nan"))
                g = torch.cuda.CUDAGraph()
                s = torch.cuda.Stream()
                s.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s):
                    with torch.cuda.graph(g, stream=s):
                        run()
                torch.cuda.current_stream().wait_stream(s)
                g.replay()
            torch.cuda.synchronize()
            res[on] = [dx.clone()] + [p.grad.clone() for p in ps]
            assert all(torch.isfinite(t.float()).all() for t in res[on])
    finally:
        layers.RELU_BITS = old
    return res


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("d,ff", [(128, 256), (512, 2048)])
def test_ffn_block_bitwise(d, ff, graph):
    """FFNBlockFn with TDG_RELU_BITS on and off (module switch, one process):
    dx and every parameter gradient bitwise equal, eager and in a captured and
    replayed graph. (d = 128 is the narrowest LayerNorm the block has a kernel
    for; the FFN GEMMs at d = 64 -- 256 x 256 x 64 -- are the (256, 256, 64)
    cases of the producer / consumer tests above.)"""
    res = _ffn_block(d, ff, graph)
    names = ["dx", "w1", "b1", "w2", "b2", "gamma", "beta"]
    for n, a, b in zip(names, res[True], res[False]):
        assert torch.equal(a, b), f"{n} differs between the bitmap and the bf16 mask"
