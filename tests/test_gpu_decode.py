"""The decoding kernels (csrc/kernels/decode.hip) against the float64
references of ref_decode.py, their bindings' validation, and beam search end
to end on the GPU."""
import pytest
import torch

import ref_decode as rd
from tensorflow_distributed_on_gke_amd.infer.beam import beam_search
from tensorflow_distributed_on_gke_amd.infer.greedy import Tester
from tensorflow_distributed_on_gke_amd.infer.tokenizer import END, START, ByteTokenizer
from tensorflow_distributed_on_gke_amd.models.transformer import Transformer, model_config
from tensorflow_distributed_on_gke_amd.ops import kernels as K
from tensorflow_distributed_on_gke_amd.ops._ext import C

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(x):
    return None if x is None else x.to(DEV)


def _view_to_dev(c):
    """k / v of a case on the GPU with the strides they have on the CPU."""
    if c.get("row_map") is None:
        return c["k"].to(DEV), c["v"].to(DEV)
    H, hd = c["q"].shape[1:]
    d = H * hd
    big = c["k"]._base.to(DEV)  # the [B, S, 4 d] tensor both are slices of
    return big[:, :, d:2 * d].unflatten(-1, (H, hd)), big[:, :, 3 * d:].unflatten(-1, (H, hd))


# ---------------------------------------------------------------- decode_attn
@pytest.mark.parametrize("hd,H,R,Lk", rd.ATTN_SHAPES)
def test_decode_attn(hd, H, R, Lk):
    for variant in rd.ATTN_VARIANTS:
        c = rd.attn_case(hd, H, R, Lk, variant)
        ref = rd.attn_ref(c)
        k, v = _view_to_dev(c)
        assert k.stride() == c["k"].stride() and bool(torch.isnan(k).any()) == bool(torch.isnan(c["k"]).any())
        out = K.decode_attn(c["q"].to(DEV), k, v, c["kv_len"].to(DEV), c["scale"], anc=_dev(c["anc"]),
                            row_map=_dev(c["row_map"]))
        out = out.cpu().double()
        assert out.shape == (R, H, hd)
        assert torch.isfinite(out).all(), f"{variant}: an unused (NaN) key reached the output"
        err, bound = (out - ref).abs(), rd.attn_bound(ref, c["vmax"])
        worst = (err - bound).max().item()
        print(f"{variant}: max err {err.max().item():.3e}, worst err - bound {worst:.3e}")
        assert worst <= 0, f"{variant}: error exceeds the bound by {worst:.3e}"


@pytest.mark.parametrize("hd,H,R,Lk", rd.ATTN_SHAPES)
def test_decode_attn_fused_append(hd, H, R, Lk):
    for with_anc in (False, True):
        c = rd.fused_case(hd, H, R, Lk, with_anc)
        q, kv_len, anc = c["q"].to(DEV), c["kv_len"].to(DEV), _dev(c["anc"])
        plain = K.decode_attn(q, c["k_ready"].to(DEV), c["v_ready"].to(DEV), kv_len, c["scale"], anc=anc)
        k, v = c["k"].to(DEV), c["v"].to(DEV)
        fused = K.decode_attn(q, k, v, kv_len, c["scale"], anc=anc, k_new=c["k_new"].to(DEV),
                              v_new=c["v_new"].to(DEV))
        assert torch.equal(fused.view(torch.int16), plain.view(torch.int16))
        # k_new / v_new at [r, t], the sentinel everywhere beyond, the rest as it was
        assert torch.equal(k.cpu().view(torch.int16), c["k_ready"].view(torch.int16))
        assert torch.equal(v.cpu().view(torch.int16), c["v_ready"].view(torch.int16))


# ---------------------------------------------------------------- beam_topk
@pytest.mark.parametrize("V,ldl,beam,B", rd.TOPK_SHAPES)
def test_beam_topk(V, ldl, beam, B):
    for kind in rd.TOPK_KINDS:
        c = rd.topk_case(V, ldl, beam, B, kind)
        r_score, r_parent, r_token, r_fin, vals = c["ref"]
        assert rd.gaps_ok(vals, kind == "ties"), kind
        score, parent, token, fin, _ = K.beam_topk(c["logits"].to(DEV), V, c["score"].to(DEV),
                                                   c["fin"].to(DEV), beam, rd.END, rd.PAD)
        score, parent, token, fin = score.cpu(), parent.cpu(), token.cpu(), fin.cpu()
        assert not torch.isnan(score).any(), kind
        assert torch.equal(token.long(), r_token) and torch.equal(parent.long(), r_parent), kind
        assert torch.equal(fin.long(), r_fin), kind
        dead = r_score == float("-inf")
        assert torch.equal(score == float("-inf"), dead), kind
        err = (score.double() - r_score)[~dead].abs()
        print(f"{kind}: max score err {err.max().item() if err.numel() else 0.0:.3e}")
        assert (err <= 1e-4 * r_score[~dead].abs().clamp(min=1.0)).all(), kind


def test_beam_topk_ancestry():
    V, ldl, beam, B = 300, 304, 4, 3
    c = rd.topk_case(V, ldl, beam, B, "random")
    R, t = B * beam, 5
    g = torch.Generator().manual_seed(0)
    anc = torch.randint(R, (R, 9), generator=g).to(torch.int32)
    out = torch.full((R, 9), -1, dtype=torch.int32, device=DEV)
    _, parent, _, _, new = K.beam_topk(c["logits"].to(DEV), V, c["score"].to(DEV), c["fin"].to(DEV), beam,
                                       rd.END, rd.PAD, anc=anc.to(DEV), t=t, anc_out=out)
    parent, new = parent.cpu().long(), new.cpu()
    assert torch.equal(parent, c["ref"][1])
    assert torch.equal(new[:, : t + 1], anc[parent, : t + 1])
    assert torch.equal(new[:, t + 1], torch.arange(R, dtype=torch.int32))
    assert (new[:, t + 2:] == -1).all()  # nothing written past column t + 1


# ---------------------------------------------------------------- bindings
SENT = 7.0


def _attn_ops(hd=64):
    g = torch.Generator().manual_seed(0)
    R, H, L = 2, 1, 16
    q = torch.randn(R, H, hd, generator=g).to(torch.bfloat16).to(DEV)
    k = torch.randn(R, L, H, hd, generator=g).to(torch.bfloat16).to(DEV)
    v = torch.randn(R, L, H, hd, generator=g).to(torch.bfloat16).to(DEV)
    out = torch.full((R, H, hd), SENT, dtype=torch.bfloat16, device=DEV)
    kv_len = torch.full((R,), L, dtype=torch.int32, device=DEV)
    return q, k, v, out, kv_len


def _untouched(*tensors):
    torch.cuda.synchronize()
    for t in tensors:
        assert (t.float() == SENT).all().item(), "a rejected call wrote to its output"


def test_decode_attn_well_formed():
    q, k, v, out, kv_len = _attn_ops()
    C().decode_attn(q, k, v, out, kv_len, 0.125)
    s = torch.einsum("rhd,rkhd->rhk", q.double(), k.double()) * 0.125
    ref = torch.einsum("rhk,rkhd->rhd", torch.softmax(s, -1), v.double()).cpu()
    assert ((out.cpu().double() - ref).abs() <= rd.attn_bound(ref, float(v.float().abs().max()))).all()


def test_decode_attn_misaligned_q():
    q, k, v, out, kv_len = _attn_ops()
    flat = torch.zeros(q.numel() + 8, dtype=torch.bfloat16, device=DEV)
    q1 = flat[1:1 + q.numel()].view(q.shape)  # 2 bytes off a 16-byte boundary
    q1.copy_(q)
    with pytest.raises(RuntimeError):
        C().decode_attn(q1, k, v, out, kv_len, 0.125)
    _untouched(out)


def test_decode_attn_int64_kv_len():
    q, k, v, out, kv_len = _attn_ops()
    with pytest.raises(RuntimeError):
        C().decode_attn(q, k, v, out, kv_len.long(), 0.125)
    _untouched(out)


def test_decode_attn_hd32():
    q, k, v, out, kv_len = _attn_ops(hd=32)
    with pytest.raises(RuntimeError):
        C().decode_attn(q, k, v, out, kv_len, 0.125)
    _untouched(out)


def test_decode_attn_short_kv_len_and_cache():
    q, k, v, out, kv_len = _attn_ops()
    with pytest.raises(RuntimeError):
        C().decode_attn(q, k, v, out, kv_len[:1], 0.125)
    with pytest.raises(RuntimeError):  # one cache row for two query rows, no row_map
        C().decode_attn(q, k[:1], v[:1], out, kv_len, 0.125)
    with pytest.raises(RuntimeError):  # float k
        C().decode_attn(q, k.float(), v, out, kv_len, 0.125)
    _untouched(out)


def test_beam_topk_beam9_and_dtypes():
    R, V = 9, 16
    logits = torch.zeros(R, V, dtype=torch.bfloat16, device=DEV)
    score = torch.zeros(R, dtype=torch.float32, device=DEV)
    fin = torch.zeros(R, dtype=torch.int32, device=DEV)
    outs = [torch.full((R,), SENT, dtype=torch.float32, device=DEV)] + \
        [torch.full((R,), int(SENT), dtype=torch.int32, device=DEV) for _ in range(3)]
    with pytest.raises(RuntimeError):
        C().beam_topk(logits, V, score, fin, 9, 3, 0, *outs)
    with pytest.raises(RuntimeError):  # int64 fin
        C().beam_topk(logits, V, score, fin.long(), 3, 3, 0, *outs)
    with pytest.raises(RuntimeError):  # f32 logits
        C().beam_topk(logits.float(), V, score, fin, 3, 3, 0, *outs)
    with pytest.raises(RuntimeError):  # too-short score
        C().beam_topk(logits, V, score[:8], fin, 3, 3, 0, *outs)
    _untouched(*outs)
    C().beam_topk(logits, V, score, fin, 3, 3, 0, *outs)  # the same call well-formed
    torch.cuda.synchronize()
    assert outs[2].tolist() == [0, 1, 2] * 3  # all candidates tie: the lowest flat indices


# ---------------------------------------------------------------- end to end
SENTS = ["muitas pessoas vieram à estação.", "olá", "este é um teste mais longo"]


@pytest.fixture(scope="module")
def gpu_model():
    m = Transformer(model_config("tiny", src_vocab=300, tgt_vocab=300)).build("cuda:0", seed=4)
    tester = Tester(ByteTokenizer(300), m)
    return m, tester, tester.src_tok.tokenize(SENTS)


def test_copy_equals_index_and_deterministic(gpu_model):
    m, _, src = gpu_model
    a = beam_search(m, src, START, END, beam=4, max_length=12, reorder="index")
    b = beam_search(m, src, START, END, beam=4, max_length=12, reorder="index")
    c = beam_search(m, src, START, END, beam=4, max_length=12, reorder="copy")
    assert a[0].shape[0] == 3 and a[0].shape[1] <= 13 and bool((a[0][:, 0] == START).all())
    assert torch.isfinite(a[1]).all()
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y), "two beam-4 runs differ"
        assert torch.equal(x, z), "reorder='copy' differs from 'index'"


def test_beam1_vs_greedy_cached(gpu_model):
    m, tester, src = gpu_model
    greedy = tester.greedy_cached(src, max_length=12).cpu()
    tokens = beam_search(m, src, START, END, beam=1, max_length=12, alpha=0.0)[0].cpu()
    n = min(greedy.shape[1], tokens.shape[1])
    gen = greedy[:, 1:n]
    live = torch.ones_like(gen, dtype=torch.bool)
    for b in range(gen.shape[0]):
        row = gen[b].tolist()
        if END in row:
            live[b, row.index(END) + 1:] = False
    # argmax flips between differently shaped bf16 computations (test_tester.py)
    frac = (tokens[:, 1:n][live] != gen[live]).float().mean().item()
    print(f"beam 1 vs greedy_cached: {frac:.3f} of live tokens differ")
    assert frac <= 0.1
