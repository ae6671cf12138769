"""The wide beam selection (csrc/kernels/beam_wide.hip): the narrow kernel's bits where both run, the
float64 reference of ref_decode.py above width 8, the binding's validation, beam search at width 16."""
import itertools

import pytest
import torch

import ref_decode as rd
from tensorflow_distributed_on_gke_amd.infer.beam import beam_search
from tensorflow_distributed_on_gke_amd.infer.tokenizer import END, START, ByteTokenizer
from tensorflow_distributed_on_gke_amd.models.transformer import Transformer, model_config
from tensorflow_distributed_on_gke_amd.ops import kernels as K
from tensorflow_distributed_on_gke_amd.ops._ext import C

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 7
NINF = float("-inf")


def _outs(R):
    return [torch.full((R,), float(SENT), dtype=torch.float32, device=DEV)] + \
        [torch.full((R,), SENT, dtype=torch.int32, device=DEV) for _ in range(3)]


def _ws(R, beam):
    return torch.full(((2 * beam + 1) * R,), SENT, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("V,ldl,beam,B", rd.TOPK_SHAPES)
def test_wide_equals_narrow_bitwise(V, ldl, beam, B):
    R, t = B * beam, 5
    anc = torch.randint(R, (R, 9), generator=torch.Generator().manual_seed(0)).to(torch.int32).to(DEV)
    for kind in rd.TOPK_KINDS:
        c = rd.topk_case(V, ldl, beam, B, kind)
        ops = (c["logits"].to(DEV), V, c["score"].to(DEV), c["fin"].to(DEV), beam, rd.END, rd.PAD)
        narrow, wide = _outs(R), _outs(R)
        a_n, a_w = (torch.full((R, 9), -1, dtype=torch.int32, device=DEV) for _ in range(2))
        C().beam_topk(*ops, *narrow, anc, a_n, t)
        C().beam_topk_wide(*ops, *wide, _ws(R, beam), anc, a_w, t)
        assert torch.equal(narrow[0].view(torch.int32), wide[0].view(torch.int32)), kind
        for n, w in zip(narrow[1:] + [a_n], wide[1:] + [a_w]):
            assert torch.equal(n, w), kind
        assert (a_w[:, t + 2:] == -1).all(), kind  # nothing written past column t + 1


_WIDTHS, _ALL = (9, 16, 33, 64), rd.TOPK_KINDS
_NO_INITIAL = ("random", "all_finished", "ties")
WIDE_CASES = list(dict.fromkeys(
    [(V, l, beam, B, k) for (V, l), beam, B, k in itertools.product(
        ((7, 8), (300, 304), (7010, 7040)), _WIDTHS, (1, 3), ("ties",))] +
    [(7, 8, beam, B, k) for beam, B, k in itertools.product(_WIDTHS, (1, 3), _ALL)] +
    [(V, l, 9, 1, k) for (V, l), k in itertools.product(((300, 304), (7010, 7040), (8185, 8192)), _ALL)] +
    [(V, l, 16, 1, k) for (V, l), k in itertools.product(((300, 304), (7010, 7040), (8200, 8200)), _ALL)] +
    [(8200, 8200, 64, 1, k) for k in _NO_INITIAL] + [(65536, 65536, 16, 1, k) for k in _NO_INITIAL]))


@pytest.mark.parametrize("V,ldl,beam,B,kind", WIDE_CASES)
def test_wide_beam_topk(V, ldl, beam, B, kind):
    c = rd.topk_case(V, ldl, beam, B, kind)
    r_score, r_parent, r_token, r_fin, vals = c["ref"]
    assert rd.gaps_ok(vals, kind == "ties")
    score, parent, token, fin, _ = K.beam_topk(c["logits"].to(DEV), V, c["score"].to(DEV),
                                               c["fin"].to(DEV), beam, rd.END, rd.PAD)
    score, parent, token, fin = score.cpu(), parent.cpu(), token.cpu(), fin.cpu()
    assert not torch.isnan(score).any()
    assert torch.equal(token.long(), r_token) and torch.equal(parent.long(), r_parent)
    assert torch.equal(fin.long(), r_fin)
    dead = r_score == NINF
    assert torch.equal(score == NINF, dead)
    if kind == "initial" and (V, beam) == (7, 64):
        assert int(dead.sum()) == 57 * B
    err = (score.double() - r_score)[~dead].abs()
    assert (err <= 1e-4 * r_score[~dead].abs().clamp(min=1.0)).all()


def _check_selection(flat, beam, V, score, parent, token):
    """One sentence; flat: its f64 candidate values [beam * V] (-inf: none); parent: local."""
    tol = lambda v: 1e-4 * v.abs().clamp(min=1.0)
    n = int((score > NINF).sum())
    assert beam - n == max(0, beam - int((flat > NINF).sum())) and (score[:n] > NINF).all()
    idx = (parent * V + token)[:n].long()
    val = flat[idx]
    assert ((score[:n].double() - val).abs() <= tol(val)).all()
    assert idx.unique().numel() == n, "a candidate chosen twice"
    d = score[1:n] - score[:n - 1]
    assert (d <= 0).all() and (idx[1:][d == 0] > idx[:-1][d == 0]).all()
    rest = flat.clone()
    rest[idx] = NINF
    assert rest.max() <= val.min() + tol(val.min()), "a better candidate was left out"


def test_wide_beam_topk_undecidable_order():
    V, ldl, beam, B = 7010, 7040, 64, 3
    R = B * beam
    g = torch.Generator().manual_seed(1)
    logits = torch.full((R, ldl), 1e4).to(torch.bfloat16)  # topk_case's "random", without the seed search
    logits[:, :V] = (torch.randn(R, V, generator=g) * 3.0).to(torch.bfloat16)
    score = -5.0 * torch.rand(R, generator=g)
    fin = torch.zeros(R, dtype=torch.int32)
    fin[torch.rand(R, generator=g) < 0.3] = 1
    score[1] = NINF
    out = K.beam_topk(logits.to(DEV), V, score.to(DEV), fin.to(DEV), beam, rd.END, rd.PAD)
    o_score, o_parent, o_token = (x.cpu() for x in out[:3])
    x = logits[:, :V].double()
    cand = score.double().view(R, 1) + (x - torch.logsumexp(x, dim=-1, keepdim=True))
    only_pad = torch.full_like(cand, NINF)
    only_pad[:, rd.PAD] = score.double()
    cand = torch.where(fin.view(R, 1) != 0, only_pad, cand)
    for s in range(B):
        rows = slice(s * beam, (s + 1) * beam)
        _check_selection(cand[rows].reshape(-1), beam, V, o_score[rows], o_parent[rows] - s * beam,
                         o_token[rows])


@pytest.mark.parametrize("bad", ["beam65", "int64_fin", "f32_logits", "small_ws"])
def test_wide_binding_refuses_before_writing(bad):
    beam = 65 if bad == "beam65" else 16
    R, V = beam * 2, 16
    logits = torch.zeros(R, V, dtype=torch.bfloat16, device=DEV)
    score = torch.zeros(R, dtype=torch.float32, device=DEV)
    fin = torch.zeros(R, dtype=torch.int32, device=DEV)
    outs, ws = _outs(R), _ws(R, beam)
    fin = fin.long() if bad == "int64_fin" else fin
    logits = logits.float() if bad == "f32_logits" else logits
    ws = ws[:-1] if bad == "small_ws" else ws
    with pytest.raises(RuntimeError):
        C().beam_topk_wide(logits, V, score, fin, beam, 3, 0, *outs, ws)
    torch.cuda.synchronize()
    for x in outs + [ws]:
        assert (x.float() == SENT).all().item(), "a rejected call wrote to its output"


def test_beam16_end_to_end():
    m = Transformer(model_config("tiny", src_vocab=300, tgt_vocab=300)).build("cuda:0", seed=4)
    src = ByteTokenizer(300).tokenize(["muitas pessoas vieram à estação.", "olá", "este é um teste mais longo"])
    a = beam_search(m, src, START, END, beam=16, max_length=12, reorder="index")
    b = beam_search(m, src, START, END, beam=16, max_length=12, reorder="index")
    c = beam_search(m, src, START, END, beam=16, max_length=12, reorder="copy")
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y), "two beam-16 runs differ"
        assert torch.equal(x, z), "reorder='copy' differs from 'index'"
    all_scores = a[3].cpu()
    assert all_scores.shape == (3, 16) and torch.isfinite(all_scores[:, 0]).all()
    assert torch.equal(all_scores, all_scores.sort(dim=1, descending=True).values)
    narrow = beam_search(m, src, START, END, beam=8, max_length=12)[3].cpu()
    assert (all_scores[:, 0] >= narrow[:, 0]).all(), (all_scores[:, 0], narrow[:, 0])
