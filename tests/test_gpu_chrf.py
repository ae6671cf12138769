"""The character n-gram kernels (csrc/kernels/chrf.hip) against the Counter
reference of ref_chrf.py, bit for bit, and corpus chrF and chrF-utility MBR on
the GPU against the same reference."""
import random

import pytest
import torch

import ref_chrf as R
from tensorflow_distributed_on_gke_amd.infer.chrf import corpus_chrf
from tensorflow_distributed_on_gke_amd.infer.mbr import select_text
from tensorflow_distributed_on_gke_amd.ops._ext import C
from tensorflow_distributed_on_gke_amd.ops.kernels.chrf import char_ngram_matches
from tensorflow_distributed_on_gke_amd.ops.kernels.overlap import ngram_matches

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -77
MARGIN = 16  # sentinel rows beyond P in the allocation the output is a view of


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _run(chr_, length, pa, pb):
    """The binding on garbage-filled scratch, into the first P rows of a
    longer sentinel-filled allocation; returns that view after checking the margin."""
    P = pa.numel()
    N, L = chr_.shape
    buf = torch.full((P + MARGIN, 6), SENT, dtype=torch.int32, device=DEV)
    keys = torch.full((N, L, 2), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=DEV)
    ranks = torch.full((N, L, 8), -1, dtype=torch.int16, device=DEV)
    C().char_ngram_matches(chr_, length, pa, pb, buf[:P], keys, ranks)
    torch.cuda.synchronize()
    assert (buf[P:] == SENT).all(), "the kernel wrote beyond row P"
    return buf[:P]


def _packed(rows, L=None, fill=0):
    chr_, length = R.pack(rows, L, fill)
    return chr_.to(DEV), length.to(DEV)


def _pairs(pairs):
    return _i32([p[0] for p in pairs]), _i32([p[1] for p in pairs])


@pytest.mark.parametrize("case", R.cases(), ids=lambda c: c[0])
def test_kernel_matches_reference(case):
    _, rows, pairs, exp = case
    chr_, length = _packed(rows)
    pa, pb = _pairs(pairs)
    want = _i32(exp)
    got = _run(chr_, length, pa, pb)
    assert torch.equal(got, want)
    assert torch.equal(_run(chr_, length, pb, pa), want), "m(a, b) != m(b, a)"
    assert torch.equal(char_ngram_matches(chr_, length, pa, pb), want), "the public wrapper"
    # the all-pairs kernel on the same tensors, where it admits both rows
    short = [k for k, (a, b) in enumerate(pairs) if max(len(rows[a]), len(rows[b])) <= 512]
    four = ngram_matches(chr_[:, :512], length.clamp(max=512), pa[short], pb[short])
    assert torch.equal(got[short, :4], four)


def test_rows_and_output_handling():
    """Strided rows, poisoned padding, clamped lengths, bad indices, the
    pairs-per-workgroup tails, and independence of P and of the pair order."""
    rng = random.Random(3)
    al = R.ALPHABETS["two"]
    rows = [[rng.choice(al) for _ in range(n)] for n in (0, 5, 64, 65, 130, 257, 300, 9)]
    N, L = len(rows), 300
    wide = torch.full((N, 400), al[0], dtype=torch.int32, device=DEV)
    for i, r in enumerate(rows):  # beyond its length a row holds its own, then its partner's characters
        src = (r or al) + (rows[i ^ 1] or al)
        wide[i, 37:37 + L] = _i32([r[k] if k < len(r) else src[k % len(src)] for k in range(L)])
    chr_ = wide[:, 37:37 + L]  # a column slice: row stride 400
    length = _i32([len(r) for r in rows])
    for P in (1, 3, 5, 257):
        pairs = [(rng.randrange(-1, N + 1), rng.randrange(N)) for _ in range(P)]
        want = [list(R.matches_ref(rows[a], rows[b])) if 0 <= a < N else [-1] * 6 for a, b in pairs]
        pa, pb = _pairs(pairs)
        first = _run(chr_, length, pa, pb)
        assert first.tolist() == want
        assert torch.equal(first, _run(chr_, length, pa, pb))
        perm = torch.randperm(P, generator=torch.Generator().manual_seed(P)).to(DEV)
        assert torch.equal(_run(chr_, length, pa[perm], pb[perm]), first[perm])
        assert torch.equal(_run(chr_, length, pa[:2], pb[:2]), first[:2]), "depends on P"
    got = _run(chr_, _i32([-3, 5, 64, L + 9, 130, 257, L, 9]), _i32([0, 3, 6, 0, 2 ** 31 - 1]),
               _i32([3, 6, 0, 0, 1]))
    x, y = chr_[3].tolist(), chr_[6].tolist()
    assert got.tolist() == [list(R.matches_ref([], x)), list(R.matches_ref(x, y)), [0] * 6, [0] * 6, [-1] * 6]


LINES = ["the cat sat on the mat", "the  cat sat\ton a mat ", "猫がマットの上に座った", "été comme été",
         "𝒳 maps 😀 to 𝒴", "", " \t ", "The Cat"]
REFS = ["the cat is on the mat", "the cat sat on a mat", "猫はマットの上に座った", "e\u0301te\u0301 comme été",
        "𝒳 maps 😀 to 𝒵", "not empty", "", "the cat"]


@pytest.mark.parametrize("lc,beta,order", [(False, 2.0, 6), (True, 1.0, 6), (False, 3.0, 4)])
def test_corpus_chrf(lc, beta, order):
    got = corpus_chrf(LINES, REFS, lowercase=lc, beta=beta, order=order, device=DEV)
    assert abs(got.score - R.corpus_ref(LINES, REFS, lc, beta, order)) <= 1e-12
    assert got.hyp_chars == sum(len(R.units(h)) for h in LINES)


@pytest.mark.parametrize("lc", [False, True])
def test_select_text_chrf(lc):
    groups = [LINES, REFS[:5], [LINES[0]], ["", " "], LINES[::-1] + REFS]
    got = select_text(groups, lowercase=lc, device=DEV, utility="chrf")
    for (best, util), cands in zip(got, groups):
        want, expected = R.mbr_ref(cands, lc)
        assert best == want
        assert abs(100.0 * (util - expected[want])) <= 1e-12
