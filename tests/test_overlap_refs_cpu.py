"""The n-gram overlap references against each other and the hand cases, and the
wrapper's CPU arm against them (no GPU)."""
import pytest
import torch

import ref_overlap as R
from tensorflow_distributed_on_gke_amd.ops.kernels.overlap import ngram_matches

CANDS = ["the cat sat on the mat", "the cat sat on a mat", "a cat sat on the mat", "a dog"]

HAND = [
    ([7] * 10, [7] * 3, (3, 2, 1, 0)),
    ([], [1, 2, 3], (0, 0, 0, 0)),
    ([1, 2, 3], [], (0, 0, 0, 0)),
    ([1, 2, 3, 4], [1, 2, 3, 4], (4, 3, 2, 1)),
    ([1, 2, 1, 2, 1], [2, 1, 2], (3, 2, 1, 0)),
    ([0, 0, 5], [0, 5, 0, 0], (3, 2, 0, 0)),
    ([R.INT32_MIN, -1, R.INT32_MAX], [-1, R.INT32_MAX, R.INT32_MIN], (3, 1, 0, 0)),
]


def rank_matches(x, y):
    """The position-wise formulation, brute force: m_n = the positions i of x
    whose n-gram has fewer earlier occurrences in x than occurrences in y."""
    out = []
    for n in range(1, 5):
        gx = [tuple(x[i:i + n]) for i in range(len(x) - n + 1)]
        gy = [tuple(y[j:j + n]) for j in range(len(y) - n + 1)]
        out.append(sum(1 for i, g in enumerate(gx)
                       if sum(1 for h in gx[:i] if h == g) < sum(1 for h in gy if h == g)))
    return tuple(out)


def test_hand_cases():
    for x, y, want in HAND:
        assert R.matches_ref(x, y) == want, (x, y)
        assert rank_matches(x, y) == want, (x, y)
        assert R.matches_ref(y, x) == want, (x, y)


def test_reference_against_rank_formulation_and_symmetry():
    n = 0
    for name, rows, pairs, exp in R.cases():
        for (a, b), want in zip(pairs, exp):
            x, y = rows[a], rows[b]
            if max(len(x), len(y)) > 129:  # the brute force is quadratic
                continue
            assert rank_matches(x, y) == want, name
            assert R.matches_ref(y, x) == want, name
            n += 1
    assert n > 1000


def test_self_pair_counts_every_ngram():
    for L in R.LENGTHS:
        x = [i % 3 for i in range(L)]
        assert R.matches_ref(x, x) == tuple(max(L - n + 1, 0) for n in range(1, 5))


def test_worked_mbr_example():
    cands = [c.split() for c in CANDS]
    u = lambda i, j: R.sentence_bleu(R.matches_ref(cands[i], cands[j]), len(cands[i]), len(cands[j]))
    assert abs(u(0, 1) - 0.638943) < 1e-6
    assert abs(u(0, 2) - 0.803428) < 1e-6
    assert u(0, 3) == 0.0
    assert abs(u(3, 1) - 0.095696) < 1e-6
    assert abs(u(1, 3) - 0.193049) < 1e-6
    assert all(u(i, i) == 1.0 for i in range(4))
    best, expected = R.mbr_ref(cands)
    assert best == 2
    for got, want in zip(expected, (0.610593, 0.576216, 0.617337, 0.297848)):
        assert abs(got - want) < 1e-6


def test_worked_bleu_example():
    b = R.corpus_bleu_ref(["the cat sat on the mat", "a dog barked"],
                          ["the cat sat on a mat", "the dog barked loudly"])
    assert b["matches"] == [7, 4, 2, 1] and b["totals"] == [9, 7, 5, 3]
    assert (b["hyp_len"], b["ref_len"]) == (9, 10)
    assert abs(b["score"] - 44.150346) < 1e-6


@pytest.mark.parametrize("case", R.cases(), ids=lambda c: c[0])
def test_cpu_arm_matches_reference(case):
    _, rows, pairs, exp = case
    tok, length = R.pack(rows)
    pa = torch.tensor([p[0] for p in pairs], dtype=torch.int32)
    pb = torch.tensor([p[1] for p in pairs], dtype=torch.int32)
    want = torch.tensor(exp, dtype=torch.int32)
    assert torch.equal(ngram_matches(tok, length, pa, pb), want)
    assert torch.equal(ngram_matches(tok, length, pb, pa), want)


def test_cpu_arm_hand_cases_lengths_and_bad_pairs():
    rows = [r for x, y, _ in HAND for r in (x, y)]
    tok, length = R.pack(rows, L=12, fill=7)  # the fill equals real tokens: it must not count
    P = len(HAND)
    pa = torch.arange(0, 2 * P, 2, dtype=torch.int32)
    got = ngram_matches(tok, length, pa, pa + 1)
    assert got.tolist() == [list(w) for _, _, w in HAND]
    # lengths outside [0, L] are clamped into it
    tok = torch.tensor([[1, 2, 1, 2, 1, 2], [2, 1, 2, 1, 2, 1]], dtype=torch.int32)
    odd = torch.tensor([-3, 6 + 9], dtype=torch.int32)
    assert ngram_matches(tok, odd, torch.tensor([0, 1, 1], dtype=torch.int32),
                         torch.tensor([1, 0, 1], dtype=torch.int32)).tolist() == [
        [0, 0, 0, 0], [0, 0, 0, 0], [6, 5, 4, 3]]
    # indices outside [0, N) give -1, their neighbours are unaffected
    full = torch.tensor([6, 6], dtype=torch.int32)
    got = ngram_matches(tok, full, torch.tensor([0, -1, 0, 2, 1], dtype=torch.int32),
                        torch.tensor([1, 0, 1, 1, 0], dtype=torch.int32))
    want = list(R.matches_ref(tok[0].tolist(), tok[1].tolist()))
    assert got.tolist() == [want, [-1] * 4, want, [-1] * 4, want]
    assert ngram_matches(tok, full, full[:0], full[:0]).shape == (0, 4)
