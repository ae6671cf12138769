"""The n-gram match kernel (csrc/kernels/overlap.hip) against the Counter
reference of ref_overlap.py, bit for bit: every edge length pair, vocabulary
and kind, strided rows, poisoned padding, clamped lengths, bad indices, the
pairs-per-workgroup tails, determinism, and its binding's validation."""
import random

import pytest
import torch

import ref_overlap as R
from tensorflow_distributed_on_gke_amd.ops.kernels.overlap import ngram_matches
from tensorflow_distributed_on_gke_amd.ops._ext import C

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -77
MARGIN = 16  # sentinel rows beyond P in the allocation the output is a view of


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _run(tok, length, pa, pb, prepass=False):
    """The kernel into the first P rows of a longer, sentinel-filled
    allocation; returns that view after checking the margin."""
    P = pa.numel()
    buf = torch.full((P + MARGIN, 4), SENT, dtype=torch.int32, device=DEV)
    ranks = None
    if prepass:
        ranks = torch.full((tok.shape[0], tok.shape[1], 4), -1, dtype=torch.int16, device=DEV)
    C().ngram_matches(tok, length, pa, pb, buf[:P], ranks)
    torch.cuda.synchronize()
    assert (buf[P:] == SENT).all(), "the kernel wrote beyond row P"
    return buf[:P]


def _packed(rows, L=None, fill=0):
    tok, length = R.pack(rows, L, fill)
    return tok.to(DEV), length.to(DEV)


def _pairs(pairs):
    return _i32([p[0] for p in pairs]), _i32([p[1] for p in pairs])


@pytest.mark.parametrize("case", R.cases(), ids=lambda c: c[0])
def test_kernel_matches_reference(case):
    _, rows, pairs, exp = case
    tok, length = _packed(rows)
    pa, pb = _pairs(pairs)
    want = _i32(exp)
    got = _run(tok, length, pa, pb)
    assert torch.equal(got, want)
    assert torch.equal(_run(tok, length, pb, pa), want), "m(a, b) != m(b, a)"
    assert torch.equal(_run(tok, length, pa, pb, prepass=True), want), "ranks from the pre-pass"
    assert torch.equal(_run(tok, length, pb, pa, prepass=True), want)
    # the public wrapper is the same launch
    assert torch.equal(ngram_matches(tok, length, pa, pb), got)
    assert torch.equal(ngram_matches(tok, length, pa, pb, prepass=True), got)


def _long_case():
    """The cases that hold a row of 512 tokens."""
    return [c for c in R.cases() if max(len(r) for r in c[1]) == 512]


def test_strided_rows():
    """L = 512 with row stride 520, and a column slice of a wider tensor."""
    for _, rows, pairs, exp in _long_case()[::5]:
        tok, length = _packed(rows)
        N = tok.shape[0]
        pa, pb = _pairs(pairs)
        wide = torch.full((N, 520), 7, dtype=torch.int32, device=DEV)
        wide[:, :512] = tok
        assert torch.equal(_run(wide[:, :512], length, pa, pb), _i32(exp))
        assert torch.equal(_run(wide[:, :512], length, pa, pb, prepass=True), _i32(exp))
        wider = torch.full((N, 600), 7, dtype=torch.int32, device=DEV)
        wider[:, 37:549] = tok
        assert torch.equal(_run(wider[:, 37:549], length, pa, pb), _i32(exp))
        assert ngram_matches(wider[:, 37:549], length, pa, pb).tolist() == [list(e) for e in exp]


@pytest.mark.parametrize("prepass", [False, True])
def test_poisoned_padding(prepass):
    """Everything beyond a row's length holds the row's own first tokens, or
    its partner's tokens: neither is ever compared."""
    picked = R.cases()[3::7]
    for _, rows, pairs, exp in picked:
        L = min(512, max(len(r) for r in rows) + 70)
        for variant in ("own", "partner"):
            tok, length = _packed(rows, L)
            for a, b in pairs:
                for me, other in ((a, b), (b, a)):
                    src = rows[me] if variant == "own" else rows[other]
                    n = len(rows[me])
                    if src and n < L:
                        tail = [src[k % len(src)] for k in range(L - n)]
                        tok[me, n:] = torch.tensor(tail, dtype=torch.int64).to(torch.int32).to(DEV)
            pa, pb = _pairs(pairs)
            assert torch.equal(_run(tok, length, pa, pb, prepass), _i32(exp)), variant


@pytest.mark.parametrize("prepass", [False, True])
def test_lengths_are_clamped(prepass):
    rng = random.Random(5)
    for L in (6, 64, 130):
        rows = [[rng.choice([1, 2]) for _ in range(L)] for _ in range(3)]
        tok, _ = _packed(rows)
        pa, pb = _i32([0, 1, 2, 1, 0]), _i32([1, 2, 0, 1, 0])
        got = _run(tok, _i32([-3, L + 9, L]), pa, pb, prepass)
        assert torch.equal(got, _run(tok, _i32([0, L, L]), pa, pb, prepass))
        want = [R.matches_ref(x, y) for x, y in (([], rows[1]), (rows[1], rows[2]), (rows[2], []),
                                                 (rows[1], rows[1]), ([], []))]
        assert got.tolist() == [list(w) for w in want]


@pytest.mark.parametrize("P", [1, 3, 5, 257])
def test_pair_count_tails(P):
    rng = random.Random(P)
    rows = [[rng.choice([3, 4, 5]) for _ in range(rng.choice([0, 2, 9, 63, 64, 70]))] for _ in range(12)]
    tok, length = _packed(rows)
    pairs = [(rng.randrange(12), rng.randrange(12)) for _ in range(P)]
    want = _i32([R.matches_ref(rows[a], rows[b]) for a, b in pairs])
    for prepass in (False, True):
        assert torch.equal(_run(tok, length, *_pairs(pairs), prepass), want)


def test_repeated_self_and_swapped_pairs():
    _, rows, _, _ = R.cases()[40]
    tok, length = _packed(rows)
    a, b = 2, 7
    pairs = [(a, b), (a, b), (a, a), (b, a), (b, b)]
    got = _run(tok, length, *_pairs(pairs))
    m = list(R.matches_ref(rows[a], rows[b]))
    self_of = lambda r: [max(len(rows[r]) - n + 1, 0) for n in range(1, 5)]
    assert got.tolist() == [m, m, self_of(a), m, self_of(b)]


@pytest.mark.parametrize("prepass", [False, True])
def test_bad_indices_give_minus_one(prepass):
    _, rows, _, _ = R.cases()[8]
    tok, length = _packed(rows)
    N = len(rows)
    pairs = [(0, 1), (-1, 1), (2, 3), (2, N), (N, -1), (4, 5), (-2 ** 31, 0), (0, 2 ** 31 - 1), (6, 7)]
    got = _run(tok, length, *_pairs(pairs), prepass)
    want = [list(R.matches_ref(rows[a], rows[b])) if 0 <= a < N and 0 <= b < N else [-1] * 4
            for a, b in pairs]
    assert got.tolist() == want


def test_no_pairs():
    tok, length = _packed([[1, 2, 3]])
    empty = _i32([])
    assert _run(tok, length, empty, empty).shape == (0, 4)
    out = ngram_matches(tok, length, empty, empty)
    assert out.shape == (0, 4) and out.dtype == torch.int32 and out.is_cuda


def test_deterministic_and_order_independent():
    _, rows, _, _ = R.cases()[-1]
    tok, length = _packed(rows)
    N = len(rows)
    rng = random.Random(9)
    pairs = [(rng.randrange(N), rng.randrange(N)) for _ in range(301)]
    pa, pb = _pairs(pairs)
    first = _run(tok, length, pa, pb)
    assert torch.equal(first, _run(tok, length, pa, pb))
    perm = torch.randperm(len(pairs), generator=torch.Generator().manual_seed(1)).to(DEV)
    assert torch.equal(_run(tok, length, pa[perm], pb[perm]), first[perm])
    assert torch.equal(_run(tok, length, pa[:17], pb[:17]), first[:17]), "depends on P"


def test_binding_rejects():
    N, L, P = 4, 8, 3
    tok = torch.ones(N, L, dtype=torch.int32, device=DEV)
    length = torch.full((N,), L, dtype=torch.int32, device=DEV)
    pa, pb = _i32([0, 1, 2]), _i32([1, 2, 3])
    out = torch.full((P, 4), SENT, dtype=torch.int32, device=DEV)
    long_out = torch.full((P + 1, 4), SENT, dtype=torch.int32, device=DEV)
    wide_out = torch.full((P, 8), SENT, dtype=torch.int32, device=DEV)
    ranks = torch.full((N, L, 4), -1, dtype=torch.int16, device=DEV)

    def call(t=tok, ln=length, a=pa, b=pb, o=out, r=None):
        C().ngram_matches(t, ln, a, b, o, r)

    one = torch.zeros(1, dtype=torch.int32, device=DEV)
    bad = [dict(t=tok.long()), dict(t=tok.float()), dict(t=tok.cpu()),  # dtypes, CPU tensors
           dict(ln=length.long()), dict(a=pa.long()), dict(b=pb.long()),
           dict(ln=length.cpu()), dict(a=pa.cpu()), dict(b=pb.cpu()), dict(o=out.cpu()),
           dict(t=torch.ones(N, 513, dtype=torch.int32, device=DEV)),  # L outside [1, 512]
           dict(t=torch.ones(N, 0, dtype=torch.int32, device=DEV)),
           dict(t=tok.view(N, L, 1)), dict(t=tok.view(-1)),  # not 2-D
           dict(t=torch.ones(L, N, dtype=torch.int32, device=DEV).t()),  # columns not contiguous
           dict(ln=length[:3]), dict(ln=length.view(N, 1)),  # wrong size, not 1-D
           dict(ln=torch.cat([length, length])[::2]),  # not contiguous
           dict(a=pa[:2]), dict(b=pb[:2]), dict(b=pb.view(P, 1)), dict(a=pa.view(1, P)),
           dict(a=_i32([0, 9, 1, 9, 2, 9])[::2]), dict(b=_i32([1, 9, 2, 9, 3, 9])[::2]),
           dict(o=long_out), dict(o=out[:2]), dict(o=wide_out), dict(o=wide_out[:, :4]),
           dict(o=out.view(-1)), dict(o=out.float()), dict(o=out.long()),
           dict(o=torch.full((4, P), SENT, dtype=torch.int32, device=DEV).t()),
           dict(r=ranks.int()), dict(r=ranks[:, :, :2]), dict(r=ranks.cpu()), dict(r=ranks[:2]),
           # N or P >= 2 ** 31 (views without memory behind every element)
           dict(t=one.view(1, 1).expand(2 ** 31, 1)), dict(a=one.expand(2 ** 31))]
    if torch.cuda.device_count() > 1:
        other = torch.device("cuda", 1)
        bad += [dict(ln=length.to(other)), dict(a=pa.to(other)), dict(o=out.to(other))]
    for kw in bad:
        with pytest.raises(RuntimeError):
            call(**kw)
        torch.cuda.synchronize()
        for o in (out, long_out, wide_out):
            assert (o == SENT).all(), f"a rejected call wrote its output: {list(kw)}"
        assert (ranks == -1).all()
    call()  # the same call well-formed
    torch.cuda.synchronize()
    assert out.tolist() == [[8, 7, 6, 5]] * P
    call(r=ranks)
    torch.cuda.synchronize()
    assert out.tolist() == [[8, 7, 6, 5]] * P
    assert ranks[0, :, 0].tolist() == list(range(L))


def test_wrapper_rejects():
    tok = torch.ones(2, 8, dtype=torch.int32, device=DEV)
    ln = torch.full((2,), 8, dtype=torch.int32, device=DEV)
    p = _i32([0])
    for kw in (dict(tok=tok.long()), dict(tok=tok.view(-1)), dict(length=ln[:1]), dict(pair_b=_i32([0, 1])),
               dict(pair_a=p.long()), dict(length=ln.cpu()),
               dict(tok=torch.ones(2, 513, dtype=torch.int32, device=DEV))):
        with pytest.raises(RuntimeError):
            ngram_matches(**dict(dict(tok=tok, length=ln, pair_a=p, pair_b=p), **kw))
