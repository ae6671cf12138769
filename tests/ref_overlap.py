"""References for the n-gram overlap kernel and what is built on it: clipped
match counts with `collections.Counter`, and sentence BLEU, MBR selection and
corpus BLEU in Python `math`. Imports nothing from the package's kernels."""
from __future__ import annotations

import math
import random
from collections import Counter
from functools import lru_cache

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1

# rows shorter than n, the 64-lane chunk edges (n-grams straddle them), the maximum
SHORT = (0, 1, 2, 3, 4, 5)
EDGE = (63, 64, 65, 67, 127, 128, 129, 511, 512)
LENGTHS = SHORT + EDGE

VOCABS = {
    "one": [7],  # clipping decides everything
    "two": [3, 4],  # many repeats: ranks are stressed
    "thousand": list(range(1000)),
    "extreme": [-1, -2, INT32_MIN, INT32_MAX, 0],  # no value is a sentinel
}
KINDS = ("random", "shared", "repeat", "disjoint")
ROWS_PER_CASE = 40


def ngrams(x, n):
    return Counter(tuple(x[i:i + n]) for i in range(len(x) - n + 1))


def matches_ref(x, y):
    """(m_1 .. m_4): m_n = sum_g min(count_x(g), count_y(g))."""
    return tuple(sum((ngrams(x, n) & ngrams(y, n)).values()) for n in range(1, 5))


def sentence_bleu(m, len_h, len_r):
    """Smoothed sentence BLEU of a hypothesis of len_h tokens against a
    reference of len_r with clipped matches m (4 ints): p_1 = m_1 / len_h,
    p_n = (m_n + 1) / (max(len_h - n + 1, 0) + 1) for n = 2..4, brevity
    penalty min(1, exp(1 - len_r / len_h)); 0 without a unigram match."""
    if len_h == 0 or m[0] == 0:
        return 0.0
    logs = math.log(m[0] / len_h)
    for n in (2, 3, 4):
        logs += math.log((m[n - 1] + 1) / (max(len_h - n + 1, 0) + 1))
    return min(1.0, math.exp(1.0 - len_r / len_h)) * math.exp(0.25 * logs)


def mbr_ref(cands, valid=None):
    """cands: token lists of one group -> (best, expected): expected[i] = the
    mean over the valid j (i included) of u(i, j), -inf for an invalid i; best
    = the first argmax, 0 for a group without a valid candidate."""
    n = len(cands)
    valid = [True] * n if valid is None else list(valid)
    nv = sum(valid)
    expected = []
    for i in range(n):
        if not valid[i]:
            expected.append(float("-inf"))
            continue
        us = [sentence_bleu(matches_ref(cands[i], cands[j]), len(cands[i]), len(cands[j]))
              for j in range(n) if valid[j]]
        expected.append(math.fsum(us) / nv)
    best = 0
    for i in range(n):
        if expected[i] > expected[best]:
            best = i
    return best, expected


def content(row, end, pad):
    """A decoded row ([START] first) -> its tokens up to the first `end`,
    without the `pad`s they end in."""
    row = list(row[1:])
    row = row[:row.index(end)] if end in row else row
    while row and row[-1] == pad:
        row.pop()
    return row


def corpus_bleu_ref(hyps, refs, lowercase=False):
    """Papineni's corpus BLEU over whitespace words, one reference per
    hypothesis -> dict(score, precisions, bp, hyp_len, ref_len, matches, totals)."""
    m, tot = [0] * 4, [0] * 4
    lh = lr = 0
    for h, r in zip(hyps, refs):
        if lowercase:
            h, r = h.lower(), r.lower()
        h, r = h.split(), r.split()
        for n, v in enumerate(matches_ref(h, r)):
            m[n] += v
            tot[n] += max(len(h) - n, 0)
        lh += len(h)
        lr += len(r)
    prec = [m[n] / tot[n] if tot[n] else 0.0 for n in range(4)]
    bp = 1.0 if lh >= lr else (math.exp(1.0 - lr / lh) if lh else 0.0)
    score = 0.0 if min(m) == 0 else 100.0 * bp * math.exp(0.25 * sum(math.log(p) for p in prec))
    return dict(score=score, precisions=prec, bp=bp, hyp_len=lh, ref_len=lr, matches=m, totals=tot)


def make_pair(kind, vocab, la, lb, rng):
    """Two rows of la and lb tokens."""
    pick = lambda n, v=vocab: [rng.choice(v) for _ in range(n)]
    if kind == "random":
        return pick(la), pick(lb)
    if kind == "shared":  # y: x (repeated or cut to lb) with a few substitutions
        x = pick(la)
        y = [x[i % la] for i in range(lb)] if la else pick(lb)
        for _ in range(min(3, lb)):
            y[rng.randrange(lb)] = rng.choice(vocab)
        return x, y
    if kind == "repeat":  # a short period repeated; y the same period, another phase
        period = pick(rng.randint(1, 5))
        ph = rng.randrange(len(period))
        return ([period[i % len(period)] for i in range(la)],
                [period[(i + ph) % len(period)] for i in range(lb)])
    # disjoint: the halves of the vocabulary (a single-token one: y from outside it)
    half = max(1, len(vocab) // 2)
    vy = vocab[half:] or [vocab[0] + 1]
    return pick(la, vocab[:half]), pick(lb, vy)


@lru_cache(maxsize=None)
def cases():
    """Every (vocabulary, kind) over every ordered length pair with at least one
    edge length, at most ROWS_PER_CASE rows each: tuples (name, rows, pairs,
    expected) with rows = token lists, pairs = (a, b) row indices and expected
    = matches_ref per pair. Computed once; do not modify."""
    lens = sorted(((la, lb) for la in LENGTHS for lb in LENGTHS if la in EDGE or lb in EDGE),
                  key=lambda p: (max(p), p))
    per = ROWS_PER_CASE // 2
    out = []
    for vi, (vname, vocab) in enumerate(VOCABS.items()):
        for ki, kind in enumerate(KINDS):
            rng = random.Random(1000 * vi + ki)
            for c0 in range(0, len(lens), per):
                rows, pairs, exp = [], [], []
                for la, lb in lens[c0:c0 + per]:
                    x, y = make_pair(kind, vocab, la, lb, rng)
                    pairs.append((len(rows), len(rows) + 1))
                    rows += [x, y]
                    exp.append(matches_ref(x, y))
                out.append((f"{vname}-{kind}-{c0 // per}", rows, pairs, exp))
    return tuple(out)


def pack(rows, L=None, fill=0):
    """rows -> (tok int32 [N, L], length int32 [N]) torch tensors on the CPU."""
    import torch

    L = max(1, max(len(r) for r in rows)) if L is None else L
    tok = torch.full((len(rows), L), fill, dtype=torch.int32)
    for i, r in enumerate(rows):
        tok[i, :len(r)] = torch.tensor(r, dtype=torch.int64).to(torch.int32)
    return tok, torch.tensor([len(r) for r in rows], dtype=torch.int32)
