"""References for the character n-gram kernel and what is built on it: clipped
match counts with `collections.Counter` for n = 1..6, and the chrF score, its
corpus form and MBR selection in Python `math`. Imports nothing from the package
(the row generator and the packer are ref_overlap.py's)."""
from __future__ import annotations

import math
import random
from collections import Counter
from functools import lru_cache

from ref_overlap import make_pair, pack  # noqa: F401  (two rows of a kind; rows -> int32 tensors)

ORDERS = 6
# shorter than, equal to and just over the top order; the 64-lane chunk, the
# pre-pass workgroup (256), the sort-size (powers of two) and the row-length edges
EDGE = (0, 1, 5, 6, 7, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048)
FILL = (3, 40, 300)  # partners that are no edge: the pairs (edge, any) are what is asked for

ALPHABETS = {
    "one": [0x61],  # clipping and ranks decide everything
    "two": [0x61, 0x4E2D],
    "thousand": list(range(0x400, 0x400 + 1000)),
    "extreme": [0, 1, 0x10FFFE, 0x10FFFF],  # 0 is a character; the top of the 21 bits
}
KINDS = ("random", "shared", "repeat")


def matches_ref(x, y, orders=ORDERS):
    """(m_1 .. m_6): m_n = sum_g min(count_x(g), count_y(g)) over character n-grams."""
    grams = lambda s, n: Counter(tuple(s[i:i + n]) for i in range(len(s) - n + 1))
    return tuple(sum((grams(x, n) & grams(y, n)).values()) for n in range(1, orders + 1))


def score_ref(m, hyp, ref, beta=2.0):
    """chrF in [0, 1] from per-order matches and n-gram totals of the two
    sides: over the orders with both totals > 0, P = mean m / hyp, R = mean
    m / ref, F = (1 + b^2) P R / (b^2 P + R); 0 without such an order or with P + R = 0."""
    eff = [n for n in range(len(m)) if hyp[n] > 0 and ref[n] > 0]
    if not eff:
        return 0.0
    p = math.fsum(m[n] / hyp[n] for n in eff) / len(eff)
    r = math.fsum(m[n] / ref[n] for n in eff) / len(eff)
    return (1.0 + beta * beta) * p * r / (beta * beta * p + r) if p + r > 0 else 0.0


def units(line, lowercase=False):
    """The code points of a line without its whitespace."""
    return [ord(c) for c in "".join((line.lower() if lowercase else line).split())]


def totals(length, orders=ORDERS):
    return [max(length - n, 0) for n in range(orders)]


def sentence_ref(h, r, beta=2.0, orders=ORDERS):
    return score_ref(matches_ref(h, r, orders), totals(len(h), orders), totals(len(r), orders), beta)


def corpus_ref(hyps, refs, lowercase=False, beta=2.0, orders=ORDERS):
    """Corpus chrF on the 0-100 scale: statistics summed over the lines first."""
    m, th, tr = [0] * orders, [0] * orders, [0] * orders
    for h, r in zip(hyps, refs):
        h, r = units(h, lowercase), units(r, lowercase)
        for n, v in enumerate(matches_ref(h, r, orders)):
            m[n] += v
            th[n] += totals(len(h), orders)[n]
            tr[n] += totals(len(r), orders)[n]
    return 100.0 * score_ref(m, th, tr, beta)


def mbr_ref(cands, lowercase=False):
    """Candidate strings of one group -> (best, expected): expected[i] = the
    mean over all j, i included, of chrF(i as hypothesis, j as reference); the first argmax."""
    rows = [units(c, lowercase) for c in cands]
    expected = [math.fsum(sentence_ref(h, r) for r in rows) / len(rows) for h in rows]
    return max(range(len(rows)), key=lambda i: (expected[i], -i)), expected


@lru_cache(maxsize=None)
def cases(max_len=2048):
    """Per (alphabet, kind) one case over the ordered length pairs (edge, any)
    and (fill, edge) up to `max_len`: tuples (name, rows, pairs, expected) with
    pairs = (a, b) row indices and expected = matches_ref per pair. Every edge
    length meets a short, an equal and the longest partner. Computed once; do
    not modify."""
    edge = [e for e in EDGE if e <= max_len]
    lens = [(e, o) for i, e in enumerate(edge) for o in {edge[i], edge[(i * 5 + 3) % len(edge)], edge[-1]}]
    lens += [(f, e) for f in FILL for e in edge[1::3]]
    out = []
    for ai, (aname, alphabet) in enumerate(ALPHABETS.items()):
        for ki, kind in enumerate(KINDS):
            rng = random.Random(100 * ai + ki)
            rows, pairs, exp = [], [], []
            for la, lb in sorted(lens):
                x, y = make_pair(kind, alphabet, la, lb, rng)
                pairs.append((len(rows), len(rows) + 1))
                rows += [x, y]
                exp.append(matches_ref(x, y))
            out.append((f"{aname}-{kind}", rows, pairs, exp))
    return tuple(out)
