"""Cases and the float64 reference of teacher-forced scoring
(ops.kernels.decode.score_tokens, csrc/kernels/decode.hip): the label's value and the
row maximum of the mixture that ref_ensemble.py defines. The logits are
ref_ensemble's cases; the labels are drawn here from a seeded generator and
then forced to hit every special column and row of the case.
"""
import functools

import torch

import ref_ensemble as re_

NINF = re_.NINF
PAD = 0


def score_ref(mix, labels, pad_id=PAD):
    """mix f64 [R, V] (ensemble_ref), labels int [R] -> (tok f64 [R], top f64
    [R]): tok = mix[r, label], -inf for a label outside [0, V); top = the row
    maximum; both 0 on a row whose label is pad_id."""
    R, V = mix.shape
    lab = labels.long()
    inside = (lab >= 0) & (lab < V)
    tok = mix.gather(1, lab.clamp(0, V - 1).view(R, 1)).view(R)
    tok = torch.where(inside, tok, torch.full_like(tok, NINF))
    top = mix.max(dim=1).values
    ignored = lab == pad_id
    zero = torch.zeros(R, dtype=torch.float64)
    return torch.where(ignored, zero, tok), torch.where(ignored, zero, top)


def _forced(logits, V, R, kind):
    """(row, label) pairs every label set of a case must contain between
    them: the peaked column, a masked column, the NaN column, a pad_id row and
    a label == V."""
    out = [(r, (37 * r + 5) % V) for r in range(R)] if kind == "peaked" else []
    if kind == "masked":
        x0 = logits[0]
        out.append((0, V // 2))  # the NaN of member 0
        assert torch.isnan(x0[0, V // 2])
        for r in range(R):
            cols = (x0[r, :V] == NINF).nonzero().view(-1)
            if cols.numel():
                out.append((r, int(cols[0])))
                break
        else:
            raise AssertionError("no masked column")
    out.append((R // 2, PAD))
    out.append((0, V))
    return out


@functools.lru_cache(maxsize=None)
def case(V, ld, M, R, kind):
    """(logits, weights, sets): ref_ensemble.case's logits and weights and a
    tuple of label sets (labels int64 [R], tok f64 [R], top f64 [R]). Treat as
    read-only: the cases are shared."""
    logits, weights, mix = re_.case(V, ld, M, R, kind)
    g = torch.Generator().manual_seed(7000 + 100 * M + 10 * R + V % 991 + len(kind))
    todo = _forced(logits, V, R, kind)
    sets = []
    while True:
        labels = torch.randint(0, V, (R,), generator=g)
        used, rest = set(), []
        if sets:  # the first set is all random
            for r, lab in todo:
                if r in used:
                    rest.append((r, lab))
                else:
                    labels[r] = lab
                    used.add(r)
            todo = rest
        sets.append((labels,) + score_ref(mix, labels))
        if sets[1:] and not todo:
            return logits, weights, tuple(sets)


def check(got, ref, tag):
    """got f32 [R] against ref f64 [R]: no NaN, the -inf pattern exactly,
    finite values within ref_ensemble.f32_bound. Returns the largest error."""
    got = got.double().cpu()
    dead = ref == NINF
    assert not torch.isnan(got).any(), tag
    assert torch.equal(got == NINF, dead), (tag, "-inf pattern differs")
    err = (got - ref)[~dead].abs()
    assert (err <= re_.f32_bound(ref)[~dead]).all(), (tag, float(err.max()))
    return float(err.max()) if err.numel() else 0.0
