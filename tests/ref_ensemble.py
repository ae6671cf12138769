"""Case tables and the float64 reference of the ensemble's combine step
(ops.kernels.ensemble_logprobs, csrc/kernels/decode.hip): the log of the
weighted mean of M members' next-token probabilities.

Every logit of a case is a bf16 value held in f32, so the CPU tests (f32
inputs) and the GPU tests (the same values as bf16) share cases and reference.
The padding columns [V, ldl) of a member hold +1e4: a kernel that read them
would show it.
"""
import functools
import math

import torch

NINF = float("-inf")
SHAPES = ((7, 8), (300, 304), (7010, 7040))  # (V, ldo); members' ldl = ldo
BIG_SHAPE = (65536, 65536)                   # GPU only, R = 2
MEMBERS = (1, 2, 3, 8)
ROWS = (1, 5)
KINDS = ("random", "peaked", "masked", "weights")


def _bf(x):
    return x.to(torch.bfloat16).float()


def ensemble_ref(logits_list, V, weights=None):
    """f64 [R, V]: log sum_m w_m softmax(x_m[r])[v], weights normalised to sum
    1. A NaN or -inf logit has probability 0; a member's row without a finite
    logit contributes nothing; a row no member has a finite logit in is -inf."""
    M = len(logits_list)
    w = [1.0] * M if weights is None else [float(x) for x in weights]
    total = math.fsum(w)
    parts = []
    for x, wm in zip(logits_list, w):
        x = x[:, :V].double()
        x = torch.where(x > NINF, x, torch.full_like(x, NINF))
        lse = torch.logsumexp(x, dim=1, keepdim=True)
        parts.append(torch.where(lse > NINF, x - lse + math.log(wm / total), torch.full_like(x, NINF)))
    return torch.logsumexp(torch.stack(parts), dim=0)


@functools.lru_cache(maxsize=None)
def case(V, ld, M, R, kind):
    """(logits: M tensors f32 [R, ld] of bf16 values, weights or None, ref f64
    [R, V]). Treat as read-only: the cases are shared."""
    g = torch.Generator().manual_seed(1000 * M + 10 * R + V % 997 + len(kind))
    logits = []
    for m in range(M):
        x = torch.full((R, ld), 1e4)
        x[:, :V] = _bf(torch.randn(R, V, generator=g) * 4.0)
        logits.append(x)
    weights = None
    if kind == "peaked":
        # one member is certain of a column: there the others vanish beside it,
        # everywhere else it vanishes beside them
        for r in range(R):
            logits[(r + 1) % M][r, (37 * r + 5) % V] += 60.0
    elif kind == "masked":
        for m in range(M):
            for r in range(R):
                logits[m][r, torch.randperm(V, generator=g)[: V // 3]] = NINF
        logits[0][0, V // 2] = float("nan")
        if M > 1:
            logits[1][0, :V] = NINF  # a member's row without a finite logit
        if R > 1:
            for m in range(M):
                logits[m][R - 1, :V] = NINF  # a row dead in every member
            logits[0][R - 1, 0] = float("nan")
    elif kind == "weights":
        weights = tuple(0.5 + ((3 * m + 1) % 5) for m in range(M))
    for x in logits:
        x[:, :V] = torch.where(torch.isnan(x[:, :V]), x[:, :V], _bf(x[:, :V]))
    return tuple(logits), weights, ensemble_ref(logits, V, weights)


def live_mass(logits_list, V, weights=None):
    """f64 [R]: the total weight of the members that have a finite logit in
    the row, which is what the mixture's probabilities sum to by its
    definition: 1 where every member is alive, 0 on a row dead in all."""
    M = len(logits_list)
    w = [1.0] * M if weights is None else [float(x) for x in weights]
    alive = torch.stack([(x[:, :V] > NINF).any(dim=1) for x in logits_list]).double()
    return (alive * torch.tensor(w, dtype=torch.float64).view(M, 1)).sum(dim=0) / math.fsum(w)


def f32_bound(ref):
    """The f32 logsumexp tolerance the selection kernels' scores are held to."""
    return 1e-4 * ref.abs().clamp(min=1.0)


def bf16_bound(ref):
    """One bf16 rounding of the output (round to nearest: half an ulp, below
    2^-8 |ref|) plus the f32 accumulation term."""
    return 2.0 ** -8 * ref.abs() + 1e-4


def check_against(out, ref, bound, tag):
    """out [R, >= V] against ref f64 [R, V]: the -inf pattern exactly, finite
    values within `bound`, columns from V on all -inf. Returns the largest
    error."""
    V = ref.shape[1]
    got = out[:, :V].double().cpu()
    dead = ref == NINF
    assert not torch.isnan(got).any(), tag
    assert torch.equal(got == NINF, dead), (tag, "-inf pattern differs")
    assert (out[:, V:].float().cpu() == NINF).all(), (tag, "padding columns are not -inf")
    err = (got - ref)[~dead].abs()
    assert (err <= bound(ref)[~dead]).all(), (tag, float(err.max()))
    return float(err.max()) if err.numel() else 0.0
