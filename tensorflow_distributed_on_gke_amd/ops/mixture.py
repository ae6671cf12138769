"""The weights of a mixture of distributions over the vocabulary: an ensemble's
members, a student's teachers. One copy for every launch wrapper and caller
that takes them (the family modules of ops.kernels import no sibling, so it
lives beside them)."""
from __future__ import annotations

import math
from typing import List


def normalised_weights(n: int, weights, needs: str, exc=RuntimeError) -> List[float]:
    """n finite weights > 0 (None: uniform), normalised to sum 1 by math.fsum.
    Anything else raises exc(f"{needs}, got {the weights}")."""
    w = [1.0] * n if weights is None else [float(x) for x in weights]
    if len(w) != n or not all(0.0 < x < float("inf") for x in w):
        raise exc(f"{needs}, got {w}")
    total = math.fsum(w)
    return [x / total for x in w]
