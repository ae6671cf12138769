"""LayerNorm family (csrc/kernels/norm.hip): forward, backward and the fold
of deferred column partials."""
from __future__ import annotations

import math
import os

import torch

from tensorflow_distributed_on_gke_amd.ops._ext import C
from tensorflow_distributed_on_gke_amd.ops.kernels.workspace import workspace


def ln_fwd(x, s, gamma, beta, p, seed, ctr, site, eps=1e-6, save=True, y8=None, s8=None,
           amax8=None, kbits=None):
    """y = LN(x + dropout(s)); optionally also y8 = e4m3(y * s8) (fp8 copy,
    amax recorded into amax8) and kbits (uint8 [M, D / 8]): the dropout keep
    mask as a row-major bitmap for a fused backward (dgrad_ln_bwd)."""
    D = x.shape[-1]
    M = x.numel() // D
    y = torch.empty_like(x)
    h = torch.empty_like(x) if save else None
    mean = torch.empty(M, dtype=torch.float32, device=x.device) if save else None
    rstd = torch.empty(M, dtype=torch.float32, device=x.device) if save else None
    C().ln_fwd(x, s, gamma, beta, y, h, mean, rstd, p, seed, ctr, site, eps, y8, s8, amax8, kbits)
    return y, h, mean, rstd


# LayerNorm-backward rows per workgroup (norm.hip ln_bwd_d): 16 on 4 waves,
# 32 / 64 on 8 waves -- fewer dgamma / dbeta partial rows for the fold.
# Measured (profiles/r3s2/ln_rpb.txt): 32 for D <= 512 (base step 5.00-5.02 vs
# 5.02-5.05 ms, LN backward 308 vs 321 us + fold 10.6 vs 20.4 us), 16 for
# D = 1024 (big 13.14-13.19 vs 13.20-13.22 ms); 64 loses 3.5 % (two serial
# row passes). Non-zero LN_BWD_RPB forces one value (tests).
LN_BWD_RPB = int(os.environ.get("TDG_LN_BWD_RPB", "0") or 0)


def ln_bwd_rpb(D: int) -> int:
    return LN_BWD_RPB or (32 if D <= 512 else 16)


def ln_bwd_nparts(M: int, D: int) -> int:
    """Partial-sum rows ln_bwd writes (one per workgroup)."""
    return math.ceil(M / ln_bwd_rpb(D))


def ln_bwd(dy, h, mean, rstd, gamma, dgamma, dbeta, dbias, p, seed, ctr, site, want_ds=True,
           dres=None, accumulate=False, defer=None, ds8=None, s8=None, amax8=None, kbits=None):
    """`defer` (a list): leave the dgamma / dbeta / dbias partial sums in a
    per-site workspace and append their fold to `defer` (run later, all
    LayerNorms of a backward in one launch, by reduce_partials_multi).
    ds8 (e5m2, shape of dy) with scale s8 / amax slot amax8: also the e5m2
    copy of ds for an fp8 backward; with want_ds=False the bf16 ds is then
    not written at all (the bias column sums still come from ds). kbits
    (uint8 [M, D / 8], from ln_fwd): the dropout mask read instead of
    regenerated."""
    D = dy.shape[-1]
    M = dy.numel() // D
    dh = torch.empty_like(dy)
    need_ds = (want_ds and (p > 0 or dres is not None)) or (dbias is not None and ds8 is None)
    ds = torch.empty_like(dy) if need_ds else None
    if defer is None:
        ws = workspace("ln_bwd", 3 * ln_bwd_nparts(M, D) * D, dy.device)
    else:  # partials must survive until the fold: one workspace per site
        ws = workspace(f"ln_bwd_part_{site}", 3 * ln_bwd_nparts(M, D) * D, dy.device)
    C().ln_bwd(dy, h, mean, rstd, gamma, dh, ds, dres, dgamma, dbeta, dbias, ws, p, seed, ctr, site,
               accumulate, defer is not None, ln_bwd_rpb(D), ds8, s8, amax8, kbits)
    if defer is not None:
        nb = ln_bwd_nparts(M, D)
        outs = [dgamma, dbeta] + ([dbias] if dbias is not None else [])
        for i, o in enumerate(outs):
            defer.append((ws[i * nb * D:(i + 1) * nb * D], o, nb, D, 1.0 if accumulate else 0.0))
    if ds is None:
        ds = dh
    return dh, ds


def reduce_partials_multi(items) -> None:
    """Fold deferred (partials, out, nparts, N, beta) column reductions; one
    launch per (N, beta) group of up to 96."""
    groups = {}
    for part, out, nparts, N, beta in items:
        groups.setdefault((N, beta), []).append((part, out, nparts))
    for (N, beta), its in groups.items():
        for c0 in range(0, len(its), 96):
            ch = its[c0:c0 + 96]
            C().reduce_partials_multi([i[0] for i in ch], [i[1] for i in ch], [i[2] for i in ch],
                                      N, beta)
