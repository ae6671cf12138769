"""Case tables and the float64 reference of the sampling step (sample_token),
shared by the CPU and the GPU tests: the CPU file proves every case reachable
and decided and the reference a correct sampler, the GPU file holds the kernel
to it.

The reference implements the definition (ops/kernels/decode.py sample_token) in
float64 with the exact uniforms of ops/philox.py. Two quantities say whether
an f32 implementation must agree with it on a row:

* the gap between the two best Gumbel keys. An f32 key is off by about 1e-5:
  |-log(-log u)| <= 17 at a few ulp (2^-24 * 17 * 4 ~ 4e-6), plus x / T
  (|x| <= 20, T >= 0.7: one ulp of 30 is 2e-6). A row's draw is *decided*
  when the gap is larger than GAP = 1e-3;
* the top-p margin: the distance from top_p to the nearest cumulative
  kept-mass fraction at a value boundary. An f32 mass fraction is off by
  about 2e-6 (about 30 sequential adds per thread at V = 7010, each 2^-24
  relative, and the terms' own rounding). A row's nucleus is decided when
  the margin is larger than P_GAP = 1e-4.

Both constants leave more than 50x headroom.

Inputs are bf16-valued; a case is built once per process and never modified.
"""
import functools
import itertools

import torch

from tensorflow_distributed_on_gke_amd.ops import philox

START, END, PAD = 2, 3, 0  # infer/tokenizer.py
GAP = 1e-3
P_GAP = 1e-4
NINF = float("-inf")

SHAPES = ((7, 8), (300, 304), (7010, 7040))
ROWS = (1, 5, 64)
KINDS = ("random", "ties", "minus_inf")
N_SETTINGS = 6
P_STAR = "p*"  # top_p chosen per case: a midpoint between two boundary fractions near 0.9


def settings(V):
    """(temperature, top_k, top_p) of the table."""
    return [(1.0, 0, 1.0), (0.7, 10, 1.0), (1.3, 0, P_STAR), (0.8, 40, P_STAR), (1.0, 1, 1.0),
            (1.0, V + 5, 1.0)]


CASES = [(V, ldl, R, si, kind) for (V, ldl), R, si, kind in
         itertools.product(SHAPES, ROWS, range(N_SETTINGS), KINDS)]
BIG_CASE = (65536, 65536, 5, 3, "random")  # once: the largest row, 32 loads per thread and pass
# where the kernel changes how it holds a row (in registers up to 2048 and up to
# 8192 columns, re-read beyond): both sides of each threshold
EDGE_CASES = [(V, ldl, 5, si, "random")
              for V, ldl in ((2048, 2048), (2049, 2056), (8192, 8192), (8193, 8200)) for si in (0, 3)]
DIST_ROWS = {7: 20000, 300: 4096, 7010: 4096}
DIST_LDL = dict(SHAPES)


def _bf(x):
    return x.to(torch.bfloat16)


# ---------------------------------------------------------------- the definition, float64
def uniforms(seed, step, row_id, cols):
    """f64 [R, len(cols)]: u = ((w >> 9) + 0.5) * 2^-23, w = word v & 3 of
    Philox(seed, offset = step, idx = row_id << 32 | v >> 2), for v in cols."""
    grp = cols >> 2
    gs = torch.unique(grp)
    idx = (row_id.to(torch.int64).view(-1, 1) << 32) | gs.view(1, -1)
    words = torch.stack(philox.philox4x32(seed, step, idx), dim=2)  # [R, groups, 4]
    w = words[:, torch.searchsorted(gs, grp), cols & 3]
    return ((w >> 9).double() + 0.5) * 2.0 ** -23


def top_k_set(x, top_k):
    """x f64 [V] with a finite entry -> K = {x >= tau_k} (bool [V])."""
    finite = x > NINF
    xs = torch.sort(x[finite], descending=True).values
    tau = xs[top_k - 1] if 0 < top_k < xs.numel() else xs[-1]
    return finite & (x >= tau)


def boundaries(x, T, top_k):
    """(K, the values occurring in K by descending value, the fraction of K's
    mass exp((x - max x) / T) on {x >= value}); the last fraction is 1."""
    K = top_k_set(x, top_k)
    vals, counts = torch.unique(x[K], return_counts=True)
    vals, counts = vals.flip(0), counts.flip(0)
    cum = torch.cumsum(torch.exp((vals - vals[0]) / T) * counts, 0)
    return K, vals, cum / cum[-1]


def kept_set(x, T, top_k, top_p):
    """(S bool [V], top-p margin) of one row with a finite entry."""
    K, vals, frac = boundaries(x, T, top_k)
    if top_p >= 1.0:
        return K, float("inf")
    j = int((frac >= top_p).nonzero()[0])  # tau_p = vals[j]: the largest value reaching top_p
    return K & (x >= vals[j]), float((frac - top_p).abs().min())


def sample_ref(logits, V, score, fin, row_id, T, top_k, top_p, seed, step, shared=False):
    """float64 reference of one step. `shared`: all rows hold the same logits
    (the distribution batches), the kept set is computed once. Returns a dict
    of per-row tensors: token / fin int64, score f64, kept bool [R, V], gap
    (best key minus second best, inf with one kept), margin (top-p), live."""
    R = logits.shape[0]
    x = logits[:, :V].double()
    rid = torch.arange(R) if row_id is None else row_id.long()
    live = (fin == 0) & (score > NINF) & (x > NINF).any(dim=1)
    kept = torch.zeros(R, V, dtype=torch.bool)
    margin = torch.full((R,), float("inf"), dtype=torch.float64)
    if shared:
        assert bool(live.all())
        k0, m0 = kept_set(x[0], T, top_k, top_p)
        kept[:], margin[:] = k0, m0
        cols = k0.nonzero().view(-1)
    else:
        for r in live.nonzero().view(-1).tolist():
            kept[r], margin[r] = kept_set(x[r], T, top_k, top_p)
        cols = torch.arange(V)
    token = torch.full((R,), PAD, dtype=torch.int64)
    gap = torch.full((R,), float("inf"), dtype=torch.float64)
    chunk = max(1, (1 << 21) // max(1, cols.numel()))
    for r0 in range(0, R, chunk):
        sl = slice(r0, min(R, r0 + chunk))
        u = uniforms(seed, step, rid[sl], cols)
        key = x[sl][:, cols] / T - torch.log(-torch.log(u))
        key = torch.where(kept[sl][:, cols], key, torch.full_like(key, NINF))
        best = torch.topk(key, min(2, cols.numel()), dim=1)
        token[sl] = cols[best.indices[:, 0]]
        if cols.numel() > 1:
            gap[sl] = torch.where(best.values[:, 1] > NINF, best.values[:, 0] - best.values[:, 1],
                                  torch.full_like(best.values[:, 0], float("inf")))
    token = torch.where(live, token, torch.full_like(token, PAD))
    gap = torch.where(live, gap, torch.full_like(gap, float("inf")))
    lse = torch.logsumexp(x, dim=1)
    out = score.double() + (x.gather(1, token.view(R, 1)).view(R) - lse)
    out = torch.where(live, out, torch.full_like(out, NINF))
    out = torch.where(fin != 0, score.double(), out)  # ended: unchanged, whatever it is
    o_fin = (~live | (token == END)).long()
    return dict(token=token, fin=o_fin, score=out, kept=kept, gap=gap, margin=margin, live=live)


def decided(ref):
    """bool [R]: rows on which an f32 implementation must give the reference's token."""
    return ref["live"] & (ref["gap"] > GAP) & (ref["margin"] > P_GAP)


def pick_p(logits, V, rows, T, top_k):
    """p*: the midpoint of the widest pair of neighbouring boundary fractions
    (of the given rows, pooled) whose midpoint lies in [0.8, 0.97]; without
    one, the midpoint of the pair around 0.9. Rounded to f32, as it is passed."""
    fr = [torch.tensor([0.0], dtype=torch.float64)]
    for r in rows:
        fr.append(boundaries(logits[r, :V].double(), T, top_k)[2])
    fr = torch.unique(torch.cat(fr))  # ascending, 0 and 1 included
    lo, hi = fr[:-1], fr[1:]
    mid = (lo + hi) / 2
    ok = (mid >= 0.8) & (mid <= 0.97)
    if not bool(ok.any()):
        ok = (lo <= 0.9) & (hi > 0.9)
    width = torch.where(ok, hi - lo, torch.zeros_like(lo))
    return float(torch.tensor(float(mid[int(width.argmax())]), dtype=torch.float32))


def _plant_ties(row, V, top_k):
    """The row maximum twice, and the kk-th largest value three times, so that
    {x >= tau_k} holds more than kk entries (kk = top_k where it cuts)."""
    order = torch.sort(-row[:V].float(), stable=True).indices
    kk = top_k if 0 < top_k <= V - 2 else min(3, V - 2)
    row[order[1]] = row[order[0]]
    if kk >= 3:
        row[order[kk]] = row[order[kk - 1]]
        row[order[kk + 1]] = row[order[kk - 1]]
    else:
        row[order[2]] = row[order[0]]


def _build(V, ldl, R, si, kind, seed0):
    T, top_k, top_p = settings(V)[si]
    for attempt in range(200):
        g = torch.Generator().manual_seed(attempt * 7919 + seed0)
        logits = torch.full((R, ldl), 1e4).to(torch.bfloat16)  # a read past V shows
        logits[:, :V] = _bf(torch.randn(R, V, generator=g) * 3.0)
        score = (-5.0 * torch.rand(R, generator=g)).float()
        fin = torch.zeros(R, dtype=torch.int32)
        row_id = None
        if kind == "random":
            fin[torch.rand(R, generator=g) < 0.3] = 1
            fin[0] = 0
            if R > 1:
                score[1] = NINF  # a dead row among live ones
            row_id = (torch.randperm(R, generator=g) + 1000).to(torch.int32)
        elif kind == "ties":
            for r in range(R):
                _plant_ties(logits[r], V, top_k)
        elif kind == "minus_inf":
            for r in range(R):
                logits[r, torch.randperm(V, generator=g)[: V // 2]] = NINF
            if R > 1:
                logits[R - 1, :V] = NINF  # a row without a finite logit
        x = logits[:, :V].float()
        live = (fin == 0) & (score > NINF) & (x > NINF).any(dim=1)
        p = top_p
        if p == P_STAR:
            p = pick_p(logits, V, live.nonzero().view(-1).tolist(), T, top_k)
        seed = (0xC0FFEE << 40) + 1000 * V + attempt  # more than 32 bits of seed
        step = 3 + si if V < 65536 else (1 << 33) + 5
        ref = sample_ref(logits, V, score, fin, row_id, T, top_k, p, seed, step)
        assert torch.equal(ref["live"], live)
        if bool((decided(ref) == live).all()):
            return dict(logits=logits, score=score, fin=fin, row_id=row_id, T=T, top_k=top_k, top_p=p,
                        seed=seed, step=step, ref=ref)
    raise AssertionError("no seed makes every live row decided")


@functools.lru_cache(maxsize=None)
def sample_case(V, ldl, R, si, kind):
    """Inputs of one case (CPU) and its reference: logits bf16 [R, ldl] with
    +1e4 in the padding columns, score f32 [R], fin int32 [R], row_id int32
    [R] or None, the setting with p* resolved, seed, step. The generator seed
    is the first for which every live row is decided (gap and margin)."""
    return _build(V, ldl, R, si, kind, V + 10 * R + 1000 * si + len(kind))


@functools.lru_cache(maxsize=None)
def dist_case(V, si):
    """The distribution batch: DIST_ROWS[V] rows of the same logits that
    differ only in row_id = 0 .. R - 1; score 0, none ended. Not every row is
    decided (the tests count them)."""
    R, ldl = DIST_ROWS[V], DIST_LDL[V]
    T, top_k, top_p = settings(V)[si]
    g = torch.Generator().manual_seed(77 + V)
    logits = torch.full((R, ldl), 1e4).to(torch.bfloat16)
    logits[:, :V] = _bf(torch.randn(V, generator=g) * 3.0).view(1, V)
    if top_p == P_STAR:
        top_p = pick_p(logits, V, [0], T, top_k)
    score = torch.zeros(R, dtype=torch.float32)
    fin = torch.zeros(R, dtype=torch.int32)
    row_id = torch.arange(R, dtype=torch.int32)
    seed, step = 20240 + V, 11 + si
    ref = sample_ref(logits, V, score, fin, row_id, T, top_k, top_p, seed, step, shared=True)
    return dict(logits=logits, score=score, fin=fin, row_id=row_id, T=T, top_k=top_k, top_p=top_p,
                seed=seed, step=step, ref=ref)


def kept_probs(c):
    """f64 [V]: the distribution a dist_case samples from (kept and renormalised)."""
    V = c["ref"]["kept"].shape[1]
    x = c["logits"][0, :V].double()
    w = torch.where(c["ref"]["kept"][0], torch.exp((x - x.max()) / c["T"]), torch.zeros_like(x))
    return w / w.sum()


def chi_square_z(tokens, probs):
    """(chi^2 - dof) / sqrt(2 dof) of the token counts against `probs`, bins
    of expected count < 5 pooled into one; 0 when a single bin is left."""
    n = tokens.numel()
    counts = torch.bincount(tokens, minlength=probs.numel()).double()
    exp = probs * n
    small = exp < 5
    obs_b, exp_b = counts[~small], exp[~small]
    if bool(small.any()) and float(exp[small].sum()) > 0:
        po, pe = counts[small].sum(), exp[small].sum()
        if float(pe) >= 5 or exp_b.numel() == 0:
            obs_b, exp_b = torch.cat([obs_b, po.view(1)]), torch.cat([exp_b, pe.view(1)])
        else:  # too light for a bin of its own: into the lightest one
            j = int(exp_b.argmin())
            obs_b[j] += po
            exp_b[j] += pe
    dof = exp_b.numel() - 1
    if dof < 1:
        return 0.0
    chi2 = float(((obs_b - exp_b) ** 2 / exp_b).sum())
    return (chi2 - dof) / (2.0 * dof) ** 0.5


# ---------------------------------------------------------------- the decoding loop
def check_steps(tokens, scores, steps, V, n, seed, row_id0, opts, max_length):
    """The loop's bookkeeping, and every step replayed through the float64
    reference on the step's own logits. Returns the share of decided rows."""
    B = tokens.shape[0]
    R = B * n
    hist = tokens.view(R, -1).cpu()
    assert hist.shape[1] == len(steps) + 1 and (hist[:, 0] == START).all()
    fin = torch.zeros(R, dtype=torch.int32)
    score = torch.zeros(R, dtype=torch.float64)
    rid = torch.arange(R, dtype=torch.int32) + row_id0
    n_dec = n_live = 0
    for t, (lg, tok, fin_new) in enumerate(steps):
        lg, tok, fin_new = lg.cpu(), tok.cpu().long(), fin_new.cpu()
        ref = sample_ref(lg, V, score.float(), fin, rid, opts["temperature"], opts["top_k"],
                         opts["top_p"], seed, t)
        dec = decided(ref)
        n_dec, n_live = n_dec + int(dec.sum()), n_live + int(ref["live"].sum())
        assert torch.equal(tok[dec], ref["token"][dec]), f"step {t}"
        assert torch.equal(hist[:, t + 1], tok)
        ended = fin != 0
        assert (tok[ended] == PAD).all() and (fin_new[ended] == 1).all()
        assert torch.equal(fin_new[~ended].long(), (tok[~ended] == END).long())
        x = lg[:, :V].double()
        logp = x.gather(1, tok.view(R, 1)).view(R) - torch.logsumexp(x, dim=1)
        score = torch.where(ended, score, score + logp)
        fin = fin_new
    assert bool(fin.all()) or len(steps) == max_length
    err = (scores.view(R).cpu().double() - score).abs()
    assert (err <= 1e-4 * score.abs().clamp(min=1.0)).all(), "scores are not the running sums"
    return n_dec / max(1, n_live)
