"""Float64 references, comparators, case builders and mutants for the fused
residual + dropout + LayerNorm kernels (csrc/kernels/norm.hip,
csrc/include/tdg_ln.h), the deferred column folds (reduce_partials_multi) and
the embedding forward (csrc/kernels/embed.hip). No GPU needed.

Built like tests/ref_tail.py, whose comparators and bookkeeping it reuses: the
references start from exactly what the kernels get (bf16 tensors, f32 gamma /
beta / mean / rstd, f32-rounded p and eps, the Philox keep mask) and evaluate
in float64. The `*_f32` functions are the straightforward float32 PyTorch
evaluation (two-pass variance, torch.rsqrt, f32 sums in row order); with
`mutant=...` they are deliberately wrong in one line.
tests/test_norm_refs_cpu.py shows that the comparators accept the former and
reject every mutant, so tests/test_gpu_norm.py, which puts the HIP kernels
through the same comparators, cannot pass vacuously.
"""
from __future__ import annotations

import functools
import math
from collections import namedtuple
from dataclasses import dataclass

import torch

import ref_tail as R
from ref_tail import BF16, BF16_ULP, F32, F64, MARGIN, Mismatch, close_f32, exact, tol  # noqa: F401
from tensorflow_distributed_on_gke_amd.ops import philox

# --------------------------------------------------------------------------- tolerances
# f32 outputs: ref_tail.close_f32, |got - ref| <= tol * (|ref| + scale). bf16
# outputs: close_bf16 below, |got - ref| <= 2^-8 |ref| + tol * scale. tol = 8 *
# E32, `scale` the magnitude of the operands the value is formed from (given
# at each entry).
#
# E32 is the worst ratio of the float32 PyTorch evaluation (`*_f32` below; for
# a bf16 output its f32 value before the rounding, which 2^-8 |ref| covers)
# against the float64 reference over all cases of tests/test_gpu_norm.py,
# measured on the CPU by test_norm_refs_cpu.py::test_e32_table_is_measured.
# The margin of 8 is for the kernels' rsqrtf and their other summation order
# (wave DPP sums, 4- or 8-wave LDS folds, 16-way partial lanes). `kernel` is
# the worst ratio of the HIP kernels on the MI355X over the same cases, in the
# same unit (for a bf16 output: what of its error 2^-8 |ref| does not cover).
#
#   entry          E32        kernel     what
E32 = {
    "ln_mean":    8.2e-9,   # 8.2e-9   row mean; scale = mean|h| of the row
    "ln_rstd":    1.5e-7,   # 1.6e-7   row 1 / sqrt(var + eps); scale = 0
    "ln_y":       2.6e-7,   # 3.4e-8   y (bf16); scale = |gamma| rstd (|h| + |mean|) + |beta| (save=False: y_scale)
    "ln_dh":      3.6e-6,   # 8.4e-8   dh (bf16); scale = rstd (|dy gamma| + |sg| + |xhat sgx|) + |dres|
    "ln_ds":      3.6e-6,   # 8.4e-8   ds (bf16); scale = the same bracket * keep / (1 - p)
    "ln_dgamma":  1.1e-7,   # 9.5e-8   scale = sum over rows |dy xhat| (+ |old| when accumulating)
    "ln_dbeta":   2.9e-8,   # 2.2e-8   scale = sum over rows |dy| (+ |old|)
    "ln_dbias":   1.6e-7,   # 1.7e-7   column sums of the unrounded ds; scale = sum over rows of the ds scale (+ |old|)
    "fold":       1.5e-7,   # 1.5e-7   reduce_partials_multi; scale = |beta out_old| + sum |parts|
    "embed":      1.9e-7,   # 0        embedding output (bf16); scale = (|table| scale + |pe|) / (1 - p)
}
# (ln_dh / ln_ds: sg and sgx are means that cancel; where they come out small, and gamma = 0 leaves
# them alone in the bracket, their own f32 rounding is many times 1e-7 of it. The sharp check of the
# row arithmetic is ln_dbias, the column sums of the f32 ds.)
R.register(E32)

LN_EPS = 1e-6
SEED, CTR, SITE = 1234, 5, 7  # the dropout stream of every case (a non-zero device counter)
DS = (128, 256, 512, 1024)


def _fail(what, msg):
    raise Mismatch(f"{what}: {msg}")


def _sc(p: float) -> float:
    """The kept elements' multiplier 1 / (1 - p), p as the f32 the kernels get."""
    return 1.0 / (1.0 - R._f32r(p)) if p > 0 else 1.0


@functools.lru_cache(maxsize=None)
def keep_mask(M, D, p, seed=SEED, ctr=CTR, site=SITE):
    """Boolean [M, D]: the kernels' Philox keep decisions (all True at p = 0)."""
    if p <= 0:
        return torch.ones(M, D, dtype=torch.bool)
    return philox.keep_mask(seed, philox.rng_offset(ctr, site), M * D, p).view(M, D).clone()


def pack_bits(keep):
    """The keep bitmap the kernels write: uint8 [M, D / 8], bit c % 8 of byte c / 8 = column c."""
    M, D = keep.shape
    w = 1 << torch.arange(8, dtype=torch.int64)
    return (keep.view(M, D // 8, 8).to(torch.int64) * w).sum(-1).to(torch.uint8)


# --------------------------------------------------------------------------- comparators
def close_bf16(got, ref, key, what, scale, zero=None):
    """A bf16 output against its float64 reference, every element:
    |got - ref| <= 2^-8 |ref| + tol(key) * scale; the elements of `zero`
    (boolean) exactly +-0. Returns the worst (err - 2^-8 |ref|) / scale."""
    if got.dtype != BF16:
        _fail(what, f"dtype {got.dtype}")
    g = got.detach().cpu().to(F64)
    if g.shape != ref.shape:
        _fail(what, f"shape {tuple(g.shape)} vs {tuple(ref.shape)}")
    if not bool(torch.isfinite(g).all()):
        _fail(what, "non-finite values")
    if zero is not None and bool((g[zero] != 0).any()):
        _fail(what, "dropped elements not zero")
    over = ((g - ref).abs() - BF16_ULP * ref.abs()).clamp_min(0)
    scale = torch.as_tensor(scale, dtype=F64).expand_as(over)
    ratio = torch.where(over > 0, over / scale.clamp_min(1e-300), torch.zeros_like(over))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    R._note(key, worst)
    if worst > tol(key):
        i = int(ratio.argmax())
        _fail(what, f"[{key}] element {i}: got {g.flatten()[i].item()!r} ref {ref.flatten()[i].item()!r}, "
                    f"excess {worst:.3e} > {tol(key):.3e} (x scale {scale.flatten()[i].item():.3e})")
    return worst


def f32_ratio(val, ref, scale):
    """Worst |val - ref| / scale of a bf16 output's f32 value before its rounding: the unit of its E32."""
    err = (val.to(F64) - ref).abs()
    scale = torch.as_tensor(scale, dtype=F64).expand_as(err)
    r = torch.where(err > 0, err / scale.clamp_min(1e-300), torch.zeros_like(err))
    return float(r.max()) if r.numel() else 0.0


def h_slack(h, s, keep, p):
    """How far the f32 x + s * sc may lie from the float64 h: half an ulp of t
    = s * sc, half an ulp of the sum, and the rounding of sc = 1 / (1 - p) itself."""
    t = s.to(F64) * keep.to(F64) * _sc(p)
    return 0.5 * R.ulp32(t) + 0.5 * R.ulp32(h) + t.abs() * 2.0 ** -24


def check_hsave(got, h, x, s, keep, p, what):
    """The stored bf16 h is a correct rounding of the float64 h, up to the f32
    roundings on the way: h = x exactly without s; else t = s * sc and x + t
    are rounded once each (one rounding when contracted into an FMA), and sc
    is itself an f32. Exact otherwise: `got` must be the bf16 nearest to some
    value within that distance of h."""
    if got.dtype != BF16:
        _fail(what, f"dtype {got.dtype}")
    got = got.detach().cpu()
    if s is None:
        return exact(got, x, what)
    if got.shape != h.shape:
        _fail(what, f"shape {tuple(got.shape)} vs {tuple(h.shape)}")
    if not bool(torch.isfinite(got.float()).all()):
        _fail(what, "non-finite values")
    d = h_slack(h, s, keep, p)
    inf = torch.full_like(got, math.inf)
    g = got.to(F64)
    lo = (g + torch.nextafter(got, -inf).to(F64)) / 2  # the values that round to `got`
    hi = (g + torch.nextafter(got, inf).to(F64)) / 2
    bad = (h + d < lo) | (h - d > hi)
    if bool(bad.any()):
        i = int(bad.flatten().nonzero()[0])
        _fail(what, f"{int(bad.sum())} elements are no rounding of h, first at {i}: "
                    f"{g.flatten()[i].item()!r} vs {h.flatten()[i].item()!r}")


# --------------------------------------------------------------------------- LayerNorm forward
LnFwd = namedtuple("LnFwd", "h mean rstd y src")


def ref_ln_fwd(x, s, gamma, beta, keep, p, eps=LN_EPS, h_saved=None):
    """h = x + s * keep / (1 - p) (s None: h = x); mean, rstd = 1 / sqrt(var +
    eps) and y = (h - mean) * rstd * gamma + beta of `src`: the bf16 h the
    kernel stored (h_saved: what its backward will see), else the float64 h
    (save=False). All float64."""
    h = x.to(F64)
    if s is not None:
        h = h + s.to(F64) * keep.to(F64) * _sc(p)
    src = h if h_saved is None else h_saved.detach().cpu().to(F64)
    mean = src.mean(-1)
    d = src - mean[:, None]
    rstd = 1.0 / torch.sqrt((d * d).mean(-1) + R._f32r(eps))
    y = d * rstd[:, None] * gamma.to(F64) + beta.to(F64)
    return LnFwd(h, mean, rstd, y, src)


def y_scale(ref: LnFwd, gamma, beta, a=None):
    """|gamma| rstd (|h| + |mean|) + |beta|, h the stored one that the
    statistics and y were formed from. a (save=False): there no h is ever
    stored, y is formed from x and t = s keep / (1 - p) themselves, and the f32
    sum x + t is off by a rounding of |x| + |t|, which a cancelling row makes
    many times |h|: the same formula on the operands, a = |x| + |t| for |h|
    and its row mean for |mean|. (Measured against |h| there, the f32
    evaluation itself is off by 1.4e-3 of the scale on the `cancel` row of
    ln_rows, 5000 times its error anywhere else: no f32 code could be held to
    it. With a saved h the kernel's rounded h is the operand and |h| stands.)"""
    if a is None:
        a, am = ref.src.abs(), ref.mean.abs()
    else:
        am = a.mean(-1)
    return gamma.to(F64).abs() * ref.rstd[:, None] * (a + am[:, None]) + beta.to(F64).abs()


def h_operands(x, s, keep, p):
    """|x| + |s keep / (1 - p)|: what the f32 h of the save=False arm is a sum of."""
    a = x.to(F64).abs()
    return a if s is None else a + (s.to(F64) * keep.to(F64) * _sc(p)).abs()


def lane_order(D):
    """perm[column] = the index a lane-major walk (lane * VEC + i) gives that
    column under tdg_ln.h RowMap: columns (i / 8) * 512 + lane * 8 + i % 8."""
    vec = D // 64
    lane = torch.arange(64).view(64, 1)
    i = torch.arange(vec).view(1, vec)
    w = min(vec, 8)
    col = (i // w) * (64 * w) + lane * w + i % w
    perm = torch.empty(D, dtype=torch.int64)
    perm[col.flatten()] = (lane * vec + i).flatten()
    return perm


LN_FWD_MUTANTS = ("one_pass_var", "var_over_Dm1", "eps_outside_sqrt", "stats_from_other_h",
                  "mask_not_rescaled", "mask_on_x", "lane_order_params")


def ln_fwd_f32(x, s, gamma, beta, keep, p, eps=LN_EPS, save=True, mutant=None):
    """The float32 PyTorch evaluation. Returns (y f32, h bf16 or None, mean, rstd)."""
    assert mutant is None or mutant in LN_FWD_MUTANTS
    D = x.shape[-1]
    h = x.to(F32)
    if s is not None:
        k = keep.to(F32)
        sc = 1 / (1 - torch.tensor(p, dtype=F32)) if p > 0 and mutant != "mask_not_rescaled" else 1.0
        if mutant == "mask_on_x":
            h = h * k
        h = h + s.to(F32) * k * sc
    hb = h.to(BF16)
    src = hb.to(F32) if save != (mutant == "stats_from_other_h") else h
    mean = src.sum(-1) / D
    d = src - mean[:, None]
    var = (d * d).sum(-1) / (D - 1 if mutant == "var_over_Dm1" else D)
    if mutant == "one_pass_var":
        var = (src * src).sum(-1) / D - mean * mean
    e = torch.tensor(eps, dtype=F32)
    rstd = 1 / (torch.sqrt(var) + e) if mutant == "eps_outside_sqrt" else torch.rsqrt(var + e)
    if mutant == "lane_order_params" and D >= 512:
        gamma, beta = gamma[lane_order(D)], beta[lane_order(D)]
    y = d * rstd[:, None] * gamma + beta
    return y, (hb if save else None), mean, rstd


def check_ln_fwd(got, x, s, gamma, beta, keep, p, save, what, eps=LN_EPS):
    """got = (y bf16, hsave bf16, mean, rstd) as ops.kernels.ln_fwd returns
    them (the last three None with save=False). Returns the reference."""
    y, h, mean, rstd = got
    if save:
        h0 = ref_ln_fwd(x, s, gamma, beta, keep, p, eps).h
        check_hsave(h, h0, x, s, keep, p, what + " hsave")
        ref = ref_ln_fwd(x, s, gamma, beta, keep, p, eps, h_saved=h)
        close_f32(mean.detach().cpu(), ref.mean, "ln_mean", what + " mean", scale=ref.src.abs().mean(-1))
        close_f32(rstd.detach().cpu(), ref.rstd, "ln_rstd", what + " rstd")
    else:
        if h is not None or mean is not None or rstd is not None:
            _fail(what, "save=False returned saved tensors")
        ref = ref_ln_fwd(x, s, gamma, beta, keep, p, eps)
    close_bf16(y, ref.y, "ln_y", what + " y", fwd_y_scale(ref, x, s, gamma, beta, keep, p, save))
    return ref


def fwd_y_scale(ref, x, s, gamma, beta, keep, p, save):
    return y_scale(ref, gamma, beta, None if save else h_operands(x, s, keep, p))


# --------------------------------------------------------------------------- LayerNorm backward
LnBwd = namedtuple("LnBwd", "dh ds dgamma dbeta dbias s_dh s_ds s_dgamma s_dbeta s_dbias")


def ref_ln_bwd(dy, hsave, mean, rstd, gamma, keep, p, dres=None):
    """With xhat = (h - mean) rstd, g = dy gamma, sg = mean g, sgx = mean g xhat:
    dh0 = rstd (g - sg - xhat sgx); ds = dh0 keep / (1 - p); dh = dh0 + dres;
    dgamma = sum dy xhat, dbeta = sum dy, dbias = sum ds over rows. Float64,
    with the scale of each output (header of this file)."""
    dy, h, gm = dy.to(F64), hsave.to(F64), gamma.to(F64)
    m, r = mean.to(F64)[:, None], rstd.to(F64)[:, None]
    xhat = (h - m) * r
    g = dy * gm
    sg = g.mean(-1, keepdim=True)
    sgx = (g * xhat).mean(-1, keepdim=True)
    dh = r * (g - sg - xhat * sgx)
    k = keep.to(F64) * _sc(p)
    ds = dh * k
    br = r * (g.abs() + sg.abs() + (xhat * sgx).abs())
    s_dh = br
    if dres is not None:
        dh = dh + dres.to(F64)
        s_dh = br + dres.to(F64).abs()
    return LnBwd(dh, ds, (dy * xhat).sum(0), dy.sum(0), ds.sum(0), s_dh, br * k,
                 (dy * xhat).abs().sum(0), dy.abs().sum(0), (br * k).sum(0))


LN_BWD_MUTANTS = ("no_sg", "no_sgx", "sums_without_gamma", "over_Dm1", "ds_after_dres",
                  "dbias_from_dh", "dgamma_with_gamma", "wrong_mask")


def ln_bwd_f32(dy, hsave, mean, rstd, gamma, keep, p, dres=None, mutant=None, keep_wrong=None):
    """The float32 PyTorch evaluation. Returns a dict of f32 tensors dh, ds,
    dgamma, dbeta, dbias (dh and ds before their bf16 rounding)."""
    assert mutant is None or mutant in LN_BWD_MUTANTS
    D = dy.shape[-1]
    dy, h = dy.to(F32), hsave.to(F32)
    r = rstd.to(F32)[:, None]
    xhat = (h - mean.to(F32)[:, None]) * r
    g = dy * gamma
    n = D - 1 if mutant == "over_Dm1" else D
    a = dy if mutant == "sums_without_gamma" else g
    sg = 0.0 if mutant == "no_sg" else a.sum(-1, keepdim=True) / n
    sgx = 0.0 if mutant == "no_sgx" else (a * xhat).sum(-1, keepdim=True) / n
    dh0 = r * (g - sg - xhat * sgx)
    sc = 1 / (1 - torch.tensor(p, dtype=F32)) if p > 0 else 1.0
    k = (keep_wrong if mutant == "wrong_mask" else keep).to(F32) * sc
    dh = dh0 if dres is None else dh0 + dres.to(F32)
    ds = (dh if mutant == "ds_after_dres" else dh0) * k
    return {"dh": dh, "ds": ds,
            "dgamma": ((g if mutant == "dgamma_with_gamma" else dy) * xhat).sum(0),
            "dbeta": dy.sum(0),
            "dbias": (dh if mutant == "dbias_from_dh" else ds).sum(0)}


def check_ln_bwd(got, ref: LnBwd, keep, what, old=None):
    """got: dict with dh, dgamma, dbeta and, where the call produced them, ds
    and dbias. old: what the three column sums were accumulated onto."""
    close_bf16(got["dh"], ref.dh, "ln_dh", what + " dh", ref.s_dh)
    if got.get("ds") is not None:
        close_bf16(got["ds"], ref.ds, "ln_ds", what + " ds", ref.s_ds, zero=~keep)
    for name in ("dgamma", "dbeta", "dbias"):
        if got.get(name) is None:
            continue
        want, scale = getattr(ref, name), getattr(ref, "s_" + name)
        if old is not None:
            want, scale = want + old[name].to(F64), scale + old[name].to(F64).abs()
        close_f32(got[name].detach().cpu(), want, "ln_" + name, f"{what} {name}", scale=scale)


# --------------------------------------------------------------------------- folds
def ref_fold(parts, out_old, beta):
    """beta * out_old + the column sums of parts [P, N], float64."""
    return R._f32r(beta) * out_old.to(F64) + parts.to(F64).sum(0)


def fold_scale(parts, out_old, beta):
    return (R._f32r(beta) * out_old.to(F64)).abs() + parts.to(F64).abs().sum(0)


FOLD_MUTANTS = ("beta_ignored", "last_row_dropped")


def fold_f32(parts, out_old, beta, mutant=None):
    assert mutant is None or mutant in FOLD_MUTANTS
    p = parts[:-1] if mutant == "last_row_dropped" else parts
    b = 0.0 if mutant == "beta_ignored" else beta
    return (b * out_old if b != 0 else torch.zeros_like(out_old)) + p.to(F32).sum(0)


def check_fold(got, parts, out_old, beta, what):
    close_f32(got.detach().cpu(), ref_fold(parts, out_old, beta), "fold", what,
              scale=fold_scale(parts, out_old, beta))


FOLD_N, FOLD_ITEMS, FOLD_P = 132, 100, (1, 15, 16, 17, 513)  # N % 4 == 0 with a partial 64-column strip


@functools.lru_cache(maxsize=None)
def fold_case(beta, seed=0):
    """100 (parts [P, N], out_old [N]) of one (N, beta): more than one launch
    holds. Partial rows of mixed magnitudes and signs, so that columns cancel."""
    g = torch.Generator().manual_seed(977 + seed + int(beta))
    items = []
    for i in range(FOLD_ITEMS):
        P = FOLD_P[i % len(FOLD_P)]
        mag = 10.0 ** (4 * torch.rand(P, 1, generator=g) - 2)
        items.append((torch.randn(P, FOLD_N, generator=g) * mag, torch.randn(FOLD_N, generator=g) * 3))
    return items


# --------------------------------------------------------------------------- embedding forward
def ref_embed_fwd(tok, table, pe, scale, keep, p):
    """(table[tok] * scale + pe[row % L]) * keep / (1 - p) for tok [B, L],
    float64 [B * L, D], and its scale."""
    L = tok.shape[1]
    t = tok.reshape(-1).to(torch.int64)
    pos = torch.arange(t.numel()) % L
    sc, k = R._f32r(scale), keep.to(F64) * _sc(p)
    e, pp = table.to(F64)[t], pe.to(F64)[pos]
    return (e * sc + pp) * k, (e.abs() * sc + pp.abs()) * _sc(p)


EMBED_MUTANTS = ("pe_row", "scale_on_pe", "mask_before_pe")


def embed_f32(tok, table, pe, scale, keep, p, mutant=None):
    """The float32 PyTorch evaluation (before the bf16 rounding)."""
    assert mutant is None or mutant in EMBED_MUTANTS
    L = tok.shape[1]
    t = tok.reshape(-1).to(torch.int64)
    rows = torch.arange(t.numel())
    pp = pe[rows if mutant == "pe_row" else rows % L]
    sc = torch.tensor(scale, dtype=F32)
    k = keep.to(F32) * (1 / (1 - torch.tensor(p, dtype=F32)) if p > 0 else 1.0)
    e = table.to(F32)[t]
    if mutant == "scale_on_pe":
        return (e + pp) * sc * k
    if mutant == "mask_before_pe":
        return e * sc * k + pp
    return (e * sc + pp) * k


def check_embed(got, tok, table, pe, scale, keep, p, what):
    ref, s = ref_embed_fwd(tok, table, pe, scale, keep, p)
    close_bf16(got.reshape(ref.shape), ref, "embed", what, s, zero=~keep)


EMBED_V, EMBED_BL, PE_OFF, PE_LEN = 53, ((3, 37), (1, 1)), 5, 128


def sinusoid(n, D, start=0):
    """Interleaved sin / cos position table rows start .. start + n (f32)."""
    pos = torch.arange(start, start + n, dtype=F64).view(-1, 1)
    i = torch.arange(D).view(1, -1)
    ang = pos / torch.pow(torch.tensor(10000.0, dtype=F64), (2 * (i // 2)).to(F64) / D)
    return torch.where(i % 2 == 0, torch.sin(ang), torch.cos(ang)).to(F32)


@functools.lru_cache(maxsize=None)
def embed_case(D, B, L, seed=0):
    """tok [B, L] with ids 0 and V - 1 present (V - 1 alone when B * L = 1), a
    bf16 table of mixed row magnitudes, and pe with PE_OFF + PE_LEN rows: the
    kernels get pe[PE_OFF:], as the decoder passes an offset view."""
    g = torch.Generator().manual_seed(31 * D + 7 * B + L + seed)
    tok = torch.randint(0, EMBED_V, (B, L), generator=g)
    tok.view(-1)[0] = 0
    tok.view(-1)[-1] = EMBED_V - 1
    mag = 10.0 ** (2 * torch.rand(EMBED_V, 1, generator=g) - 2)
    table = (torch.randn(EMBED_V, D, generator=g) * mag).to(BF16)
    return tok, table, sinusoid(PE_OFF + PE_LEN, D)


# --------------------------------------------------------------------------- LayerNorm cases
SPECIAL_ROWS = ("const", "offset", "tiny", "tiny", "spike", "cancel", "huge")


def huge(D):
    """The largest power of two H with D * (2.5 H)^2 <= 2^126: rows of |x| in
    [H, 1.25 H) of either sign keep their f32 sum of squared deviations finite."""
    return 2.0 ** math.floor(0.5 * (126 - math.log2(D)) - math.log2(2.5))


def ln_rows(M, D, seed=0, keep=None, p=0.0):
    """x, s (bf16 [M, D]), gamma, beta (f32 [D]) and the kind of every row.
    gamma in [0.5, 1.5) with three negative entries and one zero. The rows are
    the special ones (M >= 9: all of them; below that the first M of their
    shuffle with two ordinary rows) among ordinary N(0, 1) rows:
      const   x constant, s = 0: var = 0, rstd = 1 / sqrt(eps)
      offset  x = 100 + 0.5 n: a one-pass variance cancels
      tiny    magnitude 1e-3: eps matters
      spike   one 50 in a zero row
      cancel  x = 1e-3 n - s keep / (1 - p): h is the small rest of a cancellation
      huge    |x| in [H, 1.25 H), H = huge(D) (2^56 at D = 1024): the largest magnitudes whose
              variance stays finite in f32
    keep / p: the mask of the case (for `cancel`)."""
    g = torch.Generator().manual_seed(100003 * seed + 131 * M + D)
    n = max(M, len(SPECIAL_ROWS) + 2)
    kinds = list(SPECIAL_ROWS) + ["plain"] * (n - len(SPECIAL_ROWS))
    kinds = [kinds[i] for i in torch.randperm(n, generator=g).tolist()[:M]]
    x = torch.randn(M, D, generator=g)
    s = torch.randn(M, D, generator=g)
    k = torch.ones(M, D) if keep is None else keep.to(F32) * _sc(p)
    for r, kind in enumerate(kinds):
        if kind == "const":
            x[r], s[r] = 3.25, 0.0
        elif kind == "offset":
            x[r] = 100 + 0.5 * x[r]
            s[r] = 0.5 * s[r]
        elif kind == "tiny":
            x[r] *= 1e-3
            s[r] *= 1e-3
        elif kind == "spike":
            x[r], s[r] = 0.0, 0.0
            x[r, int(torch.randint(0, D, (1,), generator=g))] = 50.0
        elif kind == "cancel":
            x[r] = 1e-3 * x[r] - s[r].to(BF16).to(F32) * k[r]
        elif kind == "huge":
            x[r] = torch.sign(x[r]) * huge(D) * (1 + 0.25 * torch.rand(D, generator=g))
    gamma = torch.rand(D, generator=g) + 0.5
    idx = torch.randperm(D, generator=g)[:4]
    gamma[idx[:3]] *= -1
    gamma[idx[3]] = 0.0
    return x.to(BF16), s.to(BF16), gamma, torch.randn(D, generator=g), kinds


def ln_grads(M, D, xhat, seed=0):
    """dy (bf16 [M, D]): of every four rows one with a common offset (dy = 1 +
    0.1 n: sg is large), one correlated with xhat (dy = xhat + 0.1 n: sgx is
    large), two ordinary. In the first two kinds dh is a small difference of
    large terms."""
    g = torch.Generator().manual_seed(7919 * seed + 17 * M + D)
    n = torch.randn(M, D, generator=g)
    dy = n.clone()
    dy[0::4] = 1 + 0.1 * n[0::4]
    dy[2::4] = xhat.to(F32)[2::4] + 0.1 * n[2::4]
    return dy.to(BF16)


FwdIn = namedtuple("FwdIn", "x s gamma beta keep kinds")
FWD_M = (1, 3, 5, 130)
FWD_P = (0.0, 0.1)


@functools.lru_cache(maxsize=None)
def fwd_inputs(D, M, p):
    keep = keep_mask(M, D, p)
    x, s, gamma, beta, kinds = ln_rows(M, D, 0, keep, p)
    return FwdIn(x, s, gamma, beta, keep, kinds)


def fwd_settings():
    """(p, has_s, save) of every forward case of one (D, M): dropout needs s."""
    return [(p, has_s, save) for p in FWD_P for has_s in (True, False) for save in (True, False)
            if has_s or p == 0]


BwdIn = namedtuple("BwdIn", "dy hsave mean rstd gamma keep dres ref kinds")


@functools.lru_cache(maxsize=None)
def bwd_inputs(D, M, p, dres=False):
    """Reference-built backward inputs: hsave, mean and rstd are ref_ln_fwd's,
    rounded to their storage types, so that a forward error neither hides nor
    causes a backward failure. ref: ref_ln_bwd of exactly these."""
    keep = keep_mask(M, D, p)
    x, s, gamma, beta, kinds = ln_rows(M, D, 1, keep, p)
    hsave = ref_ln_fwd(x, s, gamma, beta, keep, p).h.to(F32).to(BF16)
    f = ref_ln_fwd(x, s, gamma, beta, keep, p, h_saved=hsave)
    mean, rstd = f.mean.to(F32), f.rstd.to(F32)
    xhat = (hsave.to(F64) - mean.to(F64)[:, None]) * rstd.to(F64)[:, None]
    dy = ln_grads(M, D, xhat, 1)
    e = None
    if dres:
        g = torch.Generator().manual_seed(5 * M + D)
        e = torch.randn(M, D, generator=g).to(BF16)
    return BwdIn(dy, hsave, mean, rstd, gamma, keep, e,
                 ref_ln_bwd(dy, hsave, mean, rstd, gamma, keep, p, e), kinds)


RPBS = (16, 32, 64)


def bwd_ms(rpb):
    """M = rpb + 1: the last workgroup has one live row, its other waves idle
    and (iters > 1) its later row groups past M; 2 * rpb + 3: a partial RPW
    group in the middle of a wave."""
    return (1, rpb - 1, rpb, rpb + 1, 2 * rpb + 3)


@dataclass(frozen=True)
class BwdCase:
    D: int
    rpb: int
    M: int
    p: float
    dres: bool = False
    dbias: bool = True
    want_ds: bool = True
    accumulate: bool = False
    defer: bool = False
    kbits: bool = False  # D >= 512, p > 0: the mask read from the bitmap

    def __str__(self):
        opts = [k for k in ("dres", "dbias", "want_ds", "accumulate", "defer", "kbits") if getattr(self, k)]
        return f"D={self.D} rpb={self.rpb} M={self.M} p={self.p} " + "+".join(opts)


def bwd_cases(D, rpb):
    """Every M of one (D, rpb) with p, dres and dbias alternating (over the
    file all eight combinations at every kind of M), then the options on the
    two M that leave the last workgroup nearly empty and that split a wave's
    row group."""
    out = []
    j = 3 * DS.index(D) + RPBS.index(rpb)
    for i, M in enumerate(bwd_ms(rpb)):
        k = i + 5 * j
        out.append(BwdCase(D, rpb, M, FWD_P[k % 2], dres=k // 2 % 2 == 1, dbias=k // 4 % 2 == 0))
    for M in (rpb + 1, 2 * rpb + 3):
        out += [BwdCase(D, rpb, M, 0.1, dbias=M == rpb + 1, want_ds=False),
                BwdCase(D, rpb, M, 0.1, dres=True, accumulate=True),
                BwdCase(D, rpb, M, 0.1, dbias=M != rpb + 1, defer=True),
                BwdCase(D, rpb, M, 0.0, dres=True, dbias=False, accumulate=True, defer=True)]
        if D >= 512:
            out.append(BwdCase(D, rpb, M, 0.1, dres=M == rpb + 1, kbits=True))
    return out


CHAINED = ((256, 37), (1024, 37))  # (D, M): kernel forward into kernel backward, p = 0.1


@functools.lru_cache(maxsize=None)
def chained_dy(D, M):
    """dy of a chained case: ln_grads around the reference forward's xhat."""
    i = fwd_inputs(D, M, 0.1)
    f = ref_ln_fwd(i.x, i.s, i.gamma, i.beta, i.keep, 0.1)
    return ln_grads(M, D, (f.h - f.mean[:, None]) * f.rstd[:, None], 2)
