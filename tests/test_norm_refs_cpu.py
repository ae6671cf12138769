"""The references, comparators and cases of tests/ref_norm.py, without a GPU:
the float32 PyTorch evaluation of the fused LayerNorm forward and backward,
the column folds and the embedding forward passes every case that
tests/test_gpu_norm.py puts the HIP kernels through, every mutant is rejected
where it applies, the tolerance table is the measured one, the case builders
hold what they promise, the float64 references are
torch.nn.functional.layer_norm and its autograd in float64, and the project's
own CPU paths (models/layers._ln_fwd / _ln_bwd with the Philox mask, EmbedFn)
pass the same comparators."""
import functools
import math

import pytest
import torch

import ref_norm as N
import ref_tail as R
from ref_norm import BF16, F32, F64


def _rejected(fn):
    try:
        fn()
    except R.Mismatch:
        return True
    return False


# --------------------------------------------------------------------------- LayerNorm forward
def _fwd_f32(D, M, p, has_s, save, mutant=None):
    """(what ops.kernels.ln_fwd returns, y before its rounding) of the f32 evaluation."""
    i = N.fwd_inputs(D, M, p)
    y, h, mean, rstd = N.ln_fwd_f32(i.x, i.s if has_s else None, i.gamma, i.beta, i.keep, p, save=save,
                                    mutant=mutant)
    return (y.to(BF16), h, mean if save else None, rstd if save else None), y


def _check_fwd(got, D, M, p, has_s, save, what="f32"):
    i = N.fwd_inputs(D, M, p)
    return N.check_ln_fwd(got, i.x, i.s if has_s else None, i.gamma, i.beta, i.keep, p, save, what)


def _fwd_mutant_applies(mut, D, M, p, has_s, save):
    """Where the mutant changes what is compared by more than the comparators allow."""
    kinds = set(N.fwd_inputs(D, M, p).kinds)
    rounded = bool(kinds & {"plain", "offset", "tiny", "cancel"})  # rows whose x + s needs a rounding
    return {# rstd; y alone stays within its bf16 ulp. (D <= 256: the offset row's sums of squares,
            # multiples of 0.25 below 2^22, are exact in f32)
            "one_pass_var": save and "offset" in kinds and D >= 512,
            "var_over_Dm1": save and kinds != {"const"},
            "eps_outside_sqrt": "tiny" in kinds or (save and "const" in kinds),
            "stats_from_other_h": has_s and ((save and rounded) or (not save and "offset" in kinds)),
            "mask_not_rescaled": p > 0 and rounded,
            "mask_on_x": p > 0 and kinds != {"spike"},
            "lane_order_params": D == 1024}[mut]  # (D = 512: one chunk per lane, RowMap is the identity)


@functools.lru_cache(maxsize=None)
def _fwd_verdicts(D, M):
    out = {m: [] for m in N.LN_FWD_MUTANTS}
    for p, has_s, save in N.fwd_settings():
        what = f"D={D} M={M} p={p} s={has_s} save={save}"
        _check_fwd(_fwd_f32(D, M, p, has_s, save)[0], D, M, p, has_s, save, what)
        for m in N.LN_FWD_MUTANTS:
            got = _fwd_f32(D, M, p, has_s, save, m)[0]
            out[m].append((_rejected(lambda: _check_fwd(got, D, M, p, has_s, save, what)),
                           _fwd_mutant_applies(m, D, M, p, has_s, save), what))
    return out


@pytest.mark.parametrize("M", N.FWD_M)
@pytest.mark.parametrize("D", N.DS)
def test_ln_fwd_f32_accepted_mutants_rejected(D, M):
    for m, res in _fwd_verdicts(D, M).items():
        for rejected, expected, what in res:
            assert rejected or not expected, f"mutant {m} accepted at {what}"


def test_every_ln_fwd_mutant_rejected_somewhere():
    for m in N.LN_FWD_MUTANTS:
        assert any(r for D in (128, 1024) for r, _, _ in _fwd_verdicts(D, 130)[m]), m


def test_hsave_check_is_a_rounding_check():
    """One bf16 ulp off in one element of the stored h is rejected; so is a
    truncation instead of the rounding."""
    D, M, p = 256, 5, 0.1
    i = N.fwd_inputs(D, M, p)
    got, _ = _fwd_f32(D, M, p, True, True)
    h0 = N.ref_ln_fwd(i.x, i.s, i.gamma, i.beta, i.keep, p).h
    N.check_hsave(got[1], h0, i.x, i.s, i.keep, p, "hsave")
    off = got[1].clone()
    off[2, 17] = torch.nextafter(off[2, 17], torch.tensor(math.inf, dtype=BF16))
    assert _rejected(lambda: N.check_hsave(off, h0, i.x, i.s, i.keep, p, "one ulp off"))
    trunc = (h0.to(F32).view(torch.int32) & -65536).view(F32).to(BF16)
    assert _rejected(lambda: N.check_hsave(trunc, h0, i.x, i.s, i.keep, p, "truncated"))


# --------------------------------------------------------------------------- LayerNorm backward
def _bwd_keys():
    """The distinct (D, M, p, dres, dbias, accumulate) of every backward case of the GPU file."""
    seen = {}
    for D in N.DS:
        for rpb in N.RPBS:
            for c in N.bwd_cases(D, rpb):
                seen[(c.D, c.M, c.p, c.dres, c.dbias, c.accumulate)] = None
    return list(seen)


OLD = 2.0  # what the accumulating cases add onto


def _bwd_f32(D, M, p, dres, dbias, accumulate, mutant=None):
    """(the dict check_ln_bwd takes, the f32 dh and ds) of the f32 evaluation."""
    i = N.bwd_inputs(D, M, p, dres)
    wrong = N.keep_mask(M, D, p, site=N.SITE + 1)
    o = N.ln_bwd_f32(i.dy, i.hsave, i.mean, i.rstd, i.gamma, i.keep, p, i.dres, mutant, wrong)
    got = {"dh": o["dh"].to(BF16), "ds": o["ds"].to(BF16)}
    for k in ("dgamma", "dbeta") + (("dbias",) if dbias else ()):
        got[k] = o[k] + OLD if accumulate else o[k]
    return got, o


def _check_bwd(got, D, M, p, dres, accumulate, what="f32"):
    i = N.bwd_inputs(D, M, p, dres)
    old = {k: torch.full((D,), OLD) for k in ("dgamma", "dbeta", "dbias")} if accumulate else None
    N.check_ln_bwd(got, i.ref, i.keep, what, old)


def _bwd_mutant_applies(mut, D, M, p, dres, dbias):
    kinds = set(N.bwd_inputs(D, M, p, dres).kinds)
    return {"no_sg": True, "no_sgx": kinds != {"const"},  # (xhat = 0 in a constant row)
            "sums_without_gamma": True, "over_Dm1": True,
            "ds_after_dres": dres, "dbias_from_dh": dbias and (p > 0 or dres),
            "dgamma_with_gamma": kinds != {"const"}, "wrong_mask": p > 0}[mut]


@functools.lru_cache(maxsize=None)
def _bwd_verdicts():
    out = {m: [] for m in N.LN_BWD_MUTANTS}
    for D, M, p, dres, dbias, acc in _bwd_keys():
        what = f"D={D} M={M} p={p} dres={dres} dbias={dbias} acc={acc}"
        _check_bwd(_bwd_f32(D, M, p, dres, dbias, acc)[0], D, M, p, dres, acc, what)
        for m in N.LN_BWD_MUTANTS:
            got = _bwd_f32(D, M, p, dres, dbias, acc, m)[0]
            out[m].append((_rejected(lambda: _check_bwd(got, D, M, p, dres, acc, what)),
                           _bwd_mutant_applies(m, D, M, p, dres, dbias), what))
    return out


def test_ln_bwd_f32_accepted_mutants_rejected():
    for m, res in _bwd_verdicts().items():
        assert any(r for r, _, _ in res), f"mutant {m} never rejected"
        for rejected, expected, what in res:
            assert rejected or not expected, f"mutant {m} accepted at {what}"


def test_bwd_cases_cover_every_option():
    cs = [c for D in N.DS for rpb in N.RPBS for c in N.bwd_cases(D, rpb)]
    for D in N.DS:
        for rpb in N.RPBS:
            mine = [c for c in cs if (c.D, c.rpb) == (D, rpb)]
            assert {c.M for c in mine} == {1, rpb - 1, rpb, rpb + 1, 2 * rpb + 3}
            for f in (lambda c: c.p > 0, lambda c: c.p == 0, lambda c: c.dres, lambda c: not c.dbias,
                      lambda c: not c.want_ds and not c.dbias, lambda c: c.accumulate,
                      lambda c: c.defer and c.dbias, lambda c: c.defer and not c.dbias):
                assert any(f(c) for c in mine), (D, rpb)
            assert any(c.kbits for c in mine) == (D >= 512)
    # over the whole file: all eight (p, dres, dbias) at every kind of M
    for which in range(5):
        combos = {(c.p > 0, c.dres, c.dbias) for c in cs if c.M == N.bwd_ms(c.rpb)[which]}
        assert len(combos) == 8, which


def _chained_f32(D, M):
    """The f32 forward into the f32 backward, checked as the GPU file checks
    the kernels: the backward reference from the forward's own outputs."""
    p = 0.1
    i = N.fwd_inputs(D, M, p)
    (y, h, mean, rstd), _ = _fwd_f32(D, M, p, True, True)
    _check_fwd((y, h, mean, rstd), D, M, p, True, True, "chained forward")
    dy = N.chained_dy(D, M)
    o = N.ln_bwd_f32(dy, h, mean, rstd, i.gamma, i.keep, p)
    ref = N.ref_ln_bwd(dy, h, mean, rstd, i.gamma, i.keep, p)
    got = dict(o, dh=o["dh"].to(BF16), ds=o["ds"].to(BF16))
    N.check_ln_bwd(got, ref, i.keep, f"chained D={D} M={M}")
    return o, ref


@pytest.mark.parametrize("D,M", N.CHAINED)
def test_chained_f32(D, M):
    _chained_f32(D, M)


# --------------------------------------------------------------------------- folds, embedding
def test_fold_f32_accepted_mutants_rejected():
    for beta in (0.0, 1.0):
        items = N.fold_case(beta)
        assert len(items) == N.FOLD_ITEMS > 96 and {p.shape[0] for p, _ in items} == set(N.FOLD_P)
        hit = {m: 0 for m in N.FOLD_MUTANTS}
        for parts, old in items:
            N.check_fold(N.fold_f32(parts, old, beta), parts, old, beta, "fold")
            for m in N.FOLD_MUTANTS:
                rej = _rejected(lambda: N.check_fold(N.fold_f32(parts, old, beta, m), parts, old, beta, m))
                assert rej or (m == "beta_ignored" and beta == 0), (m, beta, parts.shape)
                hit[m] += rej
        assert hit["last_row_dropped"] == N.FOLD_ITEMS and hit["beta_ignored"] == N.FOLD_ITEMS * (beta != 0)


def _embed_settings():
    for D in N.DS:
        for B, L in N.EMBED_BL:
            for p in N.FWD_P:
                tok, table, pe = N.embed_case(D, B, L)
                yield D, B, L, p, tok, table, pe[N.PE_OFF:], N.keep_mask(B * L, D, p)


def test_embed_f32_accepted_mutants_rejected():
    hit = {m: 0 for m in N.EMBED_MUTANTS}
    for D, B, L, p, tok, table, pe, keep in _embed_settings():
        sc = math.sqrt(D)
        what = f"D={D} B={B} L={L} p={p}"
        N.check_embed(N.embed_f32(tok, table, pe, sc, keep, p).to(BF16), tok, table, pe, sc, keep, p, what)
        for m in N.EMBED_MUTANTS:
            got = N.embed_f32(tok, table, pe, sc, keep, p, m).to(BF16)
            rej = _rejected(lambda: N.check_embed(got, tok, table, pe, sc, keep, p, what))
            applies = {"pe_row": B > 1, "scale_on_pe": True, "mask_before_pe": p > 0}[m]
            assert rej or not applies, f"mutant {m} accepted at {what}"
            hit[m] += rej
    assert all(hit.values()), hit


# --------------------------------------------------------------------------- the case builders
def test_ln_rows_hold_what_they_promise():
    eps = R._f32r(N.LN_EPS)
    for D in N.DS:
        for p in N.FWD_P:
            i = N.fwd_inputs(D, 130, p)
            assert set(i.kinds) == set(N.SPECIAL_ROWS) | {"plain"}
            f = N.ref_ln_fwd(i.x, i.s, i.gamma, i.beta, i.keep, p)
            var = ((f.h - f.mean[:, None]) ** 2).mean(-1)
            k = {kind: i.kinds.index(kind) for kind in N.SPECIAL_ROWS}
            assert var[k["const"]] == 0 and f.rstd[k["const"]] == 1 / math.sqrt(eps)
            assert abs(f.mean[k["offset"]] - 100) < 1 and 0.05 < var[k["offset"]] < 1
            assert var[k["tiny"]] < 10 * eps                      # eps is a tenth of var + eps or more
            assert (f.h[k["spike"]] != 0).sum() == 1 and f.h[k["spike"]].max() == 50
            h, x = f.h[k["cancel"]].abs(), i.x[k["cancel"]].double().abs()
            assert h.mean() < 0.02 * x.mean()                     # the rest of a cancellation
            assert f.h[k["huge"]].abs().min() >= N.huge(D) - 8 and i.x[k["huge"]].float().abs().max() <= 1.25 * N.huge(D)
            assert D * float(var[k["huge"]]) < D * (2.5 * N.huge(D)) ** 2 <= 2.0 ** 126  # finite in f32 ...
            assert D * (2.5 * 4 * N.huge(D)) ** 2 > 2.0 ** 128    # ... and two binades more need not be
            assert (i.gamma < 0).sum() == 3 and (i.gamma == 0).sum() == 1
            assert 0.5 <= i.gamma.abs()[i.gamma != 0].min() and i.gamma.abs().max() < 1.5
    for M in N.FWD_M:
        assert len(N.fwd_inputs(128, M, 0.0).kinds) == M


def test_masks_keep_and_drop_in_every_row():
    shapes = {(M, D) for D in N.DS for M in N.FWD_M}
    shapes |= {(c.M, c.D) for D in N.DS for rpb in N.RPBS for c in N.bwd_cases(D, rpb)}
    shapes |= {(B * L, D) for D in N.DS for B, L in N.EMBED_BL} | set((M, D) for D, M in N.CHAINED)
    for M, D in shapes:
        keep = N.keep_mask(M, D, 0.1)
        assert bool(keep.any(-1).all()) and bool((~keep).any(-1).all()), (M, D)
        assert bool(N.keep_mask(M, D, 0.0).all())
        assert not torch.equal(keep, N.keep_mask(M, D, 0.1, site=N.SITE + 1))
        bits = N.pack_bits(keep)
        assert bits.shape == (M, D // 8) and bits.dtype == torch.uint8
        c = 8 * 3 + 5
        assert torch.equal((bits[:, 3] >> 5 & 1).bool(), keep[:, c])


def test_ln_grads_hold_what_they_promise():
    i = N.bwd_inputs(512, 35, 0.1)
    g = i.dy.double() * i.gamma.double()
    xhat = (i.hsave.double() - i.mean.double()[:, None]) * i.rstd.double()[:, None]
    sg, sgx = g.mean(-1).abs(), (g * xhat).mean(-1).abs()
    live = torch.tensor([k != "const" for k in i.kinds])
    assert bool((sg[0::4] > 0.5).all()) and bool((sg[1::2] < 0.3).all())
    assert bool((sgx[2::4][live[2::4]] > 0.5).all()) and bool((sgx[1::2] < 0.3).all())


def test_lane_order_is_the_row_map():
    for D in (512, 1024):
        perm = N.lane_order(D)
        assert sorted(perm.tolist()) == list(range(D))
        vec = D // 64
        for lane, i in ((0, 0), (1, 0), (0, 8 % vec), (63, vec - 1), (5, 9 % vec)):
            assert perm[(i // 8) * 512 + lane * 8 + i % 8] == lane * vec + i
    assert not torch.equal(N.lane_order(1024), torch.arange(1024))
    assert torch.equal(N.lane_order(512), torch.arange(512))


# --------------------------------------------------------------------------- float64 references
@pytest.mark.parametrize("D,p", [(128, 0.0), (256, 0.1), (1024, 0.1)])
def test_references_are_torch_layer_norm_in_float64(D, p):
    M = 130
    i = N.fwd_inputs(D, M, p)
    eps = R._f32r(N.LN_EPS)
    k = i.keep.double() * N._sc(p)
    x, s, gm, bt = (t.double().requires_grad_() for t in (i.x, i.s, i.gamma, i.beta))
    y = torch.nn.functional.layer_norm(x + s * k, (D,), gm, bt, eps)
    f = N.ref_ln_fwd(i.x, i.s, i.gamma, i.beta, i.keep, p)
    assert float(((f.y - y.detach()).abs() / N.y_scale(f, i.gamma, i.beta)).max()) <= 1e-12
    dy = N.ln_grads(M, D, (f.h - f.mean[:, None]) * f.rstd[:, None])
    y.backward(dy.double())
    b = N.ref_ln_bwd(dy, f.h, f.mean, f.rstd, i.gamma, i.keep, p)
    for got, want, scale in ((b.dh, x.grad, b.s_dh), (b.ds, s.grad, b.s_dh), (b.dgamma, gm.grad, b.s_dgamma),
                             (b.dbeta, bt.grad, b.s_dbeta), (b.dbias, s.grad.sum(0), b.s_dbias)):
        assert float(((got - want).abs() / scale).max()) <= 1e-11
    assert bool((b.ds[~i.keep] == 0).all())


# --------------------------------------------------------------------------- the project's CPU paths
def _param(t):
    from tensorflow_distributed_on_gke_amd.models.params import Param

    p = Param(name="p", shape=tuple(t.shape), init=None)
    p.master, p.grad, p.compute = t.clone(), torch.full_like(t, float("nan")), t
    return p


def _rt(p):
    from tensorflow_distributed_on_gke_amd.models.layers import RunCtx

    return RunCtx(training=True, dropout=p, seed=N.SEED, ctr=torch.tensor([N.CTR]))


@pytest.mark.parametrize("D,M", [(128, 130), (256, 37), (1024, 35)])
@pytest.mark.parametrize("p", N.FWD_P)
def test_layers_cpu_layernorm_path(D, M, p):
    """models/layers._ln_fwd / _ln_bwd on CPU tensors. That path saves its h
    in f32: the statistics and y against the reference of that stored h, as
    for the kernels, and the stored h within the f32 roundings of x + s * ks
    (twice h_slack: ks = keep / (1 - p) is rounded from the double 1 / (1 - p)
    there). The backward on reference-built inputs."""
    from tensorflow_distributed_on_gke_amd.models import layers

    i = N.fwd_inputs(D, M, p)
    gm, bt, sb = _param(i.gamma), _param(i.beta), _param(torch.zeros(D))
    y, saved = layers._ln_fwd(i.x.float(), i.s.float(), gm, bt, N.SITE, _rt(p))
    h0 = N.ref_ln_fwd(i.x, i.s, i.gamma, i.beta, i.keep, p).h
    assert saved[0].dtype == F32 and bool(((saved[0].double() - h0).abs() <= 2 * N.h_slack(h0, i.s, i.keep, p)).all())
    ref = N.ref_ln_fwd(i.x, i.s, i.gamma, i.beta, i.keep, p, h_saved=saved[0])
    R.close_f32(saved[1].view(-1), ref.mean, "ln_mean", "cpu mean", scale=ref.src.abs().mean(-1))
    R.close_f32(saved[2].view(-1), ref.rstd, "ln_rstd", "cpu rstd")
    N.close_bf16(y.to(BF16), ref.y, "ln_y", "cpu y", N.y_scale(ref, i.gamma, i.beta))
    b = N.bwd_inputs(D, M, p)
    ks = layers._keep_scale(_rt(p), N.SITE, (M, D), "cpu")
    assert (ks is None) == (p == 0)
    saved = (b.hsave.float(), b.mean.view(-1, 1), b.rstd.view(-1, 1), ks, None)
    gm = _param(b.gamma)
    dh, ds = layers._ln_bwd(b.dy.float(), saved, gm, bt, sb, N.SITE, _rt(p))
    N.check_ln_bwd({"dh": dh.to(BF16), "ds": ds.to(BF16), "dgamma": gm.grad, "dbeta": bt.grad,
                    "dbias": sb.grad}, b.ref, b.keep, "cpu backward")


@pytest.mark.parametrize("p", N.FWD_P)
def test_layers_cpu_embedding_path(p):
    from tensorflow_distributed_on_gke_amd.models.layers import EmbedFn

    for D in (128, 512):
        for B, L in N.EMBED_BL:
            tok, table, pe = N.embed_case(D, B, L)
            out = EmbedFn.apply(torch.zeros((), requires_grad=True), tok, _param(table.float()),
                                pe[N.PE_OFF:], N.SITE, _rt(p))
            N.check_embed(out.detach().to(BF16), tok, table, pe[N.PE_OFF:], math.sqrt(D),
                          N.keep_mask(B * L, D, p), p, f"EmbedFn D={D} B={B}")


# --------------------------------------------------------------------------- the table
BF16_KEYS = ("ln_y", "ln_dh", "ln_ds", "embed")


def _measure_e32():
    """E32 of every entry of ref_norm.E32 over the cases of the GPU file: the
    comparators' own ratio for the f32 outputs, f32_ratio of the value before
    its rounding for the bf16 ones."""
    R.WORST.clear()
    got = {k: 0.0 for k in BF16_KEYS}

    def note(k, v):
        got[k] = max(got[k], v)

    cases = [(D, M, p, has_s, save) for D in N.DS for M in N.FWD_M for p, has_s, save in N.fwd_settings()]
    for D, M, p, has_s, save in cases + [(D, M, 0.1, True, True) for D, M in N.CHAINED]:
        out, y32 = _fwd_f32(D, M, p, has_s, save)
        i = N.fwd_inputs(D, M, p)
        ref = _check_fwd(out, D, M, p, has_s, save)
        scale = N.fwd_y_scale(ref, i.x, i.s if has_s else None, i.gamma, i.beta, i.keep, p, save)
        note("ln_y", N.f32_ratio(y32, ref.y, scale))
    for D, M in N.CHAINED:
        o, ref = _chained_f32(D, M)
        note("ln_dh", N.f32_ratio(o["dh"], ref.dh, ref.s_dh))
        note("ln_ds", N.f32_ratio(o["ds"], ref.ds, ref.s_ds))
    for D, M, p, dres, dbias, acc in _bwd_keys():
        out, o = _bwd_f32(D, M, p, dres, dbias, acc)
        _check_bwd(out, D, M, p, dres, acc)
        ref = N.bwd_inputs(D, M, p, dres).ref
        note("ln_dh", N.f32_ratio(o["dh"], ref.dh, ref.s_dh))
        note("ln_ds", N.f32_ratio(o["ds"], ref.ds, ref.s_ds))
    for beta in (0.0, 1.0):
        for parts, old in N.fold_case(beta):
            N.check_fold(N.fold_f32(parts, old, beta), parts, old, beta, "fold")
    for D, B, L, p, tok, table, pe, keep in _embed_settings():
        ref, s = N.ref_embed_fwd(tok, table, pe, math.sqrt(D), keep, p)
        note("embed", N.f32_ratio(N.embed_f32(tok, table, pe, math.sqrt(D), keep, p), ref, s))
    got.update({k: v for k, v in R.WORST.items() if k not in BF16_KEYS})
    return got


def test_e32_table_is_measured():
    """Every tolerance is 8 x an E32 that this machine reproduces: not below
    what the float32 evaluation needs, and not inflated."""
    got = _measure_e32()
    print("measured E32:", {k: f"{v:.2e}" for k, v in sorted(got.items())})
    assert set(got) == set(N.E32)
    for k, e in N.E32.items():
        # (the same bounds as tests/test_loss_optim_refs_cpu.py::test_e32_table_is_measured)
        assert got[k] <= 1.5 * e, f"{k}: measured {got[k]:.3e} above the table's {e:.3e}"
        assert got[k] >= e / 4, f"{k}: the table's {e:.3e} is more than 4x the measured {got[k]:.3e}"
    assert N.MARGIN == 8.0 and all(math.isclose(R.tol(k), 8 * e) for k, e in N.E32.items())
    assert not set(N.E32) & set(R.E32)
