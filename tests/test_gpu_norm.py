"""The fused residual + dropout + LayerNorm kernels (norm.hip, tdg_ln.h), the
deferred column folds and the embedding forward on the MI355X against float64
references: every D, every row-count edge of the forward and backward grids,
with and without residual branch, saved h, dres, dbias, ds, keep bitmap,
accumulation and deferred fold. References, cases, comparators and the
tolerance table are tests/ref_norm.py's; tests/test_norm_refs_cpu.py shows on
the CPU that those comparators reject every mutant listed there.

Which test reaches which arm:
  D = 256 (RowMap<4>, 8-byte accesses)        every test here, at D = 256
  hsave == nullptr (save=False)               test_ln_fwd
  s == nullptr                                test_ln_fwd
  mean / rstd against a reference             test_ln_fwd, test_ln_chained
  forward workgroups with 1 / 3 live waves    test_ln_fwd (M = 1, 3, 5, 130)
  dres                                        test_ln_bwd
  M < rows per block, M % RPW != 0, M = 1,
  row groups past M, the clamped prefetch     test_ln_bwd (M = 1, rpb - 1, rpb, rpb + 1, 2 rpb + 3)
  dbias == nullptr (2-set fold), ds_out null  test_ln_bwd
  constant / offset / tiny / huge rows        every LayerNorm test (ref_norm.ln_rows)
  reduce_partials_multi past 96 items         test_reduce_partials_multi_past_96, ..._refuses_97
  embed_fwd beyond D = 128                    test_embed_fwd
"""
import pytest
import torch

import ref_norm as N
import ref_tail as R
from ref_norm import BF16
from tensorflow_distributed_on_gke_amd.ops import kernels as kk
from tensorflow_distributed_on_gke_amd.ops.kernels import layernorm

pytestmark = pytest.mark.gpu
DEV = "cuda"
OLD = 2.0  # what the accumulating cases add onto


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    print("\nkernel worst / tolerance (unit of ref_norm.E32 x 8):", R.report())


def _dev(t):
    return None if t is None else t.to(DEV)


def _cpu(ts):
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu() for t in ts)


def _ctr():
    return torch.tensor([N.CTR], dtype=torch.int64, device=DEV)


# --------------------------------------------------------------------------- LayerNorm forward
def _ln_fwd(i, p, has_s, save=True, kbits=False, **fp8):
    """ops.kernels.ln_fwd on the inputs of a case: ((y, hsave, mean, rstd), keep bitmap) on the CPU."""
    M, D = i.x.shape
    kb = torch.full((M, D // 8), 0xA5, dtype=torch.uint8, device=DEV) if kbits else None
    out = kk.ln_fwd(_dev(i.x), _dev(i.s) if has_s else None, _dev(i.gamma), _dev(i.beta), p, N.SEED, _ctr(),
                    N.SITE, save=save, kbits=kb, **fp8)
    return _cpu(out), _cpu([kb])[0]


FWD_NAMES = ("y", "hsave", "mean", "rstd")


@pytest.mark.parametrize("M", N.FWD_M)
@pytest.mark.parametrize("D", N.DS)
def test_ln_fwd(D, M):
    for p, has_s, save in N.fwd_settings():
        i = N.fwd_inputs(D, M, p)
        what = f"D={D} M={M} p={p} s={has_s} save={save}"
        out, _ = _ln_fwd(i, p, has_s, save)
        N.check_ln_fwd(out, i.x, i.s if has_s else None, i.gamma, i.beta, i.keep, p, save, what)
        if D >= 512 and p > 0:  # the keep bitmap: the mask itself, and nothing else changes
            out2, kb = _ln_fwd(i, p, has_s, save, kbits=True)
            R.exact(kb, N.pack_bits(i.keep), what + " kbits")
            for a, b, name in zip(out, out2, FWD_NAMES):
                assert (a is None) == (b is None)
                if a is not None:
                    R.exact(b, a, f"{what} {name} with kbits")


# --------------------------------------------------------------------------- LayerNorm backward
def _ln_bwd(c, i, hsave=None, mean=None, rstd=None, dy=None, kbits=None, defer=None, **fp8):
    """ops.kernels.ln_bwd as case c asks (kbits / defer: overriding it), on the
    inputs i. Returns the dict ref_norm.check_ln_bwd takes, on the CPU."""
    D = c.D
    init = OLD if c.accumulate else float("nan")
    dg, db = (torch.full((D,), init, device=DEV) for _ in range(2))
    dbias = torch.full((D,), init, device=DEV) if c.dbias else None
    kbits = c.kbits if kbits is None else kbits
    kb = _dev(N.pack_bits(i.keep)) if kbits else None
    fold = [] if (c.defer if defer is None else defer) else None
    dh, ds = kk.ln_bwd(_dev(i.dy if dy is None else dy), _dev(i.hsave if hsave is None else hsave),
                       _dev(i.mean if mean is None else mean), _dev(i.rstd if rstd is None else rstd),
                       _dev(i.gamma), dg, db, dbias, c.p, N.SEED, _ctr(), N.SITE, want_ds=c.want_ds,
                       dres=_dev(i.dres), accumulate=c.accumulate, defer=fold, kbits=kb, **fp8)
    if fold is not None:
        torch.cuda.synchronize()
        assert len(fold) == (3 if c.dbias else 2)
        R.exact(dg, torch.full((D,), init), "dgamma before the deferred fold")
        kk.reduce_partials_multi(fold)
    # without want_ds and dbias no ds is computed (the wrapper hands back dh)
    got = dict(zip(("dh", "ds", "dgamma", "dbeta", "dbias"),
                   _cpu((dh, ds if c.want_ds or c.dbias else None, dg, db, dbias))))
    assert (got["ds"] is None) == (not (c.want_ds or c.dbias))
    return got


def _same(a, b, what, keys=("dh", "ds", "dgamma", "dbeta", "dbias")):
    for k in keys:
        assert (a[k] is None) == (b[k] is None), f"{what}: {k}"
        if a[k] is not None:
            R.exact(b[k], a[k], f"{what}: {k}")


@pytest.mark.parametrize("rpb", N.RPBS)
@pytest.mark.parametrize("D", N.DS)
def test_ln_bwd(D, rpb, monkeypatch):
    monkeypatch.setattr(layernorm, "LN_BWD_RPB", rpb)  # rows per backward workgroup
    assert kk.ln_bwd_rpb(D) == rpb
    old = {k: torch.full((D,), OLD) for k in ("dgamma", "dbeta", "dbias")}
    for c in N.bwd_cases(D, rpb):
        i = N.bwd_inputs(D, c.M, c.p, c.dres)
        got = _ln_bwd(c, i)
        N.check_ln_bwd(got, i.ref, i.keep, str(c), old if c.accumulate else None)
        if c.kbits:
            _same(got, _ln_bwd(c, i, kbits=False), f"{c}: mask read against regenerated")
        if c.defer:
            _same(got, _ln_bwd(c, i, defer=False), f"{c}: deferred against immediate fold")


@pytest.mark.parametrize("D,M", N.CHAINED)
def test_ln_chained(D, M):
    """Kernel forward into kernel backward: the backward reference from the
    kernel's own hsave, mean and rstd."""
    p = 0.1
    i = N.fwd_inputs(D, M, p)
    (y, h, mean, rstd), _ = _ln_fwd(i, p, True)
    N.check_ln_fwd((y, h, mean, rstd), i.x, i.s, i.gamma, i.beta, i.keep, p, True, f"chained D={D} forward")
    dy = N.chained_dy(D, M)
    c = N.BwdCase(D, kk.ln_bwd_rpb(D), M, p)
    got = _ln_bwd(c, N.BwdIn(dy, h, mean, rstd, i.gamma, i.keep, None, None, i.kinds))
    ref = N.ref_ln_bwd(dy, h, mean, rstd, i.gamma, i.keep, p)
    N.check_ln_bwd(got, ref, i.keep, f"chained D={D} backward")


@pytest.mark.parametrize("D", N.DS)
def test_fp8_copies_leave_the_rest_alone(D):
    """With the e4m3 copy of y / the e5m2 copy of ds requested, every other
    output is bitwise that of the plain call (the copies themselves:
    tests/test_gpu_fp8.py)."""
    from tensorflow_distributed_on_gke_amd.ops import fp8 as F

    M, p = 37, 0.1
    i = N.fwd_inputs(D, M, p)
    plain, _ = _ln_fwd(i, p, True)
    meta = F.Fp8Meta(DEV)
    k = meta.slot("y")
    meta.scale[k] = 16.0
    y8 = torch.empty(M, D, dtype=F.FP8, device=DEV)
    with8, _ = _ln_fwd(i, p, True, y8=y8, s8=meta.s(k), amax8=meta.a(k))
    for a, b, name in zip(plain, with8, FWD_NAMES):
        R.exact(b, a, f"D={D} {name} with y8")
    b = N.bwd_inputs(D, M, p)
    c = N.BwdCase(D, kk.ln_bwd_rpb(D), M, p)
    gmeta = F.Fp8Meta(DEV, fmt=1)
    j = gmeta.slot("ds")
    gmeta.scale[j] = 2.0 ** 8
    ds8 = torch.empty(M, D, dtype=F.BF8, device=DEV)
    c8 = N.BwdCase(D, c.rpb, M, p, want_ds=False)
    _same(_ln_bwd(c, b), _ln_bwd(c8, b, ds8=ds8, s8=gmeta.s(j), amax8=gmeta.a(j)), f"D={D} with ds8",
          keys=("dh", "dgamma", "dbeta"))


# --------------------------------------------------------------------------- folds
def _fold_items(beta, off):
    """The items of ref_norm.fold_case on the GPU, each output `off` floats
    into its buffer (off = 1: 4-byte aligned only, the scalar kernel). With
    beta = 0 the outputs start as NaN: they must not be read."""
    items = []
    for parts, old in N.fold_case(beta):
        buf = torch.full((N.FOLD_N + off,), float("nan"), device=DEV)
        out = buf[off:]
        if beta:
            out.copy_(old)
        assert out.data_ptr() % 16 == 4 * off
        items.append((_dev(parts), out, parts.shape[0], N.FOLD_N, beta))
    return items


@pytest.mark.parametrize("arm,off", [("float4", 0), ("scalar", 1)])
@pytest.mark.parametrize("beta", [0.0, 1.0])
def test_reduce_partials_multi_past_96(beta, arm, off, monkeypatch):
    """100 items of one (N, beta): two launches through the wrapper's chunks."""
    real, launches = layernorm.C(), []

    class Spy:
        def reduce_partials_multi(self, parts, *rest):
            launches.append(len(parts))
            return real.reduce_partials_multi(parts, *rest)

    monkeypatch.setattr(layernorm, "C", lambda: Spy())  # where ln_bwd / reduce_partials_multi look it up
    items = _fold_items(beta, off)
    kk.reduce_partials_multi(items)
    torch.cuda.synchronize()
    assert launches == [96, N.FOLD_ITEMS - 96]
    for k, ((parts, old), item) in enumerate(zip(N.fold_case(beta), items)):
        N.check_fold(item[1], parts, old, beta, f"{arm} beta={beta} item {k} P={item[2]}")


def test_reduce_partials_multi_refuses_97():
    items = _fold_items(1.0, 0)[:97]
    before = [it[1].clone() for it in items]
    with pytest.raises(RuntimeError):
        layernorm.C().reduce_partials_multi([it[0] for it in items], [it[1] for it in items],
                                            [it[2] for it in items], N.FOLD_N, 1.0)
    torch.cuda.synchronize()
    for it, b in zip(items, before):
        R.exact(it[1], b, "output after the refused call")


# --------------------------------------------------------------------------- embedding forward
@pytest.mark.parametrize("B,L", N.EMBED_BL)
@pytest.mark.parametrize("D", N.DS)
def test_embed_fwd(D, B, L):
    import math

    tok, table, pe = N.embed_case(D, B, L)
    pe_view = _dev(pe)[N.PE_OFF:]  # an offset view, as the decoder passes
    assert bool((tok == 0).any()) or B * L == 1
    assert bool((tok == N.EMBED_V - 1).any())
    for p in N.FWD_P:
        keep = N.keep_mask(B * L, D, p)
        what = f"D={D} B={B} L={L} p={p}"
        outs = {}
        for dt in (torch.int64, torch.int32):
            out = kk.embed_fwd(_dev(tok.to(dt)), _dev(table), pe_view, math.sqrt(D), p, N.SEED, _ctr(), N.SITE)
            outs[dt] = _cpu([out])[0]
            N.check_embed(outs[dt], tok, table, pe[N.PE_OFF:], math.sqrt(D), keep, p, f"{what} {dt}")
        R.exact(outs[torch.int32], outs[torch.int64], what + " int32 against int64 tokens")
        if D >= 512 and p > 0:
            kb = torch.full((B * L, D // 8), 0xA5, dtype=torch.uint8, device=DEV)
            out = kk.embed_fwd(_dev(tok), _dev(table), pe_view, math.sqrt(D), p, N.SEED, _ctr(), N.SITE, kbits=kb)
            R.exact(_cpu([kb])[0], N.pack_bits(keep), what + " kbits")
            R.exact(_cpu([out])[0], outs[torch.int64], what + " output with kbits")
