"""The timed tile search (ops/tuning.py time_candidates) through its three
callers -- the bf16 GEMM, the grouped weight gradient and the fp8 GEMM -- at
the smallest shape each takes: with AUTOTUNE on and no table entry for the
shape, the first call searches and records one of the family's candidates, the
second call does not search, and the result is bitwise that of the recorded
config passed explicitly and within the family's tolerance of the float64
reference (tests/ref_gemm.py; the bounds of test_gpu_gemm.py / test_gpu_fp8.py)."""
import importlib

import pytest
import torch

import ref_gemm as G
import ref_tail as R
from tensorflow_distributed_on_gke_amd.ops import fp8 as F
from tensorflow_distributed_on_gke_amd.ops import kernels as kk
from tensorflow_distributed_on_gke_amd.ops import tuning
from tensorflow_distributed_on_gke_amd.ops._ext import C

# the module that owns the bf16 tables (`kk.gemm` is the function of that name)
kgemm = importlib.import_module("tensorflow_distributed_on_gke_amd.ops.kernels.gemm")

pytestmark = pytest.mark.gpu
DEV = "cuda"
S = 128  # M = N = K
TABLES = ((kgemm, "_TUNED"), (kgemm, "_GROUP_TUNED"), (F, "_TUNED"))


@pytest.fixture(autouse=True)
def _tables():
    """Each test runs on copies of the tuned tables (the wrappers look the
    module global up at call time), so what a search records never reaches
    another test; afterwards the live tables are back, unchanged."""
    live = [getattr(m, n) for m, n in TABLES]
    before = [dict(t) for t in live]
    for (m, n), t in zip(TABLES, live):
        setattr(m, n, dict(t))
    yield
    for (m, n), t in zip(TABLES, live):
        setattr(m, n, t)
    for (m, n), t, b in zip(TABLES, live, before):
        assert getattr(m, n) is t and t == b, f"{m.__name__}.{n} not restored"


@pytest.fixture
def searches(monkeypatch):
    """AUTOTUNE on in its owning module; the (candidates, reps) of every search run."""
    calls, real = [], tuning.time_candidates

    def counted(cands, trial, reps):
        calls.append((tuple(cands), reps))
        return real(cands, trial, reps)

    monkeypatch.setattr(tuning, "time_candidates", counted)
    monkeypatch.setattr(tuning, "AUTOTUNE", True)
    return calls


def _dev(bt):
    """A case's buffers on the GPU: {name: flat}, {name: 2-D operand view}."""
    c = bt.case
    a_kc, b_kc = G.LAYOUTS[c.layout]
    flat = {n: getattr(bt, n).to(DEV) for n in ("A", "B", "C")}
    shape = {"A": (c.M, c.K) if a_kc else (c.K, c.M), "B": (c.N, c.K) if b_kc else (c.K, c.N), "C": (c.M, c.N)}
    geo = {"A": (bt.lda, bt.a_off), "B": (bt.ldb, bt.b_off), "C": (bt.ldc, bt.c_off)}
    return flat, {n: flat[n].as_strided(shape[n], (geo[n][0], 1), geo[n][1]) for n in flat}


def test_gemm_nt(searches):
    bt = G.build(G.Case("tol", 0, "nt", S, S, S, G.EPI_NONE, False, 1.0, 0.0, "tight", "n"))
    key = (1024, S, S, True, True, kk.EPI_NONE, torch.bfloat16, bt.ldc % 8 == 0, False)
    kgemm._TUNED.pop(key, None)  # (in this test's copy of the table: _tables)

    def call(**kw):
        flat, v = _dev(bt)
        kk.gemm(v["A"], v["B"], v["C"], S, S, S, bt.lda, bt.ldb, bt.ldc, True, True, **kw)
        torch.cuda.synchronize()
        return flat["C"].cpu()

    first = call()
    assert searches == [(tuple(kgemm._CANDIDATES), 5)]
    ent = kgemm._TUNED[key]
    assert ent[0] == ent[1] and ent[0] in kgemm._CANDIDATES
    second = call()
    assert len(searches) == 1
    R.exact(second, first, "second call against the searching one")
    R.exact(call(cfg=ent[0]), first, f"cfg={ent[0]} against the searched call")
    G.check(bt, first)


def test_wgrad_grouped(searches):
    bts = [G.build(G.Case("tol", 0, "tn", S, S, S, G.EPI_NONE, True, 1.0, 0.0, "tight", "n", seed=g))
           for g in range(2)]
    b0 = bts[0]
    key = (S, S, S, 2, b0.lda, b0.ldb, False)
    kgemm._GROUP_TUNED.pop(key, None)

    def call(cfg=None):
        fv = [_dev(bt) for bt in bts]
        dys, xs, dws = ([v[n] for _, v in fv] for n in "ABC")
        if cfg is None:
            kk.wgrad_grouped(dys, xs, dws)
        else:
            C().gemm_grouped(dys, xs, dws, S, S, S, b0.lda, b0.ldb, b0.ldc, False, False, 1.0, 0.0, cfg)
        torch.cuda.synchronize()
        return [f["C"].cpu() for f, _ in fv]

    first = call()
    assert searches == [(tuple(kgemm._GROUP_CANDS), 3)]
    cfg = kgemm._GROUP_TUNED[key]
    assert cfg in kgemm._GROUP_CANDS
    second = call()
    assert len(searches) == 1
    fixed = call(cfg)
    for g, bt in enumerate(bts):
        R.exact(second[g], first[g], f"problem {g}: second call against the searching one")
        R.exact(fixed[g], first[g], f"problem {g}: cfg={cfg} against the searched call")
        G.check(bt, first[g])


def test_gemm_fp8(searches):
    torch.manual_seed(0)
    meta = F.Fp8Meta(DEV)
    ia, ib = meta.slot("a"), meta.slot("b")
    meta.scale[ia], meta.scale[ib] = 60.0, 900.0
    a = torch.randn(S, S, device=DEV).bfloat16()
    b = (torch.randn(S, S, device=DEV) * 0.05).bfloat16()
    a8, b8 = F.quantize(a, meta, ia), F.quantize(b, meta, ib)
    key = (S, S, S, F.EPI_NONE, False, True)
    F._TUNED.pop(key, None)

    def call(**kw):
        y, _ = F.gemm_fp8(a8, b8, None, meta, ia, ib, **kw)
        torch.cuda.synchronize()
        return y.cpu()

    first = call()
    assert searches == [(tuple(F._CANDS), 5)]
    cfg = F._TUNED[key]
    assert cfg in F._CANDS
    second = call()
    assert len(searches) == 1
    R.exact(second, first, "second call against the searching one")
    R.exact(call(cfg=cfg), first, f"cfg={cfg} against the searched call")
    # float64 reference of exactly the e4m3 values the kernel gets; the bound of test_gpu_fp8.py::test_gemm_fp8
    da, db = a8.float().cpu().to(G.F64) / 60.0, b8.float().cpu().to(G.F64) / 900.0
    ref = G.ref_gemm(da @ db.T, da.abs() @ db.abs().T, 1.0, 0.0, None, None, None, G.EPI_NONE).pre
    err = (first.to(G.F64) - ref).abs().max().item() / (ref.abs().max().item() + 1e-6)
    print(f"fp8 {S}^3 cfg {cfg}: max error / max |ref| = {err:.3e}")
    assert err < 1e-2, (cfg, err)
