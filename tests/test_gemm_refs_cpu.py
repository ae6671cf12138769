"""tests/ref_gemm.py on the CPU: its comparators accept the plain float32
evaluation of every case table and reject every mutant, its exact builder
keeps every value representable, its guards and poison are in place, its
tolerance table is measured, and its case tables reach every arm of the bf16
GEMM family that tests/test_gpu_gemm.py is meant to run (walked with
expected_arm, the Python mirror of launch_tiles' choice)."""
import dataclasses
import math

import pytest

import ref_gemm as G
import ref_tail as R
from ref_gemm import F32, F64

# one config per distinct case table (tile shape x depth family)
TABLE_CFGS = (3, 1, 2, 0, 14, 5, 6, 12, 20, 21, 22, 24)


def _all_tables():
    for cfg in G.ALL_CFGS:
        for layout in G.LAYOUTS:
            yield from G.exact_cases(cfg, layout)
            yield from G.tol_cases(cfg, layout)


@pytest.mark.parametrize("cfg", TABLE_CFGS)
def test_f32_evaluation_passes_and_cases_are_sound(cfg):
    """The float32 evaluation passes every comparator; the exact builder's
    representability assertion holds (build() asserts it); guards and poison
    are in place before any kernel would run."""
    for layout in G.LAYOUTS:
        for c in G.exact_cases(cfg, layout) + G.tol_cases(cfg, layout):
            bt = G.build(c)
            G.check_pristine(bt)
            G.check(bt, *G.gemm_f32(bt))


def test_f32_evaluation_passes_split_and_grouped():
    for fam in ("exact", "tol"):
        for c in G.splitk_cases(fam):
            bt = G.build(c)
            G.check_pristine(bt)
            G.check(bt, *G.gemm_f32(bt, rounding="split"), rounding="split")
            if fam == "exact":  # one rounding or two: the same bits
                R.exact(G.gemm_f32(bt, rounding="split")[0], G.gemm_f32(bt, rounding="tile")[0], c.what())
    for layout in G.LAYOUTS:
        for c, n in G.grouped_cases(layout):
            for g in {0, n - 1}:
                bt = G.build(dataclasses.replace(c, seed=g))
                G.check_pristine(bt)
                G.check(bt, *G.gemm_f32(bt))


def test_exact_family_is_bitwise_in_float32():
    """In the exact family the float32 evaluation IS the reference, bitwise,
    whatever the rounding arm: what the kernels are held to."""
    for c in G.exact_cases(3, "nt") + G.exact_cases(21, "tt"):
        bt = G.build(c)
        a, _ = G.gemm_f32(bt, rounding="tile")
        b, _ = G.gemm_f32(bt, rounding="split")
        R.exact(a, b, c.what())


# where a mutant changes the float32 evaluation's output at all, the comparators must notice
def _differs(x, y):
    return any(u is not None and not bool((G._as_int(u) == G._as_int(v)).all()) for u, v in zip(x, y))


# mutants whose effect is a rounding-sized change: visible only where the value was not representable
ROUNDING_MUTANTS = ("trunc_bf16", "third_rounding")


def test_every_mutant_is_rejected():
    hit = {m: 0 for m in G.MUTANTS}
    applied = {m: 0 for m in G.MUTANTS}
    cases = [c for layout in G.LAYOUTS for c in G.exact_cases(3, layout) + G.tol_cases(3, layout)]
    cases += list(G.exact_cases(21, "nt")[::3]) + list(G.tol_cases(12, "nn"))
    for c in cases:
        bt = G.build(c)
        clean = G.gemm_f32(bt)
        for m in G.MUTANTS:
            mut = G.gemm_f32(bt, mutant=m)
            if not _differs(mut, clean):
                continue
            applied[m] += 1
            if G.rejected(bt, *mut):
                hit[m] += 1
            elif m in ROUNDING_MUTANTS:
                # a different but still correctly rounded result (a tie, or a double
                # rounding that lands within half an ulp): only a whole matrix tells
                assert c.M * c.N < 4096, f"{m} accepted on {c.what()}"
            else:
                raise AssertionError(f"mutant {m} accepted on {c.what()}")
    print("mutants rejected / applied:", {m: f"{hit[m]}/{applied[m]}" for m in G.MUTANTS})
    for m in G.MUTANTS:
        assert hit[m] > 0, f"mutant {m} was rejected nowhere"
    # relu_ge shows only through the +-0 entries of aux, third_rounding / trunc_bf16 only in the toleranced family
    assert applied["relu_ge"] > 0 and applied["ktail_kept"] > 0 and applied["stale_tile"] > 0


def test_third_rounding_does_not_fit_the_budget():
    """The bf16 beta != 0 contract: two roundings (1 ulp) pass, three do not."""
    cs = [c for c in G.tol_cases(3, "nt") if not c.f32 and c.beta != 0 and c.M * c.N >= 4096]
    assert cs
    n = 0
    for c in cs:
        bt = G.build(c)
        clean = G.gemm_f32(bt, rounding="tile")
        G.check(bt, *clean)
        mut = G.gemm_f32(bt, mutant="third_rounding")
        if _differs(mut, clean):  # (no bias and alpha a power of two: rounding acc first changes nothing)
            assert G.rejected(bt, *mut), c.what()
            n += 1
    assert n > 0
    # and the split-K arm is held to one rounding: two do not fit it
    cs = [c for c in G.splitk_cases("tol") if not c.f32 and c.beta != 0 and c.epi != G.EPI_DRELU]
    assert cs and any(G.rejected(G.build(c), *G.gemm_f32(G.build(c), rounding="tile"), rounding="split") for c in cs)


def test_ragged_and_colsum_references():
    """The float32 evaluation of a ragged launch passes check_wgrad; the
    grouped / ragged mutants do not; column sums likewise."""
    for exactf in (True, False):
        for beta in (0.0, 1.0):
            ps = [G.wgrad_problem(N, Kx, 128, beta, i % 2 == 0, seed=i, exactf=exactf, pad=8 * (i % 2),
                                  ldw_pad=3 * (i % 2))
                  for i, (N, Kx) in enumerate(((264, 520), (264, 520), (40, 300), (8, 8)))]
            for p, (dw, db) in zip(ps, G.ragged_f32(ps, beta)):
                G.check_wgrad(p, dw, db, "f32", exactf=exactf)
            for p, (dw, db) in list(zip(ps, G.ragged_f32(ps, beta, mutant="problem_swapped")))[:2]:
                with pytest.raises(G.Mismatch):
                    G.check_wgrad(p, dw, db, "problem_swapped", exactf=exactf)
            p = ps[0]
            dw, db = G.ragged_f32([p], beta, mutant="bias_sum_all_tn")[0]
            if beta != 0:  # (beta == 0: summing the same rows again stores the same sums)
                with pytest.raises(G.Mismatch):
                    G.check_wgrad(p, dw, db, "bias_sum_all_tn", exactf=exactf)
            nt = G.tiles_of(p.N, p.Kx)
            whole = G.ragged_f32([p], beta)[0]
            for cut in range(1, nt):
                q = dataclasses.replace(p)
                q.dw, q.db = G.ragged_f32([p], beta, ranges=[(0, cut)])[0]
                two = G.ragged_f32([q], beta, ranges=[(cut, nt - cut)])[0]
                R.exact(two[0], whole[0], f"cut {cut}")
                R.exact(two[1], whole[1], f"cut {cut} bias")
                q.dw, q.db = G.ragged_f32([p], beta, ranges=[(0, cut)], mutant="range_off_by_one")[0]
                bad = G.ragged_f32([q], beta, ranges=[(cut, nt - cut)])[0]
                with pytest.raises(G.Mismatch):
                    R.exact(bad[0], whole[0], "range_off_by_one")
    for M in G.colsum_ms(128):
        for N in G.COLSUM_NS:
            for beta in (0.0, 1.0):
                for odd in (False, True):
                    x, out, ref, scale = G.colsum_case(M, N, beta, odd)
                    assert bool(x._base.isnan().sum() == x._base.numel() - M * N) and x.stride(0) % 8 == (3 if odd else 0)
                    G.check_colsum(G.colsum_f32(x, out, N, beta), out, ref, scale, N, "f32")
                    with pytest.raises(G.Mismatch):
                        G.check_colsum(G.colsum_f32(x, out, N, beta, mutant="last_row_dropped"), out, ref, scale, N, "m")


def _measure_e32():
    worst = {k: 0.0 for k in G.E32}
    seen = set()
    for cfg in G.ALL_CFGS:
        for c in G.tol_cases(cfg, "nt"):
            key = (c.M, c.N, c.K, c.epi, c.f32, c.alpha, c.beta)
            if key in seen:
                continue
            seen.add(key)
            bt = G.build(dataclasses.replace(c, f32=True, ldc="n") if c.epi < G.EPI_BIAS_RELU else c)
            if not bt.case.f32:
                continue
            got = G.interior(G.gemm_f32(bt)[0], bt.c_off, c.M, c.N, bt.ldc).to(F64)
            den = bt.ref.pre.abs() + abs(c.alpha) * bt.ref.S + (c.beta * bt.cold).abs()
            worst["gemm_acc"] = max(worst["gemm_acc"], float(((got - bt.ref.pre).abs() / den.clamp_min(1e-300)).max()))
    for T in (64, 320):
        for (N, Kx) in G.RAGGED_SHAPES:
            p = G.wgrad_problem(N, Kx, T, 1.0, True, seed=0, exactf=False)
            s = p.dy.to(F32).sum(0) + p.old_b.to(F32)
            worst["gemm_bsum"] = max(worst["gemm_bsum"], float(((s.to(F64) - p.ref_b).abs() / p.S_b).max()))
    for M in G.colsum_ms(128) + G.colsum_ms(256):
        for N in G.COLSUM_NS:
            for beta in (0.0, 1.0):
                x, out, ref, scale = G.colsum_case(M, N, beta, False)
                got = G.colsum_f32(x, out, N, beta)[:N].to(F64)
                worst["colsum"] = max(worst["colsum"], float(((got - ref).abs() / scale.clamp_min(1e-300)).max()))
    return worst


def test_e32_table_is_measured():
    """Every tolerance is 8 x an E32 that this machine reproduces: not below
    what the float32 evaluation needs, and not inflated."""
    got = _measure_e32()
    print("measured E32:", {k: f"{v:.2e}" for k, v in sorted(got.items())})
    assert set(got) == set(G.E32)
    for k, e in G.E32.items():
        # (the same bounds as tests/test_loss_optim_refs_cpu.py::test_e32_table_is_measured)
        assert got[k] <= 1.5 * e, f"{k}: measured {got[k]:.3e} above the table's {e:.3e}"
        assert got[k] >= e / 4, f"{k}: the table's {e:.3e} is more than 4x the measured {got[k]:.3e}"
    assert G.MARGIN == 8.0 and all(math.isclose(R.tol(k), 8 * e) for k, e in G.E32.items())
    assert not set(G.E32) & set(R.E32)


def test_case_tables_reach_every_arm():
    """Walks the case tables with expected_arm: every family x layout x
    epilogue x dtype that dispatch_epi / has_256 instantiate, every config,
    every nk class per depth, every ldc / alignment variant, every split-K
    triple -- and every fallback on purpose."""
    reached, nk, ldc, cfgs_own = set(), set(), set(), set()
    falls = set()
    for c in _all_tables():
        arm = c.arm
        reached.add((arm.family, c.layout, c.epi, c.f32))
        nk.add((arm.family, arm.depth, G.nk_class(arm.family, arm.depth, c.K)))
        ldc.add((arm.family, c.ldc, c.ld))
        own = (c.cfg in G.LOCK and arm.family == "lock") or (c.cfg == G.R256 and arm.family == "r256") or \
              (c.cfg in G.PIPE and arm.family == "pipe")
        if own:
            assert (arm.bm, arm.bn) == G.tile_of(c.cfg)
            cfgs_own.add(c.cfg)
        else:
            assert arm[:4] == ("lock", 128, 128, 4)  # cfg 13
            if c.cfg == G.R256:
                falls.add("K%64" if c.K % 64 else ("TT under 12" if c.layout == "tt" else
                          ("BIAS f32 under 12 NN" if (c.layout, c.epi, c.f32) == ("nn", G.EPI_BIAS, True) else "no 256")))
            else:
                falls.add("K%32" if c.K % 32 else "?")
    assert cfgs_own == set(G.ALL_CFGS), sorted(set(G.ALL_CFGS) - cfgs_own)
    for layout in G.LAYOUTS:
        for cfg, fam in ((0, "lock"), (G.R256, "r256"), (20, "pipe"), (23, "pipe")):
            for (e, f) in G.epis_of(layout, cfg):
                if fam == "r256" and not G.has_256(layout, e, f):
                    continue
                assert (fam, layout, e, f) in reached, (fam, layout, G.EPI_NAMES[e], f)
    # nk classes: lock-step below / at / above the depth with and without a K tail, for every depth
    for st in sorted({v[2] for v in G.LOCK.values()}):
        got = {k for (fam, d, k) in nk if fam == "lock" and d == st}
        for j in range(1, st + 3):
            rel = "<" if j < st else ("=" if j == st else ">")
            assert f"nk{rel}depth:{j}" in got, (st, j, sorted(got))
            assert f"nk{rel}depth:{j}:tail" in got, (st, j, sorted(got))
    assert {k for (fam, d, k) in nk if fam == "r256"} >= {"nk1", "nk2", "nk3", "nk4"}
    for ns in sorted({v[2] for v in G.PIPE.values()}):
        got = {k for (fam, d, k) in nk if fam == "pipe" and d == ns}
        assert got >= {f"nk{j}" for j in range(1, ns + 4)}, (ns, sorted(got))
    for fam in ("lock", "r256", "pipe"):
        for m in G.LDC_MODES:
            assert any((fam, m, l) in ldc for l in G.LD_MODES), (fam, m)
        for l in G.LD_MODES:
            assert any((fam, m, l) in ldc for m in G.LDC_MODES), (fam, l)
    assert falls >= {"K%64", "K%32", "TT under 12", "BIAS f32 under 12 NN"}, falls
    # split-K: every triple, every reduce epilogue, both dtypes; cfg 12 / 20 fall back to the lock-step cfg 13
    sk = G.splitk_cases("exact")
    assert {(c.K, c.splits) for c in sk} == set(G.SPLITK)
    assert {(c.epi, c.f32) for c in sk} == set(G.epis_of("tt", 99))
    assert {c.arm.splits for c in sk if (c.K, c.splits) == (64, 8)} == {1}  # collapses to gridDim.z == 1
    assert {c.arm.splits for c in sk if (c.K, c.splits) == (136, 3)} == {3}
    for cfg in (12, 20):
        assert all(c.arm[:4] == ("lock", 128, 128, 4) for c in sk if c.cfg == cfg)
        assert any(c.cfg == cfg for c in sk)
    # grouped: cfg 12 runs the 256x256 kernel where it has one, cfg 20 falls back
    for layout in G.LAYOUTS:
        gc = G.grouped_cases(layout)
        assert {n for _, n in gc} == set(G.GROUP_GS) and {c.cfg for c, _ in gc} == set(G.GROUP_CFGS)
        assert all(c.arm[:4] == ("lock", 128, 128, 4) for c, _ in gc if c.cfg == 20)
        assert any(c.arm.family == "r256" for c, _ in gc if c.cfg == 12) == (layout != "tt")
