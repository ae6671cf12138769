"""The bf16 MFMA GEMM family on the MI355X (gemm_impl.h, gemm_pipe.h,
tdg_gemm.h, gemm_{nn,nt,tn,tt}.hip; the column sums of gemm.hip) against exact
and float64 references. References, case tables, comparators and the tolerance
table are tests/ref_gemm.py's; tests/test_gemm_refs_cpu.py shows on the CPU
that those comparators reject every mutant listed there, and that the case
tables reach every arm named below.

Every launch here runs on buffers with NaN operand padding and sentinel
guards around C (ref_gemm.build), is checked for untouched guards and a fully
written interior, and asserts that the arm its launcher recorded
(gemm_last_plan) is ref_gemm.expected_arm of the case: a case named after a
config cannot silently test the cfg 13 fallback.

Which test reaches which arm:
  lock-step cfg 0-11, 13, 14: nk below / at / above STAGES,
    K tails (nk == 1 and inside the last tile)         test_gemm_exact[cfg-*]
  256x256 kernel (cfg 12): nk 1..5, K % 64 fallback    test_gemm_exact[12-*]
  pipelined cfg 20-26: nk 1..NS+3, K = 40 fallback     test_gemm_exact[20..26-*]
  TT layout, alpha = 0.5, beta = 1, six epilogues,
    ldc = N / padded / odd / unaligned C and aux       test_gemm_exact (every config)
  bitmap producer / consumer, bitmap padding           test_gemm_exact[cfg <= 22, nt / nn]
  MFMA accumulation against 8 x E32, K = 72..4096      test_gemm_f64
  splitk_reduce_kernel, gridDim.z == 1 split launch    test_splitk
  blockIdx.y problems, G = 1 / 2 / 32, cfg 12 grouped,
    cfg 20 grouped -> cfg 13                           test_grouped
  ragged classes, tile sub-ranges, fused bias sums     test_ragged_*
  colsum scalar path (ld % 8), row-block edges         test_colsum
"""
import dataclasses

import pytest
import torch

import ref_gemm as G
import ref_tail as R
from ref_gemm import F32
from tensorflow_distributed_on_gke_amd.ops import kernels as kk
from tensorflow_distributed_on_gke_amd.ops._ext import C

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    print("\nkernel worst / tolerance (unit of ref_gemm.E32 x 8):", R.report())


def _args(bt):
    """(flat device buffers kept for the checks, the views the binding takes)."""
    flat, view = {}, {}
    for name in ("A", "B", "C", "bias", "aux", "bits"):
        flat[name], view[name] = bt.dev(name, DEV)
    return flat, view


def _launch(bt, splits=1):
    """One tdg_gemm launch on the case's buffers: (C flat, bitmap flat) on the
    CPU, after asserting the recorded arm."""
    c = bt.case
    a_kc, b_kc = G.LAYOUTS[c.layout]
    flat, v = _args(bt)
    ws = torch.empty(splits * c.M * bt.ldc, dtype=F32, device=DEV) if splits > 1 else None
    epi = {G.EPI_BIAS_RELU_BITS: G.EPI_BIAS_RELU, G.EPI_DRELU_BITS: G.EPI_DRELU}.get(c.epi, c.epi)
    kw = {} if bt.bits is None else dict(relu_bits=v["bits"], ldbits=bt.ldbits)
    C().gemm(v["A"], v["B"], v["C"], v["bias"], v["aux"], c.M, c.N, c.K, bt.lda, bt.ldb, bt.ldc, bt.ldaux,
             a_kc, b_kc, epi, c.alpha, c.beta, c.cfg, splits, ws, **kw)
    arm = G.plan_arm(C().gemm_last_plan())
    want = G.expected_arm(c.cfg, c.layout, c.epi, c.f32, c.K, splits, False)
    assert arm == want, f"{c.what()}: launched {arm}, the case expects {want}"
    torch.cuda.synchronize()
    return flat["C"].cpu(), None if bt.bits is None else flat["bits"].cpu()


CFG_LAYOUT = [(cfg, lay) for cfg in G.ALL_CFGS for lay in G.LAYOUTS]


@pytest.mark.parametrize("cfg,layout", CFG_LAYOUT)
def test_gemm_exact(cfg, layout):
    for c in G.exact_cases(cfg, layout):
        bt = G.build(c)
        G.check(bt, *_launch(bt))


@pytest.mark.parametrize("cfg,layout", CFG_LAYOUT)
def test_gemm_f64(cfg, layout):
    for c in G.tol_cases(cfg, layout):
        bt = G.build(c)
        G.check(bt, *_launch(bt))


def test_splitk():
    for c in G.splitk_cases("exact"):
        bt = G.build(c)
        Cs, _ = _launch(bt, c.splits)
        G.check(bt, Cs, None, rounding="split")
        # every value and every t is representable, so one rounding or two give the same bits
        C1, _ = _launch(bt, 1)
        R.exact(Cs, C1, c.what() + " split vs unsplit")
    for c in G.splitk_cases("tol"):
        bt = G.build(c)
        Cs, _ = _launch(bt, c.splits)
        G.check(bt, Cs, None, rounding="split")


@pytest.mark.parametrize("layout", list(G.LAYOUTS))
def test_grouped(layout):
    a_kc, b_kc = G.LAYOUTS[layout]
    for c, n in G.grouped_cases(layout):
        bts = [G.build(dataclasses.replace(c, seed=g)) for g in range(n)]
        fv = [_args(bt) for bt in bts]
        b0 = bts[0]
        C().gemm_grouped([v["A"] for _, v in fv], [v["B"] for _, v in fv], [v["C"] for _, v in fv], c.M, c.N,
                         c.K, b0.lda, b0.ldb, b0.ldc, a_kc, b_kc, c.alpha, c.beta, c.cfg)
        arm = G.plan_arm(C().gemm_last_plan())
        assert arm == c.arm, f"{c.what()} G={n}: launched {arm}, the case expects {c.arm}"
        torch.cuda.synchronize()
        for bt, (f, _) in zip(bts, fv):
            G.check(bt, f["C"].cpu())
    c = G.grouped_cases(layout)[0][0]
    bt = G.build(c)
    f, v = _args(bt)
    with pytest.raises(RuntimeError):
        C().gemm_grouped([v["A"]] * 33, [v["B"]] * 33, [v["C"]] * 33, c.M, c.N, c.K, bt.lda, bt.ldb, bt.ldc,
                         a_kc, b_kc, 1.0, 0.0, 0)
    torch.cuda.synchronize()
    R.exact(f["C"].cpu(), bt.C, "C after the refused G = 33")


# --------------------------------------------------------------------------- ragged 256x256 launches
def _on_dev(view):
    """A strided view of a padded CPU buffer, rebuilt on the GPU over the whole buffer."""
    return view._base.to(DEV).as_strided(view.shape, view.stride(), view.storage_offset())


class _Dev:
    """A WgradProblem's device tensors."""

    def __init__(self, p):
        self.p = p
        self.dy, self.x = _on_dev(p.dy), _on_dev(p.x)
        self.dw_flat = p.dw.to(DEV)
        self.dw = self.dw_flat.as_strided((p.N, p.Kx), (p.ldw, 1), p.dw_off)
        self.db_flat = None if p.db is None else p.db.to(DEV)
        self.db = None if p.db is None else self.db_flat[:p.N]


R256_ARM = G.Arm("r256", 256, 256, 2, 1)


def _ragged(ds, beta, ranges=None):
    biases = [d.db for d in ds]
    kk.wgrad_ragged([d.dy for d in ds], [d.x for d in ds], [d.dw for d in ds], beta=beta,
                    biases=biases if any(b is not None for b in biases) else None, ranges=ranges)
    assert G.plan_arm(C().gemm_last_plan()) == R256_ARM
    torch.cuda.synchronize()


def _problems(P, ncls, T, beta, exactf=True):
    shapes = G.RAGGED_SHAPES[:ncls]
    per = -(-P // ncls)
    ps = []
    for i in range(P):
        N, Kx = shapes[min(i // per, ncls - 1)]
        ps.append(G.wgrad_problem(N, Kx, T, beta, with_bias=(i % 2 == 0), seed=i, exactf=exactf,
                                  pad=8 * (i // per % 2), ldw_pad=3 * (i // per % 2)))
    return ps


@pytest.mark.parametrize("T", G.RAGGED_KS)
def test_ragged_exact(T):
    """1, 8 and 64 problems in 1..8 shape classes; fused bias sums on
    alternating problems; beta 0 and 1. Bitwise (exact family)."""
    big = (64, 4) if T in (64, 320) else (16, 5)  # (the full 64 problems at the shortest and longest K)
    for P, ncls in ((1, 1), (8, 8), (8, 3), big):
        for beta in (0.0, 1.0):
            ps = _problems(P, ncls, T, beta)
            ds = [_Dev(p) for p in ps]
            _ragged(ds, beta)
            for i, d in enumerate(ds):
                G.check_wgrad(d.p, d.dw_flat, d.db_flat, f"ragged T={T} P={P} classes={ncls} beta={beta} problem {i}")


def test_ragged_f64_and_padded_vocab():
    """Toleranced operands against float64 (weights: gemm_acc, bias sums:
    scale sum |dy|), and the padded-vocab operand (7010 rows, ld 7040)."""
    for T in (64, 320):
        for beta in (0.0, 1.0):
            ps = _problems(8, 8, T, beta, exactf=False)
            ds = [_Dev(p) for p in ps]
            _ragged(ds, beta)
            for i, d in enumerate(ds):
                G.check_wgrad(d.p, d.dw_flat, d.db_flat, f"ragged f64 T={T} beta={beta} problem {i}", exactf=False)
    for exactf in (True, False):
        p = G.wgrad_problem(7010, 8, 64, 1.0, True, seed=3, exactf=exactf, pad=24)
        assert p.dy.stride(0) == 7040
        d = _Dev(p)
        _ragged([d], 1.0)
        G.check_wgrad(p, d.dw_flat, d.db_flat, f"padded vocab exact={exactf}", exactf=exactf)


def test_ragged_tile_ranges():
    """A problem cut at every tile boundary into two launches equals the
    single launch bitwise, weights and bias; a range without tn == 0 tiles
    leaves the bias untouched."""
    N, Kx, T = 264, 520, 128
    nt = G.tiles_of(N, Kx)
    for beta in (0.0, 1.0):
        p = G.wgrad_problem(N, Kx, T, beta, True, seed=1, exactf=False)
        whole = _Dev(p)
        _ragged([whole], beta)
        G.check_wgrad(p, whole.dw_flat, whole.db_flat, f"whole beta={beta}", exactf=False)
        for cut in range(1, nt):
            d = _Dev(p)
            _ragged([d], beta, ranges=[(0, cut)])
            first = (d.dw_flat.cpu(), d.db_flat.cpu())
            want = G.ragged_f32([p], beta, ranges=[(0, cut)])[0]
            # what the first launch must not have touched is still pristine
            untouched = G._as_int(want[0]) == G._as_int(p.dw)
            assert bool((G._as_int(first[0])[untouched] == G._as_int(p.dw)[untouched]).all()), \
                f"cut {cut}: the first launch wrote outside its tiles"
            _ragged([d], beta, ranges=[(cut, nt - cut)])
            R.exact(d.dw_flat.cpu(), whole.dw_flat.cpu(), f"cut {cut} beta={beta} weights")
            R.exact(d.db_flat.cpu(), whole.db_flat.cpu(), f"cut {cut} beta={beta} bias")
        # tiles 2.. of this grid (tiles_n > tiles_m: tn = t // tiles_m) have no tn == 0 tile
        assert not any(G.tile_rect(N, Kx, t)[2] for t in range(2, nt))
        d = _Dev(p)
        _ragged([d], beta, ranges=[(2, nt - 2)])
        R.exact(d.db_flat.cpu(), p.db, f"beta={beta}: bias after a range without tn == 0 tiles")


def test_ragged_refusals():
    p = G.wgrad_problem(40, 300, 64, 0.0, True, seed=0)
    d = _Dev(p)
    sh = [p.N, p.Kx, d.dy.stride(0), d.x.stride(0), p.ldw, 0, -1]

    def raw(As, Bs, Cs, shapes, K=64, a_kc=False, b_kc=False, bias=()):
        C().gemm_ragged(As, Bs, Cs, shapes, K, a_kc, b_kc, 1.0, 0.0, list(bias))

    # (its buffers also read as K-contiguous operands [40][64] and [8][64])
    p2 = G.wgrad_problem(40, 8, 64, 0.0, True, seed=1)
    d2 = _Dev(p2)
    nine = [G.wgrad_problem(8 * (i + 1), 8, 64, 0.0, False, seed=i) for i in range(9)]
    nd = [_Dev(q) for q in nine]
    bad = [
        ("rc=-2|problems", lambda: raw([], [], [], [])),
        ("problems", lambda: raw([d.dy] * 65, [d.x] * 65, [d.dw] * 65, sh * 65)),
        ("rc=-4", lambda: raw([d2.dy], [d2.x], [d2.dw], [p2.N, p2.Kx, d2.dy.stride(0), 64, p2.ldw, 0, -1],
                              a_kc=False, b_kc=True)),  # TT has no 256x256 kernel
        ("rc=-5", lambda: raw([q.dy for q in nd], [q.x for q in nd], [q.dw for q in nd],
                              sum(([q.p.N, q.p.Kx, q.dy.stride(0), q.x.stride(0), q.p.ldw, 0, -1] for q in nd), []))),
        ("rc=-6|shape", lambda: raw([d.dy], [d.x], [d.dw], [p.N, p.Kx, d.dy.stride(0) + 4, d.x.stride(0), p.ldw, 0, -1])),
        ("rc=-7|MN-contiguous", lambda: raw([d2.dy], [d2.x], [d2.dw], [p2.N, p2.Kx, 64, 64, p2.ldw, 0, -1],
                                            a_kc=True, b_kc=True, bias=[d2.db])),
        ("rc=-8", lambda: raw([d.dy], [d.x], [d.dw], sh[:5] + [1, G.tiles_of(p.N, p.Kx)])),
        ("rc=-8", lambda: raw([d.dy], [d.x], [d.dw], sh[:5] + [0, 0])),
        ("multiple of 64", lambda: raw([d.dy], [d.x], [d.dw], sh, K=72)),
    ]
    for pat, call in bad:
        with pytest.raises(RuntimeError, match=pat):
            call()
    torch.cuda.synchronize()
    R.exact(d.dw_flat.cpu(), p.dw, "dw after the refused launches")
    R.exact(d.db_flat.cpu(), p.db, "bias after the refused launches")
    R.exact(d2.dw_flat.cpu(), p2.dw, "dw after the refused launches")
    R.exact(d2.db_flat.cpu(), p2.db, "bias after the refused launches")


# --------------------------------------------------------------------------- column sums
@pytest.mark.parametrize("grouped", [False, True])
def test_colsum(grouped):
    rpb = 256 if grouped else 128  # (ops.kernels' rows per block)
    for M in G.colsum_ms(rpb):
        for N in G.COLSUM_NS:
            for beta in (0.0, 1.0):
                for odd in (False, True):
                    what = f"colsum grouped={grouped} M={M} N={N} beta={beta} odd_ld={odd}"
                    cs = [G.colsum_case(M, N, beta, odd, seed=s) for s in range(3 if grouped else 1)]
                    xs = [_on_dev(x) for x, _, _, _ in cs]
                    outs = [o.to(DEV) for _, o, _, _ in cs]
                    if grouped:
                        kk.colsum_grouped(xs, [o[:N] for o in outs], beta=beta)
                    else:
                        kk.colsum(xs[0], N, outs[0], beta=beta)
                    torch.cuda.synchronize()
                    for (x, o0, ref, scale), o in zip(cs, outs):
                        G.check_colsum(o, o0, ref, scale, N, what)
