"""The tail of the training step on the MI355X against float64 references:
the fused cross-entropy on every dispatch arm of tdg_xent, xent_stats,
count_tokens, both Adam kernels (weight update, moments, schedule, options,
the capped grid) and to_bf16. References, cases, comparators and the tolerance
table are tests/ref_tail.py's; tests/test_loss_optim_refs_cpu.py shows on the
CPU that those comparators reject every mutant listed there."""
import functools

import pytest
import torch

import ref_tail as R
from ref_tail import BF16, F32, F64, AdamCfg
from tensorflow_distributed_on_gke_amd.ops import kernels as kk
from tensorflow_distributed_on_gke_amd.ops._ext import C

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    print("\nkernel worst / tolerance (unit of ref_tail.E32 x 8):", R.report())


# --------------------------------------------------------------------------- cross-entropy
@functools.lru_cache(maxsize=None)
def _rows(V, ldl):
    return R.xent_rows(V, ldl, 16 if V == 32000 else 40)


@functools.lru_cache(maxsize=None)
def _ref(V, ldl, smoothing, workers):
    lg, lab = _rows(V, ldl)
    return R.ref_xent(lg[:, :V], lab, workers, smoothing)


def _run_xent(lg, V, lab, workers, smoothing, write_grad=True, offset=0):
    """The kernel on a copy of lg placed `offset` elements into its buffer.
    Returns (row_loss, row_correct, ntok, logits after the call) on the CPU."""
    M, ldl = lg.shape
    buf = torch.zeros(offset + M * ldl, dtype=BF16, device=DEV)
    x = buf[offset:].view(M, ldl)
    x.copy_(lg)
    assert x.is_contiguous() and x.data_ptr() % 16 == (2 * offset) % 16
    labd = lab.to(DEV)
    ntok = torch.full((1,), -1.0, device=DEV)
    kk.count_tokens(labd, ntok)
    rl = torch.full((M,), float("nan"), device=DEV)
    rc = torch.full((M,), float("nan"), device=DEV)
    kk.xent(x, V, labd, ntok, workers, smoothing, rl, rc, write_grad)
    torch.cuda.synchronize()
    return rl.cpu(), rc.cpu(), ntok.item(), x.cpu()


def _check_xent(out, V, ref, lg, workers, what):
    loss, correct, ntok, d = ref
    assert out[2] == ntok, f"{what}: ntok {out[2]} vs {ntok}"
    R.close_f32(out[0], loss, "row_loss", what + " row_loss", scale=R.row_loss_scale(lg[:, :V]))
    R.exact(out[1], correct.to(F32), what + " row_correct")
    R.close_dlogits(out[3], d, V, R.xent_scale(ntok, workers), what + " dlogits")


@pytest.mark.parametrize("workers", R.XENT_WORKERS)
@pytest.mark.parametrize("smoothing", R.XENT_SMOOTHING)
@pytest.mark.parametrize("V,ldl", R.XENT_SHAPES)
def test_xent_every_arm(V, ldl, smoothing, workers):
    lg, lab = _rows(V, ldl)
    out = _run_xent(lg, V, lab, workers, smoothing)
    _check_xent(out, V, _ref(V, ldl, smoothing, workers), lg, workers,
                f"{R.xent_expected_arm(V, ldl)} V={V} ldl={ldl} s={smoothing} w={workers}")


@pytest.mark.parametrize("V,ldl", R.XENT_BOTH_LABEL_DTYPES)
def test_xent_label_dtypes_bitwise_equal(V, ldl):
    lg, lab = _rows(V, ldl)
    a = _run_xent(lg, V, lab, 2.0, 0.1)
    b = _run_xent(lg, V, lab.to(torch.int32), 2.0, 0.1)
    _check_xent(b, V, _ref(V, ldl, 0.1, 2.0), lg, 2.0, f"int32 labels V={V}")
    assert a[2] == b[2]
    for k, name in ((0, "row_loss"), (1, "row_correct"), (3, "dlogits")):
        R.exact(b[k], a[k], f"int32 vs int64 labels: {name}")


def test_xent_both_kernels_on_the_same_data():
    """An element offset of 2 (4-byte aligned, not 16) selects the two-pass
    kernel for a shape the register kernel otherwise takes."""
    V, ldl = 7010, 7040
    lg, lab = _rows(V, ldl)
    for s in R.XENT_SMOOTHING:
        reg = _run_xent(lg, V, lab, 2.0, s)
        gen = _run_xent(lg, V, lab, 2.0, s, offset=2)
        ref = _ref(V, ldl, s, 2.0)
        _check_xent(gen, V, ref, lg, 2.0, f"generic by alignment s={s}")
        _check_xent(reg, V, ref, lg, 2.0, f"register s={s}")
        R.exact(gen[1], reg[1], "row_correct of the two kernels")


@pytest.mark.parametrize("V,ldl,offset", [(250, 256, 0), (7010, 7040, 0), (7010, 7040, 2), (8193, 8200, 0),
                                          (1001, 1002, 0)])
def test_xent_without_gradient(V, ldl, offset):
    lg, lab = _rows(V, ldl)
    a = _run_xent(lg, V, lab, 2.0, 0.1, write_grad=True, offset=offset)
    b = _run_xent(lg, V, lab, 2.0, 0.1, write_grad=False, offset=offset)
    R.exact(b[3], lg, "logits after write_grad=False (poisoned padding included)")
    R.exact(b[0], a[0], "row_loss with and without the gradient")
    R.exact(b[1], a[1], "row_correct with and without the gradient")


@pytest.mark.parametrize("V,ldl", [(250, 256), (5000, 5056), (8193, 8200), (33, 34)])
def test_xent_all_pad(V, ldl):
    lg, lab = _rows(V, ldl)
    lab = torch.zeros_like(lab)
    rl, rc, ntok, d = _run_xent(lg, V, lab, 2.0, 0.1)
    assert ntok == 0.0
    for t, name in ((rl, "row_loss"), (rc, "row_correct"), (d, "dlogits")):
        assert bool((t.float() == 0).all()), f"all PAD: {name} not all zero"
    so = torch.full((2,), float("nan"), device=DEV)
    acc = torch.zeros(4, device=DEV)
    kk.xent_stats(rl.to(DEV), rc.to(DEV), torch.zeros(1, device=DEV), 2.0, so, acc)
    assert so.tolist() == [0.0, 0.0] and acc.tolist() == [0.0, 0.0, 1.0, 0.0]


@pytest.mark.parametrize("V,ldl", [(250, 256), (7010, 7040), (8193, 8200)])
def test_xent_single_row(V, ldl):
    lg, lab = _rows(V, ldl)
    i = int((lab != 0).nonzero()[0])
    lg1, lab1 = lg[i:i + 1].contiguous(), lab[i:i + 1]
    out = _run_xent(lg1, V, lab1, 1.0, 0.1)
    _check_xent(out, V, R.ref_xent(lg1[:, :V], lab1, 1.0, 0.1), lg1, 1.0, f"M=1 V={V}")


# --------------------------------------------------------------------------- xent_stats, count_tokens
def _stats_case(M, workers, misaligned=False, step_out=True, accum=True, calls=1):
    rl, rc, ntok = R.stats_rows(M)
    off = 1 if misaligned else 0
    bl = torch.full((M + 8,), float("nan"), device=DEV)
    bc = torch.full((M + 8,), float("nan"), device=DEV)
    L, C = bl[off:off + M], bc[off:off + M]
    L.copy_(rl)
    C.copy_(rc)
    assert L.data_ptr() % 16 == 4 * off
    nt = torch.tensor([ntok], device=DEV)
    so = torch.full((2,), float("nan"), device=DEV) if step_out else None
    acc = torch.zeros(4, device=DEV) if accum else None
    for _ in range(calls):
        kk.xent_stats(L, C, nt, workers, so, acc)
    torch.cuda.synchronize()
    loss, accuracy, correct = R.ref_xent_stats(rl, rc, ntok, workers)
    what = f"xent_stats M={M} w={workers} misaligned={misaligned}"
    if so is not None:
        R.close_f32(so[0:1].cpu(), torch.tensor([loss]), "stats_loss", what)
        R.close_accuracy(so[1].item(), correct, ntok, what)
    if acc is not None:
        a = acc.tolist()
        R.close_f32(acc[0:1].cpu(), torch.tensor([calls * loss]), "stats_loss", what + " accum")
        # (the accuracy is added once per call, each within 1 ulp)
        assert abs(a[1] - calls * accuracy) <= calls * float(R.ulp32(torch.tensor([accuracy], dtype=F64)))
        assert a[2] == float(calls) and a[3] == calls * ntok, what  # exact: small integers in f32
    if so is not None and acc is not None and calls == 1:
        assert acc[:2].tolist() == so.tolist()


@pytest.mark.parametrize("M", R.STATS_M)
def test_xent_stats(M):
    for w in R.XENT_WORKERS:
        _stats_case(M, w)
    _stats_case(M, 2.0, step_out=True, accum=False)
    _stats_case(M, 2.0, step_out=False, accum=True)
    _stats_case(M, 2.0, step_out=False, accum=False)  # nothing to write: must only not fault
    _stats_case(M, 2.0, calls=2)


@pytest.mark.parametrize("M", [4096, 4100, 8196])
def test_xent_stats_misaligned_view(M):
    """M % 4 == 0 but the rows start 4 bytes into their buffers: the scalar path."""
    _stats_case(M, 2.0, misaligned=True)


@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
@pytest.mark.parametrize("M", R.COUNT_M)
def test_count_tokens(M, dtype):
    g = torch.Generator().manual_seed(M)
    lab = torch.randint(0, 5, (M,), generator=g).to(dtype)
    if M > 1:
        lab[-1] = 3
    out = torch.full((1,), -7.0, device=DEV)
    kk.count_tokens(lab.to(DEV), out)
    assert out.item() == float((lab != 0).sum())


# --------------------------------------------------------------------------- Adam
SENTINEL = 7.0
N1 = 4096 + 8


def _run_adam(kernel, p, g, m, v, it, cfg, zero_grad=True, inc_step=True, shadow=True, start=12,
              ranges=None):
    """One step of either kernel from CPU (or GPU) inputs. `adam_chunks` gets
    the data `start` elements into larger buffers, with a chunk table over
    exactly that range; everything outside it must stay as it was. ranges: the
    step applied as several calls [(a, b, inc_step)], all seeing one counter.
    Returns dict(p, g, m, v, shadow, step)."""
    n = p.numel()
    step = torch.tensor([it], dtype=torch.int64, device=DEV)
    ranges = ranges or [(0, n, inc_step)]
    if kernel == "adam":
        pd, gd, md, vd = (t.clone().to(DEV) for t in (p, g, m, v))
        sh = torch.full((n,), 3.0, dtype=BF16, device=DEV) if shadow else None
        for a, b, inc in ranges:
            kk.adam(pd[a:b], gd[a:b], md[a:b], vd[a:b], sh[a:b] if shadow else None, step, *cfg.args(),
                    zero_grad, inc)
        torch.cuda.synchronize()
        return dict(p=pd, g=gd, m=md, v=vd, shadow=sh, step=step.item())
    assert shadow and start % 4 == 0
    tot = start + n + 24
    big = [torch.full((tot,), SENTINEL, device=DEV) for _ in range(4)]
    SH = torch.full((tot,), 3.0, dtype=BF16, device=DEV)
    for B, t in zip(big, (p, g, m, v)):
        B[start:start + n] = t.to(DEV)
    scale8 = torch.ones(1, device=DEV)
    amax8 = torch.zeros(2048, dtype=torch.int32, device=DEV)
    for a, b, inc in ranges:
        rows = R.chunk_rows(start + a, start + b)
        assert all(r[0] % 4 == 0 and r[1] % 4 == 0 and 0 < r[1] <= 4096 and r[0] + r[1] <= tot for r in rows)
        tab = torch.tensor(rows, dtype=torch.int64, device=DEV)
        kk.adam_chunks(*big, SH, tab, step, *cfg.args(), zero_grad, inc, scale8, amax8)
    torch.cuda.synchronize()
    for B in big:
        assert bool((B[:start] == SENTINEL).all()) and bool((B[start + n:] == SENTINEL).all()), \
            "adam_chunks wrote outside its chunk table"
    assert bool((SH[:start] == 3.0).all()) and bool((SH[start + n:] == 3.0).all())
    assert not amax8.any()
    sl = slice(start, start + n)
    return dict(p=big[0][sl], g=big[1][sl], m=big[2][sl], v=big[3][sl], shadow=SH[sl], step=step.item())


def _check_step(out, p, g, m, v, it, cfg, what, zero_grad=True, inc_step=True):
    R.check_adam((out["p"], out["m"], out["v"]), p.to(DEV), g.to(DEV), m.to(DEV), v.to(DEV), it, cfg, what)
    if out["shadow"] is not None:  # f2bf is the hardware RNE convert of the p the kernel wrote
        R.exact(out["shadow"], out["p"].to(BF16), what + " shadow")
    assert out["step"] == it + (1 if inc_step else 0), f"{what}: iterations {out['step']}"
    if zero_grad:
        R.exact(out["g"], torch.zeros_like(out["g"]), what + " zeroed gradient")
    else:
        R.exact(out["g"], g, what + " kept gradient")


KERNELS = [("adam", N1), ("chunks", 4096 + 4092)]


@pytest.mark.parametrize("kernel,n", KERNELS)
@pytest.mark.parametrize("d_model,warmup", R.ADAM_SCHEDULES)
@pytest.mark.parametrize("it", R.ADAM_ITERATIONS)
def test_adam_one_step_noam(kernel, n, d_model, warmup, it):
    cfg = AdamCfg(d_model=d_model, warmup=warmup)
    p, g, m, v = R.adam_inputs(n)
    out = _run_adam(kernel, p, g, m, v, it, cfg)
    _check_step(out, p, g, m, v, it, cfg, f"{kernel} d={d_model:g} w={warmup:g} it={it}")
    if it == 0:
        R.exact(out["p"], p, "iterations = 0: p")
        assert bool((out["m"].cpu() != m).any()) and bool((out["v"].cpu() != v).any())


@pytest.mark.parametrize("kernel,n", KERNELS)
def test_adam_trajectory(kernel, n):
    """20 steps from zero moments across the schedule's peak, fresh gradients
    every step; the reference advances in float64 from the same f32 start."""
    cfg = AdamCfg()
    p0 = R.adam_inputs(n, zero_moments=True)[0]
    start = 12
    tot = start + n + 24
    P, G, M, V = (torch.full((tot,), SENTINEL, device=DEV) for _ in range(4))
    SH = torch.full((tot,), 3.0, dtype=BF16, device=DEV)
    sl = slice(start, start + n)
    P[sl] = p0.to(DEV)
    M[sl] = 0.0
    V[sl] = 0.0
    step = torch.tensor([R.TRAJ_START], dtype=torch.int64, device=DEV)
    tab = torch.tensor(R.chunk_rows(start, start + n), dtype=torch.int64, device=DEV)
    scale8, amax8 = torch.ones(1, device=DEV), torch.zeros(2048, dtype=torch.int32, device=DEV)
    for k, g, gmax, pr, mr, vr in R.ref_trajectory(p0, cfg, n):
        G[sl] = g.to(DEV)
        if kernel == "adam":
            kk.adam(P[sl], G[sl], M[sl], V[sl], SH[sl], step, *cfg.args(), True, True)
        else:
            kk.adam_chunks(P, G, M, V, SH, tab, step, *cfg.args(), True, True, scale8, amax8)
        R.close_f32(M[sl].cpu(), mr, "adam_m_traj", f"{kernel} step {k} m", scale=gmax)
        R.close_f32(V[sl].cpu(), vr, "adam_v_traj", f"{kernel} step {k} v", scale=gmax * gmax)
        assert not G[sl].any()
    assert step.item() == R.TRAJ_START + R.TRAJ_STEPS
    R.close_p(P[sl].cpu(), p0, p0.double() - pr, f"{kernel} trajectory p", "adam_dp_traj", steps=R.TRAJ_STEPS)
    R.exact(SH[sl], P[sl].to(BF16), "trajectory shadow")
    for B in (P, G, M, V):
        assert bool((B[:start] == SENTINEL).all()) and bool((B[start + n:] == SENTINEL).all())


@pytest.mark.parametrize("kernel,n", KERNELS)
@pytest.mark.parametrize("option", sorted(R.ADAM_OPTIONS))
def test_adam_options(kernel, n, option):
    cfg, it = R.ADAM_OPTIONS[option]
    p, g, m, v = R.adam_inputs(n)
    _check_step(_run_adam(kernel, p, g, m, v, it, cfg), p, g, m, v, it, cfg, f"{kernel} {option}")


@pytest.mark.parametrize("kernel,n", KERNELS)
def test_adam_keeps_gradient_and_step(kernel, n):
    cfg, it = AdamCfg(), 10
    p, g, m, v = R.adam_inputs(n)
    out = _run_adam(kernel, p, g, m, v, it, cfg, zero_grad=False)
    _check_step(out, p, g, m, v, it, cfg, f"{kernel} zero_grad=False", zero_grad=False)
    out = _run_adam(kernel, p, g, m, v, it, cfg, inc_step=False)
    _check_step(out, p, g, m, v, it, cfg, f"{kernel} inc_step=False", inc_step=False)
    # a step applied as two ranges: the second sees the same counter, then advances it
    h = 4096
    out = _run_adam(kernel, p, g, m, v, it, cfg, ranges=[(0, h, False), (h, n, True)])
    _check_step(out, p, g, m, v, it, cfg, f"{kernel} two ranges")


def test_adam_without_shadow():
    cfg, it = AdamCfg(), 10
    p, g, m, v = R.adam_inputs(N1)
    out = _run_adam("adam", p, g, m, v, it, cfg, shadow=False)
    _check_step(out, p, g, m, v, it, cfg, "adam shadow=None")


@pytest.mark.parametrize("kernel,n,start", [("adam", 4, 0), ("adam", N1, 0), ("chunks", 4, 12),
                                            ("chunks", 4092, 12), ("chunks", 4096, 4096 + 2052),
                                            ("chunks", N1, 12)])
def test_adam_edges(kernel, n, start):
    cfg, it = AdamCfg(), 10
    p, g, m, v = R.adam_inputs(n)
    _check_step(_run_adam(kernel, p, g, m, v, it, cfg, start=start), p, g, m, v, it, cfg, f"{kernel} n={n}")
    z = torch.zeros(n)
    out = _run_adam(kernel, p, z, z, z, it, cfg, start=start)
    R.exact(out["p"], p, "g = 0 from zero moments: p")
    assert not out["m"].any() and not out["v"].any()
    _check_step(out, p, z, z, z, it, cfg, f"{kernel} n={n} g=0")


def test_adam_capped_grid():
    """n4 = 2 * 8192 * 256 + 1001 float4 groups: the grid is capped at 8192
    blocks, so every thread runs the paired loop once and 1001 of them the
    odd tail. (The float64 reference is evaluated on the GPU with torch
    elementwise ops to stay within seconds.)"""
    n = R.ADAM_CAPPED_N
    cfg, it = AdamCfg(), 10
    p, g, m, v = R.adam_inputs(n, device=DEV)
    pd, gd, md, vd = (t.clone() for t in (p, g, m, v))
    sh = torch.full((n,), 3.0, dtype=BF16, device=DEV)
    step = torch.tensor([it], dtype=torch.int64, device=DEV)
    kk.adam(pd, gd, md, vd, sh, step, *cfg.args(), True, True)
    torch.cuda.synchronize()
    R.check_adam((pd, md, vd), p, g, m, v, it, cfg, "capped grid")
    assert bool((sh.view(torch.int16) == pd.to(BF16).view(torch.int16)).all()), "capped grid shadow"
    assert not gd.any() and step.item() == it + 1


# --------------------------------------------------------------------------- to_bf16
@pytest.mark.parametrize("n", R.TO_BF16_N)
def test_to_bf16(n):
    x = R.to_bf16_inputs(n)
    o = torch.full((n + 8,), 3.0, dtype=BF16, device=DEV)
    C().to_bf16(x.to(DEV), o[:n])
    torch.cuda.synchronize()
    R.exact(o[:n], x.to(BF16), f"to_bf16 n={n}")
    assert bool((o[n:] == 3.0).all())
