"""The distillation loss kernel (csrc/kernels/distill.hip, tdg_xent_distill)
on the MI355X against the float64 reference of tests/ref_distill.py: both
arms at every edge, 1 to 8 teachers with their own row strides and poisoned
padding, both label dtypes, and what the kernel must leave untouched.
tests/test_distill_refs_cpu.py shows on the CPU that the comparators used here
reject every mutant listed in ref_distill.py."""
import functools
import math

import pytest
import torch

import ref_distill as D
import ref_tail as R
from ref_tail import F32
from tensorflow_distributed_on_gke_amd.ops import kernels as kk
from tensorflow_distributed_on_gke_amd.ops._ext import C

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    print("\nkernel worst / tolerance (unit of E32 x 8):", R.report())


@functools.lru_cache(maxsize=None)
def _case(V, ldl, T):
    return D.teacher_rows(V, ldl, T)


def _ref(V, ldl, T, alpha, smoothing, workers):
    lg, lab, te = _case(V, ldl, T)
    return D.ref_xent_distill(lg[:, :V], [t[:, :V] for t in te], lab, workers, smoothing, alpha,
                              D.WEIGHTS[T])


def _place(t, offset=0):
    """A copy of the 2-d tensor on the GPU, `offset` elements into its buffer."""
    M, ld = t.shape
    buf = torch.zeros(offset + M * ld, dtype=t.dtype, device=DEV)
    x = buf[offset:].view(M, ld)
    x.copy_(t)
    assert x.is_contiguous() and x.data_ptr() % 16 == (2 * offset) % 16
    return x


def _run(lg, te, V, lab, workers, smoothing, alpha, weights, write_grad=True, offset=0, row_label=True):
    """The kernel on copies of the student (placed `offset` elements into its
    buffer) and the teachers. Returns (row_loss, row_label, row_correct,
    ntok, student after the call) on the CPU; the teachers must come back
    bitwise unchanged."""
    M = lg.shape[0]
    x = _place(lg, offset)
    td = [_place(t) for t in te]
    labd = lab.to(DEV)
    ntok = torch.full((1,), -1.0, device=DEV)
    kk.count_tokens(labd, ntok)
    rl, rb, rc = (torch.full((M,), float("nan"), device=DEV) for _ in range(3))
    kk.xent_distill(x, td, V, labd, ntok, workers, smoothing, alpha, weights, rl, rc,
                    rb if row_label else None, write_grad)
    torch.cuda.synchronize()
    for m, (a, b) in enumerate(zip(td, te)):
        R.exact(a, b, f"teacher {m} after the call (poisoned padding included)")
    return rl.cpu(), rb.cpu(), rc.cpu(), ntok.item(), x.cpu()


@pytest.mark.parametrize("workers", D.WORKERS)
@pytest.mark.parametrize("smoothing", D.SMOOTHING)
@pytest.mark.parametrize("alpha", D.ALPHAS)
@pytest.mark.parametrize("V,ldl,offset,T", D.CASES)
def test_distill_every_arm(V, ldl, offset, T, alpha, smoothing, workers):
    lg, lab, te = _case(V, ldl, T)
    out = _run(lg, te, V, lab, workers, smoothing, alpha, D.WEIGHTS[T], offset=offset)
    what = f"{D.expected_arm(V, ldl, offset)} V={V} ldl={ldl} T={T} a={alpha} s={smoothing} w={workers}"
    D.check(out, V, _ref(V, ldl, T, alpha, smoothing, workers), lg, workers, what)
    # row_label is what the plain kernel writes as row_loss on the same logits
    x = _place(lg, offset)
    labd = lab.to(DEV)
    ntok = torch.tensor([out[3]], device=DEV)
    rl, rc = torch.empty(lg.shape[0], device=DEV), torch.empty(lg.shape[0], device=DEV)
    kk.xent(x, V, labd, ntok, workers, smoothing, rl, rc, write_grad=False)
    R.close_f32(out[1], rl.cpu(), "row_loss", what + " row_label vs xent", scale=R.row_loss_scale(lg[:, :V]))
    R.exact(out[2], rc.cpu(), what + " row_correct vs xent")


@pytest.mark.parametrize("V,ldl,offset", [(250, 256, 0), (7010, 7040, 0), (7010, 7040, 2), (8193, 8200, 0)])
def test_distill_label_dtypes_bitwise_equal(V, ldl, offset):
    lg, lab, te = _case(V, ldl, 2)
    a = _run(lg, te, V, lab, 2.0, 0.1, 0.5, D.WEIGHTS[2], offset=offset)
    b = _run(lg, te, V, lab.to(torch.int32), 2.0, 0.1, 0.5, D.WEIGHTS[2], offset=offset)
    D.check(b, V, _ref(V, ldl, 2, 0.5, 0.1, 2.0), lg, 2.0, f"int32 labels V={V}")
    assert a[3] == b[3]
    for k, name in ((0, "row_loss"), (1, "row_label"), (2, "row_correct"), (4, "dlogits")):
        R.exact(b[k], a[k], f"int32 vs int64 labels: {name}")


@pytest.mark.parametrize("smoothing", D.SMOOTHING)
@pytest.mark.parametrize("V,ldl,offset", D.SHAPES)
def test_distill_alpha_zero_is_xent(V, ldl, offset, smoothing):
    """alpha = 0 against ref_tail.ref_xent through the plain kernel's comparators."""
    lg, lab, te = _case(V, ldl, 2)
    out = _run(lg, te, V, lab, 2.0, smoothing, 0.0, D.WEIGHTS[2], offset=offset)
    loss, correct, ntok, d = R.ref_xent(lg[:, :V], lab, 2.0, smoothing)
    what = f"alpha=0 V={V} ldl={ldl} s={smoothing}"
    assert out[3] == ntok
    sc = R.row_loss_scale(lg[:, :V])
    R.close_f32(out[0], loss, "row_loss", what + " row_loss", scale=sc)
    R.close_f32(out[1], loss, "row_loss", what + " row_label", scale=sc)
    R.exact(out[2], correct.to(F32), what + " row_correct")
    R.close_dlogits(out[4], d, V, R.xent_scale(ntok, 2.0), what + " dlogits")


@pytest.mark.parametrize("V,ldl,offset", [(250, 256, 0), (7010, 7040, 0), (7010, 7040, 2), (8193, 8200, 0)])
def test_distill_teacher_equal_to_student_has_no_gradient(V, ldl, offset):
    """One teacher, alpha = 1, s = 0, teacher == student: p - q = 0, so every
    element lies within the absolute term of the gradient tolerance."""
    lg, lab = R.xent_rows(V, ldl)
    out = _run(lg, [lg], V, lab, 1.0, 0.0, 1.0, None, offset=offset)
    bound = R.tol("distill_dlogits") * R.xent_scale(out[3], 1.0)
    worst = float(out[4].float().abs().max())
    assert worst <= bound, f"|dlogits| {worst:.3e} > {bound:.3e}"
    # the objective is then the student's entropy: lse - sum p x
    ref = D.ref_xent_distill(lg[:, :V], [lg[:, :V]], lab, 1.0, 0.0, 1.0)
    R.close_f32(out[0], ref[0], "distill_row_loss", "entropy", scale=R.row_loss_scale(lg[:, :V]))


@pytest.mark.parametrize("V,ldl,offset", [(250, 256, 0), (7010, 7040, 0), (7010, 7040, 2), (8193, 8200, 0),
                                          (33, 34, 0)])
def test_distill_without_gradient(V, ldl, offset):
    lg, lab, te = _case(V, ldl, 3)
    a = _run(lg, te, V, lab, 2.0, 0.1, 0.5, D.WEIGHTS[3], write_grad=True, offset=offset)
    b = _run(lg, te, V, lab, 2.0, 0.1, 0.5, D.WEIGHTS[3], write_grad=False, offset=offset)
    R.exact(b[4], lg, "student after write_grad=False (poisoned padding included)")
    for k, name in ((0, "row_loss"), (1, "row_label"), (2, "row_correct")):
        R.exact(b[k], a[k], f"{name} with and without the gradient")
    c = _run(lg, te, V, lab, 2.0, 0.1, 0.5, D.WEIGHTS[3], offset=offset, row_label=False)
    R.exact(c[0], a[0], "row_loss without row_label")
    R.exact(c[4], a[4], "dlogits without row_label")
    assert bool(torch.isnan(c[1]).all()), "row_label written although not passed"


@pytest.mark.parametrize("V,ldl", [(250, 256), (5000, 5056), (8193, 8200), (33, 34)])
def test_distill_all_pad(V, ldl):
    lg, lab, te = _case(V, ldl, 2)
    out = _run(lg, te, V, torch.zeros_like(lab), 2.0, 0.1, 0.5, D.WEIGHTS[2])
    assert out[3] == 0.0
    for k, name in ((0, "row_loss"), (1, "row_label"), (2, "row_correct"), (4, "dlogits")):
        assert bool((out[k].float() == 0).all()), f"all PAD: {name} not all zero"


def test_distill_launcher_refuses():
    """T = 0, T = 9 and alpha = 1.5 reach the launcher, which returns -1 and
    launches nothing; the wrapper refuses them before."""
    V, ldl = 250, 256
    lg, lab, te = _case(V, ldl, 1)
    M = lg.shape[0]
    x, t = _place(lg), _place(te[0])
    labd = lab.to(DEV)
    ntok = torch.ones(1, device=DEV)
    rl, rc = torch.zeros(M, device=DEV), torch.zeros(M, device=DEV)
    lw = math.log(1 / 9)
    for teachers, alpha, logw in (([], 0.5, []), ([t] * 9, 0.5, [lw] * 9), ([t], 1.5, [0.0])):
        with pytest.raises(RuntimeError, match="rc=-1"):
            C().xent_distill(x, teachers, V, labd, ntok, 1.0, 0.1, alpha, logw, rl, rc, None, True)
        with pytest.raises(RuntimeError, match="xent_distill"):
            kk.xent_distill(x, teachers, V, labd, ntok, 1.0, 0.1, alpha, None, rl, rc)
    torch.cuda.synchronize()
    R.exact(x, lg, "student after refused calls")
    assert not bool(rl.any()) and not bool(rc.any())
