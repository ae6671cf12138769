"""The R-Drop paired-row loss kernel (csrc/kernels/rdrop.hip) on the MI355X
against the float64 reference of tests/ref_rdrop.py: every NCH of the register
arm, the generic arm by length, stride and alignment, both label dtypes, and
what the kernel must leave untouched."""
import functools

import pytest
import torch

import ref_rdrop as D
import ref_tail as R
from tensorflow_distributed_on_gke_amd.ops import kernels as kk
from tensorflow_distributed_on_gke_amd.ops._ext import C
from tensorflow_distributed_on_gke_amd.ops.kernels.loss import xent_rdrop

pytestmark = pytest.mark.gpu
DEV = "cuda"
FEW = [(250, 256, 0), (7010, 7040, 0), (8193, 8200, 0), (33, 34, 0), (7010, 7040, 2)]
_case = functools.lru_cache(maxsize=None)(D.pair_rows)


def _run(lg2, V, lab2, workers, smoothing, alpha, write_grad=True, offset=0):
    """The kernel on a copy of the logits placed `offset` elements into its
    buffer: (row_loss, row_label, row_correct, ntok, logits after) on the CPU."""
    R2, ld = lg2.shape
    x = torch.zeros(offset + R2 * ld, dtype=lg2.dtype, device=DEV)[offset:].view(R2, ld)
    x.copy_(lg2)
    labd = lab2.to(DEV)
    ntok = torch.full((1,), -1.0, device=DEV)
    kk.count_tokens(labd, ntok)
    rl, rb, rc = (torch.full((R2,), float("nan"), device=DEV) for _ in range(3))
    xent_rdrop(x, V, labd, ntok, workers, smoothing, alpha, rl, rc, rb, write_grad)
    torch.cuda.synchronize()
    return rl.cpu(), rb.cpu(), rc.cpu(), ntok.item(), x.cpu()


@pytest.mark.parametrize("workers", D.WORKERS)
@pytest.mark.parametrize("smoothing", D.SMOOTHING)
@pytest.mark.parametrize("alpha", D.ALPHAS)
@pytest.mark.parametrize("V,ldl,offset", D.SHAPES)
def test_rdrop_every_arm(V, ldl, offset, alpha, smoothing, workers):
    lg2, lab2 = _case(V, ldl)
    out = _run(lg2, V, lab2, workers, smoothing, alpha, offset=offset)
    ref = D.ref_rdrop(lg2[:, :V], lab2, workers, smoothing, alpha)
    D.check(out, V, ref, lg2, alpha, workers, f"V={V} ldl={ldl} off={offset} a={alpha} s={smoothing} w={workers}")


@pytest.mark.parametrize("V,ldl,offset", FEW)
def test_rdrop_label_dtypes_and_no_gradient(V, ldl, offset):
    """int32 and int64 labels agree bitwise; write_grad=0 leaves the logits
    (poisoned padding included) untouched and writes the same row outputs."""
    lg2, lab2 = _case(V, ldl)
    a = _run(lg2, V, lab2, 2.0, 0.1, 5.0, offset=offset)
    b = _run(lg2, V, lab2.to(torch.int32), 2.0, 0.1, 5.0, offset=offset)
    c = _run(lg2, V, lab2, 2.0, 0.1, 5.0, write_grad=False, offset=offset)
    R.exact(c[4], lg2, "logits after write_grad=False")
    for k, name in ((0, "row_loss"), (1, "row_label"), (2, "row_correct"), (4, "dlogits")):
        R.exact(b[k], a[k], f"int32 vs int64 labels: {name}")
        if k != 4:
            R.exact(c[k], a[k], f"{name} with and without the gradient")


@pytest.mark.parametrize("V,ldl,offset", FEW)
def test_rdrop_equal_pair_has_no_consistency_part(V, ldl, offset):
    """Both copies the same bits: KL exactly 0, row_loss == row_label, and the
    two gradient rows equal each other and the plain cross entropy's."""
    lg, lab = R.xent_rows(V, ldl)
    M = lg.shape[0]
    out = _run(torch.cat([lg, lg]), V, torch.cat([lab, lab]), 1.0, 0.1, 5.0, offset=offset)
    R.exact(out[0], out[1], "row_loss vs row_label of equal pairs")
    R.exact(out[4][M:], out[4][:M], "gradient of copy 2 vs copy 1")
    _, _, ntok, d = R.ref_xent(lg[:, :V], lab, 1.0, 0.1)
    R.close_dlogits(out[4][:M], d / 2, V, R.xent_scale(2 * ntok, 1.0), "equal pairs vs plain xent")


@pytest.mark.parametrize("V,ldl", [(250, 256), (7010, 7040), (8193, 8200), (33, 34)])
def test_rdrop_all_pad(V, ldl):
    lg2, lab2 = _case(V, ldl)
    out = _run(lg2, V, torch.zeros_like(lab2), 2.0, 0.1, 5.0)
    assert out[3] == 0.0
    for k, name in ((0, "row_loss"), (1, "row_label"), (2, "row_correct"), (4, "dlogits")):
        assert bool((out[k].float() == 0).all()), f"all PAD: {name} not all zero"


def test_rdrop_launcher_refuses():
    """alpha < 0, NaN alpha and V > 65536 reach the launcher as -1 (the wrapper
    refuses them before), a row shorter than V as -2; nothing is launched."""
    V, ldl = 250, 256
    lg2, lab2 = _case(V, ldl)
    x, labd, ntok = lg2.to(DEV), lab2.to(DEV), torch.ones(1, device=DEV)
    rl, rc = torch.zeros(lg2.shape[0], device=DEV), torch.zeros(lg2.shape[0], device=DEV)
    for v, alpha, rc_want in ((V, -1.0, -1), (V, float("nan"), -1), (65537, 1.0, -1), (ldl + 1, 1.0, -2)):
        with pytest.raises(RuntimeError, match=f"rc={rc_want}"):
            C().xent_rdrop(x, v, labd, ntok, 1.0, 0.1, alpha, rl, rc, None, True)
        if rc_want == -1:
            with pytest.raises(RuntimeError, match="xent_rdrop"):
                xent_rdrop(x, v, labd, ntok, 1.0, 0.1, alpha, rl, rc)
    none = torch.empty(0, device=DEV)  # M = 0: a successful no-op
    xent_rdrop(none.bfloat16().view(0, ldl), V, none.long(), ntok, 1.0, 0.1, 1.0, none, none)
    torch.cuda.synchronize()
    R.exact(x, lg2, "logits after refused calls")
    assert not bool(rl.any()) and not bool(rc.any())
