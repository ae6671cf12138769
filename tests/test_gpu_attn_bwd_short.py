"""The fused short attention backward (attn_bwd.h attn_bwd_fused_kernel, Lq,
Lk <= 128, hd 64) at the row-band edges of its layout, plain and with the
output-projection dgrad in-kernel (FDO), against ref_attn's float64
references and tolerance table; cases, buffers, guards and comparators are
ref_attn's (build, check), as in test_gpu_attn.py.

test_gpu_attn.py's tables cover one-row and one-key problems at B 4, H 3.
Here, at B 2, H 2, in both forms: every L of 1, 15, 16, 17, 31, 32, 33, 63,
64, 65, 96, 127 and 128 (the 16- and 32-row band edges) as Lq against Lk =
128 and Lk = 1, and as Lk against Lq = 128 and Lq = 1, each pair unmasked,
padded, causal and padded + causal (causal with Lq != Lk is the kernel's
window key <= q, as ref_attn defines it for any shape), and the squares
(L, L) causal and padded + causal. The padded cases take kv_len from Lk, 0,
1 and Lk - 1, two of them per case, the start rotating from case to case.
Then: a batch row with kv_len 0 beside a full one; a key window ending
mid-band (kv_len 33 of Lk 64); B 3, H 1 (an odd number of workgroups: two
co-resident ones never pair up evenly); and the FDO form bitwise against
linear_dgrad followed by the plain form at Lq = Lk = 33 and 128. Every
launch asserts the arm its launcher recorded. Nothing the issue lists is
left out: ref_attn's helpers express every case.

That ref_attn's own float32 evaluation (attn_f32) of every case here stays
inside its tolerances is shown on the CPU by
tests/test_attn_bwd_short_cpu.py on the same tables
(tests/attn_bwd_short_cases.py).

The FDO form here has d = 64 H = 128 or 64: two K tiles of its dO GEMM or
one, all issued in the prologue, the attention's operand loads right behind
them. The K loop with stages issued from inside it (d >= 256) runs in
test_gpu_qkv_attn.py's H 8 cases and in the model tests.
"""
import pytest
import torch

import attn_bwd_short_cases as T
import ref_attn as A
import ref_tail as R
from tensorflow_distributed_on_gke_amd.ops import kernels as kk
from tensorflow_distributed_on_gke_amd.ops._ext import C

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    print("\nkernel worst / tolerance (unit of ref_attn.E32 x 8):", A.report())


def _fetch(flat):
    torch.cuda.synchronize()
    return {p: t.cpu() for p, t in flat.items()}


def _plain(bt, dout=None):
    c = bt.case
    flat, v = bt.dev(DEV)
    C().attn_bwd(v["q"], v["k"], v["v"], v["o"], v["do"] if dout is None else dout, v["lse"], v["delta"], v["dq"],
                 v["dk"], v["dv"], bt.kv_dev(DEV), bt.scale, c.causal)
    arm = A.plan_arm(C().attn_last_plan())
    assert arm == A.expected_arm("bwd", c.hd, c.Lq, c.Lk, c.B, c.H), f"{c.what()}: launched {arm}"
    return _fetch(flat)


def _fdo(bt):
    c = bt.case
    flat, v = bt.dev(DEV)
    assert C().attn_bwd_fdo(v["q"], v["k"], v["v"], v["o"], v["dy2"], v["wo"], v["lse"], v["delta"], v["dq"], v["dk"],
                            v["dv"], bt.kv_dev(DEV), bt.scale, c.causal), c.what()
    arm = A.plan_arm(C().attn_last_plan())
    assert arm == c.arm, f"{c.what()}: launched {arm}, the case expects {c.arm}"
    dout = kk.linear_dgrad(v["dy2"], v["wo"], c.H * c.hd).view(c.B, c.Lq, c.H, c.hd)
    return _fetch(flat), dout


@pytest.mark.parametrize("mask", T.MASKS)
def test_plain_band_edges(mask):
    for c in T.table("bwd", mask):
        bt = A.build(c)
        A.check(bt, _plain(bt))


@pytest.mark.parametrize("mask", T.MASKS)
def test_fdo_band_edges(mask):
    """Against float64 from the dO that linear_dgrad stores."""
    for c in T.table("fdo", mask):
        bt = A.build(c)
        after, dout = _fdo(bt)
        A.check(bt, after, dout=dout)


@pytest.mark.parametrize("L", (33, 128))
@pytest.mark.parametrize("mask", ("pad", "pad+causal"))
def test_fdo_bitwise_two_launches(L, mask):
    """The FDO form bitwise against linear_dgrad followed by the plain form."""
    c = A.Case("fdo", "peaky", 64, L, L, mask, (L, max(L - 1, 1)), "gap", 2, 2, seed=7)
    bt = A.build(c)
    fused, dout = _fdo(bt)
    two = _plain(bt, dout=dout)
    for p in bt.outputs():
        R.exact(fused[p], two[p], f"{c.what()}: {p}, fused dgrad vs linear_dgrad + attn_bwd")
