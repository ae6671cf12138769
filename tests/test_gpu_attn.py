"""The bf16 attention family on the MI355X (attn_impl.h, attn_fwd.h, attn_bwd.h,
attn_qkv.h) against exact and float64 references. References, case tables,
comparators and the tolerance table are tests/ref_attn.py's;
tests/test_attn_refs_cpu.py shows on the CPU that those comparators reject
every mutant listed there on these very tables, that the backward formulas are
float64 autograd of the forward, and that the tables reach every arm and edge
named below.

Every launch here runs on strided views of NaN-padded inputs with finite trap
rows outside the key windows, writes into sentinel-filled buffers
(ref_attn.build), is checked for untouched guards and a fully written
interior, and asserts that the arm its launcher recorded (attn_last_plan) is
ref_attn.expected_arm of the case: a case named after a kernel cannot silently
test another after a dispatch change. The backward is given o = bf16(ref O)
and lse = f32(ref lse), never the kernel's own forward; test_chained feeds the
kernel's forward into the kernel's backward on top of that.

Which test reaches which arm:
  attn_fwd_kernel<HD, 4, 64, 1>, Lq <= 64: Lq 1..64 x Lk 1..129
    (1 to 3 key tiles, the online rescale)                test_forward[fwd64-*]
  attn_fwd_kernel<HD, 4, 128, 2> (hd <= 64) and <128, 8, 128, 1>:
    Lq 65..257 x Lk 1..257, causal at 65 / 128 / 129      test_forward[fwd128*-*]
  attn_fwd_pipe_kernel (hd 64, Lq > 128): 1 to 5 key tiles through the
    3-slot ring, the unconditional prologue at Lk <= 128  test_forward[fwd_pipe-64]
  attn_probs_kernel: Lk at and around the 64-lane stride,
    a causal kv_len == 0 row                              test_probs
  attn_bwd_fused_kernel (Lq, Lk <= 128), every head dim:
    one-row and one-key problems, the 16 U w >= Lq exit   test_backward[bwd_fused-*]
  the same with the output-projection dgrad in-kernel,
    bitwise against linear_dgrad + attn_bwd               test_backward_fdo
  attn_bwd_dq_kernel / attn_bwd_dkdv_kernel (hd 16, 32,
    128; Lq or Lk > 128)                                  test_backward[bwd_split-*]
  attn_bwd_dq_pipe_kernel / attn_bwd_dkdv_pipe_kernel (hd 64): Lq > 128 over
    Lk <= 64 and the reverse, 1 to 6 tiles through the
    4-slot rings                                          test_backward[bwd_pipe-64]
  qkv_attn_fwd_kernel, self: d = 64 / 128 / 192 (1, 2, 3 projection K
    tiles over its 2 stages), bitwise against
    linear_fwd + attn_fwd                                 test_qkv[qkv_self-*]
  qkv_attn_fwd_kernel, cross (3 stages), K / V in the
    batched [B, S, layers 2d] buffer                      test_qkv[qkv_cross-*]
  kernel forward into kernel backward, every backward arm test_chained
  "no atomics, deterministic" (attn_impl.h header)        test_backward_is_deterministic
"""
import pytest
import torch

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


def _assert_arm(c):
    arm = A.plan_arm(C().attn_last_plan())
    assert arm == c.arm, f"{c.what()}: launched {arm}, the case expects {c.arm}"


def _fetch(flat):
    torch.cuda.synchronize()
    return {p: t.cpu() for p, t in flat.items()}


def _forward(bt):
    c = bt.case
    flat, v = bt.dev(DEV)
    C().attn_fwd(v["q"], v["k"], v["v"], v["o"], v["lse"], bt.kv_dev(DEV), bt.scale, c.causal)
    _assert_arm(c)
    return _fetch(flat)


def _backward(bt, o=None, lse=None, dout=None):
    """attn_bwd on the case's buffers (o / lse / dout: given instead of the
    built ones). Returns the buffers after the launch."""
    c = bt.case
    flat, v = bt.dev(DEV)
    C().attn_bwd(v["q"], v["k"], v["v"], v["o"] if o is None else o, v["do"] if dout is None else dout,
                 v["lse"] if lse is None else lse, v["delta"], v["dq"], v["dk"], v["dv"], bt.kv_dev(DEV),
                 bt.scale, c.causal)
    assert A.plan_arm(C().attn_last_plan()) == A.expected_arm("bwd", c.hd, c.Lq, c.Lk, c.B, c.H), c.what()
    return _fetch(flat)


FWD = [(arm, hd) for arm in ("fwd64", "fwd128", "fwd128w8", "fwd_pipe") for hd in A.ARM_HDS[arm]]
BWD = [(arm, hd) for arm in ("bwd_fused", "bwd_split", "bwd_pipe") for hd in A.ARM_HDS[arm]]


@pytest.mark.parametrize("arm,hd", FWD)
def test_forward(arm, hd):
    for c in A.cases(arm, hd):
        bt = A.build(c)
        A.check(bt, _forward(bt))


@pytest.mark.parametrize("hd", A.ARM_HDS["probs"])
def test_probs(hd):
    for c in A.cases("probs", hd):
        bt = A.build(c)
        flat, v = bt.dev(DEV)
        C().attn_probs(v["q"], v["k"], v["probs"], bt.kv_dev(DEV), bt.scale, c.causal)
        _assert_arm(c)
        A.check(bt, _fetch(flat))


@pytest.mark.parametrize("arm,hd", BWD)
def test_backward(arm, hd):
    for c in A.cases(arm, hd):
        bt = A.build(c)
        A.check(bt, _backward(bt))


def test_backward_fdo():
    """attn_bwd_fused_kernel<64, 1, true>: against float64 from the dO that
    linear_dgrad stores, and bitwise against attn_bwd on that dO."""
    for c in A.cases("bwd_fdo", 64):
        bt = A.build(c)
        flat, v = bt.dev(DEV)
        assert C().attn_bwd_fdo(v["q"], v["k"], v["v"], v["o"], v["dy2"], v["wo"], v["lse"], v["delta"], v["dq"],
                                v["dk"], v["dv"], bt.kv_dev(DEV), bt.scale, c.causal), c.what()
        _assert_arm(c)
        fused = _fetch(flat)
        d = c.H * c.hd
        dout = kk.linear_dgrad(v["dy2"], v["wo"], d).view(c.B, c.Lq, c.H, c.hd)
        A.check(bt, fused, dout=dout)
        two = _backward(bt, dout=dout)
        for p in bt.outputs():
            R.exact(fused[p], two[p], f"{c.what()}: {p}, fused dgrad vs linear_dgrad + attn_bwd")


@pytest.mark.parametrize("arm,H", [(arm, H) for arm in ("qkv_self", "qkv_cross") for H in (1, 2, 3)])
def test_qkv(arm, H):
    """The projection against the float64 GEMM reference, the attention
    against float64 from the kernel's own bf16 projection, and both bitwise
    against linear_fwd + attn_fwd wherever the two paths round alike: not at
    Lq <= 64 over Lk >= 64, where attn_fwd_kernel<64, 4, 64, 1> takes 64-key
    tiles -- several with the online rescale, or one whole tile through
    softmax_max's unmasked branch (c folded into the exponent's FMA) -- and the
    fused kernel one 128-key tile through the masked one (logits scaled first)."""
    for c in A.cases(arm, 64, H):
        bt = A.build(c)
        flat, v = bt.dev(DEV)
        cross = arm == "qkv_cross"
        assert C().qkv_attn_fwd(v["x"], v["w"], v["bias"], v["qkv"], v["o"], v["lse"], bt.kv_dev(DEV), bt.scale,
                                c.causal, c.B, c.H, v["k"] if cross else None, v["v"] if cross else None), c.what()
        _assert_arm(c)
        after = _fetch(flat)
        A.check(bt, after)
        proj = kk.linear_fwd(v["x"], v["w"], v["bias"])
        if cross:
            q, k, vv = proj.view(c.B, c.Lq, c.H, c.hd), v["k"], v["v"]
        else:
            p5 = proj.view(c.B, c.Lq, 3, c.H, c.hd)
            q, k, vv = p5[:, :, 0], p5[:, :, 1], p5[:, :, 2]
        o0, lse0 = kk.attn_fwd(q, k, vv, bt.kv_dev(DEV), bt.scale, c.causal)
        torch.cuda.synchronize()
        R.exact(bt.view("qkv", after), proj.cpu(), c.what() + ": projection vs linear_fwd")
        if c.Lq > 64 or c.Lk < 64:
            R.exact(bt.view("o", after).contiguous(), o0.cpu(), c.what() + ": O vs linear_fwd + attn_fwd")
            R.exact(bt.view("lse", after).contiguous(), lse0.cpu(), c.what() + ": lse vs linear_fwd + attn_fwd")


CHAIN = [(arm, hd) for arm in ("bwd_fused", "bwd_split", "bwd_pipe") for hd in A.ARM_HDS[arm]] + [("bwd_fdo", 64)]


@pytest.mark.parametrize("arm,hd", CHAIN)
def test_chained(arm, hd):
    """The kernel's own forward (bf16 O, f32 lse) into the kernel's backward:
    the backward reference is a function of the o and lse it is given."""
    for c in A.cases(arm, hd)[1::4]:
        bt = A.build(c)
        flat, v = bt.dev(DEV)
        o, lse = kk.attn_fwd(v["q"], v["k"], v["v"], bt.kv_dev(DEV), bt.scale, c.causal)
        if arm == "bwd_fdo":
            dout = kk.linear_dgrad(v["dy2"], v["wo"], c.H * c.hd).view(c.B, c.Lq, c.H, c.hd)
            assert C().attn_bwd_fdo(v["q"], v["k"], v["v"], o, v["dy2"], v["wo"], lse, v["delta"], v["dq"], v["dk"],
                                    v["dv"], bt.kv_dev(DEV), bt.scale, c.causal)
            _assert_arm(c)
            A.check(bt, _fetch(flat), dout=dout, o=o, lse=lse)
        else:
            A.check(bt, _backward(bt, o=o, lse=lse), o=o, lse=lse)


@pytest.mark.parametrize("arm,hd", CHAIN)
def test_backward_is_deterministic(arm, hd):
    """No atomics: two runs on identical inputs give identical bits."""
    tab = A.cases(arm, hd)
    c = max((c for c in tab if c.family != "exact"), key=lambda c: c.Lq * c.Lk)
    bt = A.build(c)
    runs = []
    for _ in range(2):
        if arm == "bwd_fdo":
            flat, v = bt.dev(DEV)
            assert C().attn_bwd_fdo(v["q"], v["k"], v["v"], v["o"], v["dy2"], v["wo"], v["lse"], v["delta"], v["dq"],
                                    v["dk"], v["dv"], bt.kv_dev(DEV), bt.scale, c.causal)
            runs.append(_fetch(flat))
        else:
            runs.append(_backward(bt))
    for p in bt.outputs():
        R.exact(runs[0][p], runs[1][p], f"{c.what()}: {p}, run 1 vs run 2")
