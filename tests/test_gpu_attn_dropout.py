"""Attention dropout in the bf16 attention kernels (csrc/kernels/attn_impl.h,
"attention dropout"; the DROP variants of attn_fwd_kernel, attn_bwd_fused_kernel
plain and FDO, attn_bwd_dq_kernel / attn_bwd_dkdv_kernel), run through the
bindings on ref_attn's buffers with B = 2, H = 3, batch row 0 kv_len == 0 and
row 1 a short kv_len, at the tile, 8-key-block and arm edges.

Reference: float64, P = ref_attn.fwd_math's softmax, P~ = P keep / (1 - p) with
keep = philox.keep_mask(seed, ctr 4096 + site, B H Lq Lk8, p) viewed
[B, H, Lq, Lk8] and cut to Lk; O = P~ V; for the backward, from the given
bf16 O~ and f32 lse: dV = P~^T dO, dP = (dO V^T) keep / (1 - p), delta =
rowsum(dO O~), dS = P (dP - delta), dQ = scale dS K, dK = scale dS^T Q.

  exact   ref_attn's selection family at p = 0.5: P is one-hot, so O[q] is
          bitwise 2 keep[q, sel] V[sel], dV the scatter-add of 2 keep dO, dQ and
          dK exactly 0 -- a mask indexed by a tile-local or permuted key, a wrong
          Lk8 or a forward / backward disagreement shows as a wrong element.
  toleranced  "flat" and "peaky" at p = 0.1 (and the uniform kv_len == 0 row of
          every family): ref_attn.close_bf16, |got - ref| <= 2^-8 |ref| + (2^-8 +
          tol) scale, the scales over P~, tol the arm's entry of ref_attn's table.
"""
import pytest
import torch

import ref_attn as A
import ref_tail as R
from tensorflow_distributed_on_gke_amd.ops import kernels as kk
from tensorflow_distributed_on_gke_amd.ops import philox
from tensorflow_distributed_on_gke_amd.ops._ext import C

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
B, H = 2, 3
SEED, CTR, SITE = 0x1234567887654321 >> 1, 3, 2048 + 17

FWD_PTS = [(1, 1, ""), (17, 9, ""), (64, 129, ""), (65, 130, ""), (257, 257, "+causal")]
FUSED_PTS = [(37, 100, ""), (128, 128, "+causal")]
SPLIT_PTS = [(129, 64, ""), (64, 200, ""), (257, 257, "+causal")]
FAMILIES = (("exact", 0.5), ("flat", 0.1), ("peaky", 0.1))


def _case(op, family, hd, Lq, Lk, causal):
    kv = (0, max(1, (2 * Lk + 2) // 3))
    return A.Case(op, family, hd, Lq, Lk, "pad" + causal, kv, "gap", B=B, H=H)


def _arm(op, hd, Lq, Lk):
    """The arm a dropping launch must take: never a pipelined kernel."""
    bh = B * H
    if op == "fwd":
        if Lq > 64:
            return A.Arm("fwd128" if hd <= 64 else "fwd128w8", hd, A.cdiv(Lq, 128) * bh, 256 if hd <= 64 else 512, 0)
        return A.Arm("fwd64", hd, bh, 256, 0)
    if Lq <= 128 and Lk <= 128:
        return A.Arm("bwd_fdo" if op == "fdo" else "bwd_fused", hd, bh, 512, 0)
    return A.Arm("bwd_split", hd, A.cdiv(Lq, 64) * bh, 256, A.cdiv(Lk, 64) * bh)


def _keep_scale(c, p, ctr=CTR, site=SITE):
    Lk8 = A.cdiv(c.Lk, 8) * 8
    keep = philox.keep_mask(SEED, philox.rng_offset(ctr, site), B * H * c.Lq * Lk8, p)
    return keep.view(B, H, c.Lq, Lk8)[..., :c.Lk].to(F64) / (1.0 - p)


def _drop(p, ctr=CTR, site=SITE):
    return (p, SEED, torch.tensor([ctr], dtype=torch.int64, device=DEV), site)


def _fetch(flat):
    torch.cuda.synchronize()
    return {n: t.cpu() for n, t in flat.items()}


def _forward_ref(bt, ks):
    q, k, v = bt.val("q"), bt.val("k"), bt.val("v")
    f = A.fwd_math(bt.case, q, k, v, bt.scale)
    pd = f["P"] * ks
    return f, torch.einsum("bhqk,bkhd->bqhd", pd, v), A._o_scale(pd, v)


def _check_forward(c, p):
    bt = A.build(c)
    ks = _keep_scale(c, p)
    f, O, oscale = _forward_ref(bt, ks)
    flat, v = bt.dev(DEV)
    C().attn_fwd(v["q"], v["k"], v["v"], v["o"], v["lse"], bt.kv_dev(DEV), bt.scale, c.causal, *_drop(p))
    assert A.plan_arm(C().attn_last_plan()) == _arm("fwd", c.hd, c.Lq, c.Lk), c.what()
    after = _fetch(flat)
    A.check_guards(bt, after)
    got_o, what = bt.view("o", after), c.what() + f" p={p}"
    A.close_bf16(got_o, O, oscale, "attn_o", what + " O")
    zmax = f["z"].abs().masked_fill(~f["att"], 0.0).max(-1).values
    R.close_f32(bt.view("lse", after), f["lse"], "attn_lse", what + " lse", scale=zmax)  # (the undropped P's)
    if bt.exact_rows is not None:  # O[q] = keep[q, sel] / (1 - p) * V[sel], bitwise
        rows = bt.exact_rows
        kq = torch.gather(ks, 3, bt.sel.unsqueeze(-1)).permute(0, 2, 1, 3)
        A._same_values(got_o[rows], (A.exact_expect(bt)["O"] * kq)[rows], what + " O (kept selected V rows)")


def _check_backward(c, p):
    bt = A.build(c)
    ks = _keep_scale(c, p)
    q, k, v = bt.val("q"), bt.val("k"), bt.val("v")
    _, O, _ = _forward_ref(bt, ks)
    bt.view("o").copy_(O.to(torch.bfloat16))  # the dropped forward's output (the built one is the plain O)
    flat, dv_ = bt.dev(DEV)
    args = (dv_["lse"], dv_["delta"], dv_["dq"], dv_["dk"], dv_["dv"], bt.kv_dev(DEV), bt.scale, c.causal, *_drop(p))
    if c.op == "fdo":
        assert C().attn_bwd_fdo(dv_["q"], dv_["k"], dv_["v"], dv_["o"], dv_["dy2"], dv_["wo"], *args), c.what()
        do = kk.linear_dgrad(dv_["dy2"], dv_["wo"], H * c.hd).view(B, c.Lq, H, c.hd).cpu().to(F64)
    else:
        C().attn_bwd(dv_["q"], dv_["k"], dv_["v"], dv_["o"], dv_["do"], *args)
        do = bt.val("do")
    assert A.plan_arm(C().attn_last_plan()) == _arm(c.op, c.hd, c.Lq, c.Lk), c.what()
    after = _fetch(flat)
    A.check_guards(bt, after)
    o_in, s = bt.val("o"), bt.scale
    r = A.bwd_math(c, q, k, v, o_in, do, bt.val("lse"), s)  # P (undropped) and delta = rowsum(dO O~)
    P, pd = r["P"], r["P"] * ks
    dS = P * (torch.einsum("bqhd,bkhd->bhqk", do, v) * ks - r["delta"].unsqueeze(-1))
    ref = dict(dv=torch.einsum("bhqk,bqhd->bkhd", pd, do), dq=s * torch.einsum("bhqk,bkhd->bqhd", dS, k),
               dk=s * torch.einsum("bhqk,bqhd->bkhd", dS, q))
    gs = A.grad_scales(dict(P=pd, dS=dS), q, k, v, o_in, do, s)  # (the scale terms over P~)
    what = c.what() + f" p={p}"
    got = lambda n: bt.view(n, after)  # noqa: E731
    A.close_bf16(got("dv"), ref["dv"], gs["dv"], "attn_dv", what + " dV")
    A.close_bf16(got("dq"), ref["dq"], gs["dq"], "attn_dq", what + " dQ", gs["dq32"])
    A.close_bf16(got("dk"), ref["dk"], gs["dk"], "attn_dk", what + " dK", gs["dk32"])
    if bt.exact_rows is not None:  # dV = scatter-add of keep / (1 - p) * dO onto the selected keys, bitwise
        rows = bt.exact_rows
        kq = torch.gather(ks, 3, bt.sel.unsqueeze(-1)).permute(0, 2, 1, 3)
        A._same_values(got("dv")[rows], A.exact_expect(bt, do * kq)["dv"][rows], what + " dV (scatter of kept dO)")
        for n in ("dq", "dk"):
            A._same_values(got(n)[rows], torch.zeros_like(got(n)[rows]), what + f" {n} (exactly 0)")


@pytest.mark.parametrize("hd", (16, 64, 128))
def test_forward(hd):
    for Lq, Lk, causal in FWD_PTS:
        for family, p in FAMILIES:
            _check_forward(_case("fwd", family, hd, Lq, Lk, causal), p)


@pytest.mark.parametrize("op,hd,pts", [("bwd", 16, FUSED_PTS), ("bwd", 64, FUSED_PTS), ("bwd", 128, FUSED_PTS),
                                       ("fdo", 64, FUSED_PTS), ("bwd", 16, SPLIT_PTS), ("bwd", 64, SPLIT_PTS),
                                       ("bwd", 128, SPLIT_PTS)])
def test_backward(op, hd, pts):
    for Lq, Lk, causal in pts:
        for family, p in FAMILIES:
            _check_backward(_case(op, family, hd, Lq, Lk, causal), p)


def test_identity_and_freshness():
    """Drop off is the launch without the argument, bitwise; one (seed, ctr,
    site) gives one mask; another counter step or site another."""
    c = _case("fwd", "flat", 64, 65, 130, "")
    bt = A.build(c)

    def run(*drop):
        flat, v = bt.dev(DEV)
        C().attn_fwd(v["q"], v["k"], v["v"], v["o"], v["lse"], bt.kv_dev(DEV), bt.scale, c.causal, *drop)
        return _fetch(flat)

    plain, off = run(), run(*_drop(0.0))
    a, b = run(*_drop(0.1)), run(*_drop(0.1))
    for n in bt.outputs():
        R.exact(off[n], plain[n], f"{n}: p = 0 vs no dropout argument")
        R.exact(b[n], a[n], f"{n}: the same (seed, ctr, site) twice")
    for other in (_drop(0.1, ctr=CTR + 1), _drop(0.1, site=SITE + 1)):
        o2 = bt.view("o", run(*other))
        assert not torch.equal(o2, bt.view("o", a)) and not torch.equal(bt.view("o", a), bt.view("o", plain))
