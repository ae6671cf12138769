"""The CPU (f32) paths of ops.kernels.decode_attn / beam_topk against the
float64 references of ref_decode.py, on the case tables the GPU tests use."""
import pytest
import torch

import ref_decode as rd
from tensorflow_distributed_on_gke_amd.ops import kernels as K


def _call(c, **kw):
    f = lambda x: None if x is None else x.float()
    return K.decode_attn(c["q"].float(), f(kw.get("k", c["k"])), f(kw.get("v", c["v"])), c["kv_len"],
                         c["scale"], anc=c["anc"], row_map=c.get("row_map"),
                         k_new=f(kw.get("k_new")), v_new=f(kw.get("v_new")))


@pytest.mark.parametrize("hd,H,R,Lk", rd.ATTN_SHAPES)
def test_decode_attn_cpu(hd, H, R, Lk):
    for variant in rd.ATTN_VARIANTS:
        c = rd.attn_case(hd, H, R, Lk, variant)
        ref = rd.attn_ref(c)
        out = _call(c).double()
        assert out.shape == (R, H, hd) and torch.isfinite(out).all(), variant
        # f32 arithmetic, output not rounded: well inside the kernels' bound
        assert ((out - ref).abs() <= rd.attn_bound(ref, c["vmax"])).all(), variant


@pytest.mark.parametrize("hd,H,R,Lk", rd.ATTN_SHAPES)
def test_decode_attn_fused_append_cpu(hd, H, R, Lk):
    for with_anc in (False, True):
        c = rd.fused_case(hd, H, R, Lk, with_anc)
        plain = _call(c, k=c["k_ready"], v=c["v_ready"])
        k, v = c["k"].float(), c["v"].float()
        fused = _call(c, k=k, v=v, k_new=c["k_new"], v_new=c["v_new"])
        assert torch.equal(fused, plain)
        assert torch.equal(k, c["k_ready"].float()) and torch.equal(v, c["v_ready"].float())


@pytest.mark.parametrize("V,ldl,beam,B", rd.TOPK_SHAPES)
def test_beam_topk_cpu(V, ldl, beam, B):
    for kind in rd.TOPK_KINDS:
        c = rd.topk_case(V, ldl, beam, B, kind)
        r_score, r_parent, r_token, r_fin, vals = c["ref"]
        assert rd.gaps_ok(vals, kind == "ties"), kind
        score, parent, token, fin, _ = K.beam_topk(c["logits"].float(), V, c["score"], c["fin"], beam,
                                                   rd.END, rd.PAD)
        assert not torch.isnan(score).any()
        assert torch.equal(token.long(), r_token) and torch.equal(parent.long(), r_parent), kind
        assert torch.equal(fin.long(), r_fin), kind
        dead = r_score == float("-inf")
        assert torch.equal(score == float("-inf"), dead), kind
        err = (score.double() - r_score)[~dead].abs()
        assert (err <= 1e-4 * r_score[~dead].abs().clamp(min=1.0)).all(), kind


def test_beam_topk_ancestry_cpu():
    """anc'[r, :t+1] = anc[parent[r], :t+1]; anc'[r, t+1] = r."""
    V, ldl, beam, B = 300, 304, 4, 3
    c = rd.topk_case(V, ldl, beam, B, "random")
    R, t = B * beam, 5
    g = torch.Generator().manual_seed(0)
    anc = torch.randint(R, (R, 9), generator=g).to(torch.int32)
    _, parent, _, _, new = K.beam_topk(c["logits"].float(), V, c["score"], c["fin"], beam, rd.END, rd.PAD,
                                       anc=anc, t=t)
    assert torch.equal(parent.long(), c["ref"][1])
    assert torch.equal(new[:, : t + 1], anc[parent.long(), : t + 1])
    assert torch.equal(new[:, t + 1], torch.arange(R, dtype=torch.int32))


def test_limits_cpu():
    c = rd.topk_case(7, 8, 1, 1, "random")
    with pytest.raises(RuntimeError):
        K.beam_topk(c["logits"].float().repeat(9, 1), 7, torch.zeros(9), torch.zeros(9, dtype=torch.int32),
                    9, rd.END, rd.PAD)
