"""The CPU arm of ops.kernels.decode.score_tokens against the float64 reference of
ref_score.py, and the wrapper's rejections."""
import pytest
import torch

import ref_ensemble as re_
import ref_score as rs
from tensorflow_distributed_on_gke_amd.ops.kernels.decode import score_tokens


@pytest.mark.parametrize("R", re_.ROWS)
@pytest.mark.parametrize("M", re_.MEMBERS)
@pytest.mark.parametrize("V,ld", re_.SHAPES)
def test_score_tokens(V, ld, M, R):
    for kind in re_.KINDS:
        logits, weights, sets = rs.case(V, ld, M, R, kind)
        assert len(sets) >= 2
        seen = torch.cat([s[0] for s in sets])
        assert (seen == rs.PAD).any() and (seen == V).any(), "the forced labels are missing"
        for n, (labels, tok_ref, top_ref) in enumerate(sets):
            for lab in (labels, labels.to(torch.int32)):
                tok, top = score_tokens(list(logits), V, lab, weights, pad_id=rs.PAD, want_top=True)
                assert tok.dtype == top.dtype == torch.float32 and tok.shape == top.shape == (R,)
                e1 = rs.check(tok, tok_ref, (kind, n, "tok"))
                e2 = rs.check(top, top_ref, (kind, n, "top"))
                only, none = score_tokens(list(logits), V, lab, weights, pad_id=rs.PAD)
                assert none is None and torch.equal(only, tok)
            print(f"{kind} set {n}: max err tok {e1:.3e} top {e2:.3e}")
            ignored = labels == rs.PAD
            assert (tok[ignored] == 0).all() and (top[ignored] == 0).all()
            assert (tok <= top).all()


def test_label_that_is_the_argmax_hits():
    """tok_lp >= top_lp exactly where the label is the most probable token:
    the peaked column, far ahead of every other."""
    V, ld = 300, 304
    for M in re_.MEMBERS:
        logits, weights, mix = re_.case(V, ld, M, 5, "peaked")
        best = torch.tensor([(37 * r + 5) % V for r in range(5)])
        assert torch.equal(best, mix.argmax(dim=1))
        tok, top = score_tokens(list(logits), V, best, weights, pad_id=-1, want_top=True)
        assert torch.equal(tok, top)
        tok, top = score_tokens(list(logits), V, (best + 1) % V, weights, pad_id=-1, want_top=True)
        assert (tok < top).all()


def test_other_pad_id():
    V, ld = 300, 304
    logits, weights, mix = re_.case(V, ld, 2, 5, "random")
    labels = torch.tensor([0, 7, 7, 1, 299])
    tok, top = score_tokens(list(logits), V, labels, weights, pad_id=7, want_top=True)
    tok_ref, top_ref = rs.score_ref(mix, labels, pad_id=7)
    rs.check(tok, tok_ref, "tok")
    rs.check(top, top_ref, "top")
    assert tok[1] == 0 and top[2] == 0 and tok[0] < 0


def test_wrapper_rejects():
    x = torch.zeros(2, 8)
    lab = torch.zeros(2, dtype=torch.int64)
    for bad in (dict(logits_list=[]), dict(logits_list=[x] * 9), dict(V=0), dict(V=65537),
                dict(weights=[1.0]), dict(weights=[1.0, 0.0]), dict(weights=[1.0, float("nan")]),
                dict(weights=[1.0, float("inf")]), dict(weights=[1.0, -1.0]),
                dict(labels=lab.float()), dict(labels=lab[:1]), dict(labels=lab.view(2, 1))):
        kw = dict(dict(logits_list=[x, x], V=7, labels=lab, weights=None), **bad)
        with pytest.raises(RuntimeError):
            score_tokens(**kw)
