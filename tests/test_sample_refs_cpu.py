"""The float64 reference of the sampling step (ref_sample.py): every case of
the table is reachable and decided, the reference draws from the distribution
it claims to, and the CPU path of ops.kernels.sample_token equals it."""
import pytest
import torch

import ref_sample as rs
from tensorflow_distributed_on_gke_amd.ops import kernels as K


def _run(c, **over):
    a = dict(temperature=c["T"], top_k=c["top_k"], top_p=c["top_p"], seed=c["seed"], step=c["step"],
             row_id=c["row_id"])
    a.update(over)
    V = c["ref"]["kept"].shape[1]
    return K.sample_token(c["logits"], V, c["score"], c["fin"], rs.END, rs.PAD, **a)


def check_against_ref(c, score, token, fin, rows=None):
    """token / fin equal to the reference on `rows` (default: every row; the
    live ones are decided by construction), ended and dead rows as defined,
    score within 1e-4 max(1, |ref|)."""
    ref = c["ref"]
    rows = torch.ones_like(ref["live"]) if rows is None else rows
    score, token, fin = score.cpu(), token.cpu().long(), fin.cpu().long()
    assert torch.equal(token[rows], ref["token"][rows])
    assert torch.equal(fin[rows], ref["fin"][rows])
    off = ~ref["live"]
    assert (token[off] == rs.PAD).all() and (fin[off] == 1).all()
    ended = c["fin"] != 0
    assert torch.equal(score[ended], c["score"][ended])  # unchanged, bit for bit
    assert (score[off & ~ended] == rs.NINF).all()
    assert not torch.isnan(score[~ended]).any()
    live = ref["live"] & rows
    err = (score.double() - ref["score"])[live].abs()
    assert (err <= 1e-4 * ref["score"][live].abs().clamp(min=1.0)).all()
    return float(err.max()) if err.numel() else 0.0


def _all_cases(V, ldl, R):
    for si in range(rs.N_SETTINGS):
        for kind in rs.KINDS:
            yield si, kind, rs.sample_case(V, ldl, R, si, kind)


@pytest.mark.parametrize("R", rs.ROWS)
@pytest.mark.parametrize("V,ldl", rs.SHAPES)
def test_cases_reachable_and_decided(V, ldl, R):
    for si, kind, c in _all_cases(V, ldl, R):
        ref, tag = c["ref"], (si, kind)
        x = c["logits"][:, :V].float()
        assert (c["logits"][:, V:].float() > 9e3).all(), tag  # 1e4 rounded to bf16
        assert bool(ref["live"].any()), tag
        assert torch.equal(rs.decided(ref), ref["live"]), tag
        assert ((ref["token"] >= 0) & (ref["token"] < V)).all(), tag
        assert ref["kept"][torch.arange(R), ref["token"]][ref["live"]].all(), tag
        assert (x[ref["kept"]] > rs.NINF).all(), "a -inf logit is kept"
        T, top_k, top_p = rs.settings(V)[si]
        assert (c["T"], c["top_k"]) == (T, top_k), tag
        if top_p == rs.P_STAR:
            assert 0.0 < c["top_p"] < 1.0, tag
            assert torch.isfinite(ref["margin"][ref["live"]]).all(), tag
        if kind == "random" and R > 1:
            assert c["score"][1] == rs.NINF and not bool(ref["live"][1]), tag
            assert sorted(c["row_id"].tolist()) == list(range(1000, 1000 + R)), tag
        if kind == "random" and R == 64:
            assert bool((c["fin"] != 0).any()), tag
        if kind == "ties":
            for r in range(R):
                row = x[r]
                assert int((row == row.max()).sum()) >= 2, tag
                if 0 < top_k < V and top_p == 1.0:
                    assert int(ref["kept"][r].sum()) > top_k, (tag, "ties at the threshold are kept")
        if kind == "minus_inf":
            assert int((x == rs.NINF).sum(dim=1).min()) == V // 2, tag
            if R > 1:
                assert bool((x[R - 1] == rs.NINF).all()) and not bool(ref["live"][R - 1]), tag
        if top_k == 1 and kind != "ties":
            best = x.gather(1, ref["token"].view(R, 1)).view(R) == x.max(dim=1).values
            assert best[ref["live"]].all(), tag


def test_big_case_decided():
    V, ldl, R, si, kind = rs.BIG_CASE
    c = rs.sample_case(V, ldl, R, si, kind)
    assert torch.equal(rs.decided(c["ref"]), c["ref"]["live"]) and bool(c["ref"]["live"].any())
    assert c["step"] > 2 ** 32 and c["seed"] > 2 ** 63


@pytest.mark.parametrize("V,ldl,R,si,kind", rs.EDGE_CASES)
def test_edge_cases(V, ldl, R, si, kind):
    c = rs.sample_case(V, ldl, R, si, kind)
    assert torch.equal(rs.decided(c["ref"]), c["ref"]["live"]) and bool(c["ref"]["live"].any())
    check_against_ref(c, *_run(c))


@pytest.mark.parametrize("si", range(rs.N_SETTINGS))
@pytest.mark.parametrize("V", sorted(rs.DIST_ROWS))
def test_reference_is_a_sampler(V, si):
    c = rs.dist_case(V, si)
    ref = c["ref"]
    R = rs.DIST_ROWS[V]
    tok = ref["token"]
    assert ref["kept"][0, tok].all(), "a token outside the kept set"
    probs = rs.kept_probs(c)
    z = rs.chi_square_z(tok, probs)
    und = 1.0 - rs.decided(ref).double().mean().item()
    print(f"V {V} setting {si}: kept {int(ref['kept'][0].sum())}, chi-square z {z:.2f}, "
          f"undecided {und:.4%}")
    assert z < 4.0
    # P(best-two gap < GAP) is about GAP times a density of order 1
    assert und <= 0.01
    if c["top_k"] == 1:
        assert (tok == int(c["logits"][0, :V].float().argmax())).all()
    else:
        assert torch.unique(tok).numel() > 1


@pytest.mark.parametrize("R", rs.ROWS)
@pytest.mark.parametrize("V,ldl", rs.SHAPES)
def test_cpu_path_equals_reference(V, ldl, R):
    worst = 0.0
    for si, kind, c in _all_cases(V, ldl, R):
        worst = max(worst, check_against_ref(c, *_run(c)))
    print(f"max score error {worst:.3e}")


def test_cpu_path_big_case():
    V, ldl, R, si, kind = rs.BIG_CASE
    c = rs.sample_case(V, ldl, R, si, kind)
    check_against_ref(c, *_run(c))


@pytest.mark.parametrize("V", [7, 300])
@pytest.mark.parametrize("si", [0, 3])
def test_cpu_path_distribution_batch(V, si):
    c = rs.dist_case(V, si)
    score, token, fin = _run(c)
    dec = rs.decided(c["ref"])
    check_against_ref(c, score, token, fin, rows=dec)
    assert c["ref"]["kept"][0, token.long()].all()


def test_permutation():
    """Rows permuted together with their row_id: the outputs permute."""
    c = rs.sample_case(300, 304, 64, 3, "random")
    perm = torch.randperm(64, generator=torch.Generator().manual_seed(5))
    a = _run(c)
    b = K.sample_token(c["logits"][perm], 300, c["score"][perm], c["fin"][perm], rs.END, rs.PAD,
                       temperature=c["T"], top_k=c["top_k"], top_p=c["top_p"], seed=c["seed"],
                       step=c["step"], row_id=c["row_id"][perm])
    for x, y in zip(a, b):
        assert torch.equal(x[perm], y)
    # and without row_id the identity is the position
    c2 = rs.sample_case(300, 304, 64, 0, "ties")
    assert c2["row_id"] is None
    for x, y in zip(_run(c2), _run(c2, row_id=torch.arange(64, dtype=torch.int32))):
        assert torch.equal(x, y)


def test_step_and_seed():
    c = rs.dist_case(300, 0)
    base = _run(c)[1]
    assert torch.equal(base, _run(c)[1])
    for over in (dict(step=c["step"] + 1), dict(seed=c["seed"] + 1), dict(step=c["step"] + (1 << 32)),
                 dict(seed=c["seed"] + (1 << 32))):
        other = _run(c, **over)[1]
        assert (other != base).float().mean().item() > 0.25, over


def test_rejects():
    c = rs.sample_case(7, 8, 5, 0, "random")
    for over in (dict(temperature=0.0), dict(temperature=float("inf")), dict(top_p=0.0),
                 dict(top_p=1.5), dict(top_k=-1)):
        with pytest.raises(RuntimeError):
            _run(c, **over)
    with pytest.raises(RuntimeError):
        K.sample_token(c["logits"], 0, c["score"], c["fin"], rs.END, rs.PAD)
    with pytest.raises(RuntimeError):
        K.sample_token(c["logits"], 65537, c["score"], c["fin"], rs.END, rs.PAD)
