"""tests/ref_distill.py checks itself on the CPU: its comparators accept the
float32 evaluation of the distillation loss on every case of
tests/test_gpu_distill.py, reject every deliberate mutant, and its tolerance
table is what this machine measures."""
import functools
import math

import pytest
import torch

import ref_distill as D
import ref_tail as R
from ref_tail import BF16, F64


@functools.lru_cache(maxsize=None)
def _case(V, ldl, T):
    return D.teacher_rows(V, ldl, T)


def _settings():
    return [(a, s, w) for a in D.ALPHAS for s in D.SMOOTHING for w in D.WORKERS]


def _ref(V, ldl, T, a, s, w, weights):
    lg, lab, te = _case(V, ldl, T)
    return D.ref_xent_distill(lg[:, :V], [t[:, :V] for t in te], lab, w, s, a, weights)


def _accept(V, ldl, T):
    """The worst f32 ratios (row_loss, dlogits) over the case's settings."""
    lg, lab, te = _case(V, ldl, T)
    wl = wd = 0.0
    for a, s, w in _settings():
        ref = _ref(V, ldl, T, a, s, w, D.WEIGHTS[T])
        out = D.xent_distill_f32(lg, te, V, lab, w, s, a, D.WEIGHTS[T], keep_f32=True)
        D.check(out[:4] + (out[4].to(BF16),), V, ref, lg, w, f"f32 V={V} T={T} a={a} s={s} w={w}")
        sc = R.row_loss_scale(lg[:, :V])
        wl = max(wl, float(((out[0].to(F64) - ref[0]).abs() / (ref[0].abs() + sc)).max()))
        wd = max(wd, float((out[4][:, :V].to(F64) - ref[4]).abs().max()) / R.xent_scale(ref[3], w))
    return wl, wd


@functools.lru_cache(maxsize=None)
def _measured():
    got = [_accept(V, ldl, T) for V, ldl, off, T in D.CASES if off == 0]  # an offset is the same data
    return {"distill_row_loss": max(g[0] for g in got), "distill_dlogits": max(g[1] for g in got)}


def test_f32_evaluation_is_accepted_on_every_case():
    _measured()


def test_e32_table_is_measured():
    """Each tolerance is ref_tail.MARGIN x an E32 that this machine
    reproduces: not below what the float32 evaluation needs, not inflated."""
    got = _measured()
    print("measured E32:", {k: f"{v:.2e}" for k, v in sorted(got.items())})
    assert set(got) == set(D.E32)
    for k, e in D.E32.items():
        assert got[k] <= 1.5 * e, f"{k}: measured {got[k]:.3e} above the table's {e:.3e}"
        assert got[k] >= e / 4, f"{k}: the table's {e:.3e} is more than 4x the measured {got[k]:.3e}"
        assert math.isclose(R.tol(k), R.MARGIN * e)
    assert R.MARGIN == 8.0


# the case a mutant must show on: several teachers of unequal weights and
# strides past V, smoothing on, PAD rows present (every case has them)
MUTANT_CASES = [(250, 256, 2), (7010, 7040, 3), (33, 34, 2)]


@pytest.mark.parametrize("mutant", D.DISTILL_MUTANTS)
@pytest.mark.parametrize("V,ldl,T", MUTANT_CASES)
def test_comparators_reject_every_mutant(V, ldl, T, mutant):
    lg, lab, te = _case(V, ldl, T)
    a, s, w = 0.5, 0.1, 2.0
    ref = _ref(V, ldl, T, a, s, w, D.WEIGHTS[T])
    good = D.xent_distill_f32(lg, te, V, lab, w, s, a, D.WEIGHTS[T])
    D.check(good, V, ref, lg, w, "unmutated")
    bad = D.xent_distill_f32(lg, te, V, lab, w, s, a, D.WEIGHTS[T], mutant=mutant)
    with pytest.raises(R.Mismatch):
        D.check(bad, V, ref, lg, w, mutant)


def test_alpha_zero_is_the_plain_cross_entropy():
    """The reference at alpha = 0 is ref_tail.ref_xent, whatever the teachers."""
    V, ldl, T = 250, 256, 2
    lg, lab, te = _case(V, ldl, T)
    ref = _ref(V, ldl, T, 0.0, 0.1, 2.0, D.WEIGHTS[T])
    loss, correct, ntok, d = R.ref_xent(lg[:, :V], lab, 2.0, 0.1)
    assert ntok == ref[3]
    assert torch.allclose(ref[0], loss, rtol=1e-12, atol=1e-12)
    assert torch.allclose(ref[1], loss, rtol=1e-12, atol=1e-12)
    assert torch.equal(ref[2], correct)
    assert torch.allclose(ref[4], d, rtol=1e-12, atol=1e-15)


def test_teacher_equal_to_student_has_zero_gradient():
    V, ldl = 250, 256
    lg, lab = R.xent_rows(V, ldl)
    ref = D.ref_xent_distill(lg[:, :V], [lg[:, :V]], lab, 1.0, 0.0, 1.0)
    assert float(ref[4].abs().max()) < 1e-15
