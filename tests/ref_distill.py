"""Float64 reference, float32 evaluation, mutants, cases and tolerances of the
word-level distillation loss (ops.kernels.xent_distill,
csrc/kernels/distill.hip). No GPU needed. The discipline is tests/ref_tail.py's:
the reference starts from exactly what the kernel gets (bf16 logits of the
student and the teachers, f32-rounded scalars, the f32 log of each normalised
weight) and evaluates in float64; `xent_distill_f32` is the plain float32
PyTorch evaluation, deliberately wrong in one line with `mutant=...`.
tests/test_distill_refs_cpu.py shows that the comparators accept the former
and reject every mutant, so tests/test_gpu_distill.py, which puts the HIP
kernel through the same comparators, cannot pass vacuously.

    p      = softmax(x[:V])                lse = logsumexp(x[:V])
    q      = sum_m w_m softmax(z_m[:V])
    target = (1 - alpha) ((1 - s) onehot(label) + s / V) + alpha q
    row_loss  = -sum_v target[v] log p[v]
    row_label = (1 - s)(lse - x_label) + s (lse - mean x)
    dlogits   = (p - target) / (max(ntok, 1) workers)
PAD rows (label 0): 0, 0, 0 and a zero gradient row.
"""
from __future__ import annotations

import math

import torch

import ref_tail as R
from ref_tail import BF16, F32, F64, PAD

# --------------------------------------------------------------------------- tolerances
# Same form as ref_tail.E32 (tol = ref_tail.MARGIN x E32): E32 is the worst
# ratio of xent_distill_f32 against ref_xent_distill over every case of
# tests/test_gpu_distill.py (CASES below), measured on the CPU by
# test_distill_refs_cpu.py::test_e32_table_is_measured; `kernel` is the worst
# ratio of the HIP kernel on the MI355X over the same cases, in the same unit.
#
#   entry                  E32        kernel     what
E32 = {
    "distill_row_loss":  8.9e-7,   # 3.3e-7   the objective per row; scale = |lse| + max|x_row|
    "distill_dlogits":   2.2e-6,   # 1.8e-7   error of the f32 gradient before its bf16 rounding, / scale
}
R.register(E32)


# --------------------------------------------------------------------------- reference
def norm_weights(T, weights=None):
    w = [1.0] * T if weights is None else [float(x) for x in weights]
    assert len(w) == T and all(x > 0 for x in w)
    tot = math.fsum(w)
    return [x / tot for x in w]


def ref_xent_distill(logits, teachers, labels, workers, smoothing, alpha, weights=None):
    """logits [M, V] and teachers (each [M, V]): the first V columns, bf16
    values. Returns (row_loss, row_label, row_correct, ntok, dlogits [M, V])
    in float64."""
    x = logits.to(F64)
    M, V = x.shape
    lab = labels.to(torch.int64)
    s, wk, al = R._f32r(smoothing), R._f32r(workers), R._f32r(alpha)
    # the kernel gets the f32 log of each normalised weight
    w = [math.exp(R._f32r(math.log(v))) for v in norm_weights(len(teachers), weights)]
    valid = lab != PAD
    ntok = float(valid.sum())
    logp = x - torch.logsumexp(x, -1, keepdim=True)
    onehot = torch.zeros_like(x).scatter_(1, lab.view(-1, 1), 1.0)
    hard = (1 - s) * onehot + s / V
    q = sum(wm * torch.softmax(t.to(F64), -1) for t, wm in zip(teachers, w))
    target = (1 - al) * hard + al * q
    loss = -(target * logp).sum(-1) * valid
    label_loss = -(hard * logp).sum(-1) * valid
    correct = ((R._first_argmax(x) == lab) & valid).to(F64)
    scale = 1.0 / (max(ntok, 1.0) * wk)
    d = (torch.exp(logp) - target) * scale * valid.view(-1, 1)
    return loss, label_loss, correct, ntok, d


DISTILL_MUTANTS = ("teacher_lse_over_ldt", "weights_not_normalised", "geometric_mean",
                   "alpha_skips_smoothing", "pad_teacher_unmasked", "row_label_is_objective",
                   "pad_cols_kept")


def xent_distill_f32(logits, teachers, V, labels, workers, smoothing, alpha, weights=None, mutant=None,
                     keep_f32=False):
    """The float32 PyTorch evaluation on the padded bf16 student [M, ldl] and
    teachers [M, ldt]. Returns (row_loss, row_label, row_correct, ntok,
    dlogits bf16 [M, ldl])."""
    assert mutant is None or mutant in DISTILL_MUTANTS
    full = logits.to(F32)
    x = full[:, :V]
    lab = labels.to(torch.int64)
    s = torch.tensor(smoothing, dtype=F32)
    wk = torch.tensor(workers, dtype=F32)
    al = torch.tensor(alpha, dtype=F32)
    T = len(teachers)
    raw = [1.0] * T if weights is None else [float(v) for v in weights]
    w = raw if mutant == "weights_not_normalised" else norm_weights(T, weights)
    valid = lab != PAD
    ntok = valid.sum().to(F32)
    logp = torch.log_softmax(x, -1)
    onehot = torch.zeros_like(x).scatter_(1, lab.view(-1, 1), 1.0)
    tz = [(t.to(F32) if mutant == "teacher_lse_over_ldt" else t[:, :V].to(F32)) for t in teachers]
    if mutant == "geometric_mean":
        q = torch.softmax(sum(wm * torch.log_softmax(z, -1) for z, wm in zip(tz, w)), -1)
    else:
        q = sum(wm * torch.softmax(z, -1)[:, :V] for z, wm in zip(tz, w))
    hard = (1 - s) * onehot + s / V
    if mutant == "alpha_skips_smoothing":
        target = (1 - al) * (1 - s) * onehot + s / V + al * q
    else:
        target = (1 - al) * hard + al * q
    rows = -(target * logp).sum(-1)
    label_loss = -(hard * logp).sum(-1) * valid
    scale = 1 / (ntok.clamp_min(1.0) * wk)
    d = (torch.exp(logp) - target) * scale
    if mutant == "pad_teacher_unmasked":  # the label part is masked, the teacher part is not
        v = valid.to(F32)
        loss = label_loss * (1 - al) + al * -(q * logp).sum(-1)
        d = ((torch.exp(logp) - hard) * v.view(-1, 1) * (1 - al) + al * (torch.exp(logp) - q)) * scale
    else:
        loss = rows * valid
        d = d * valid.view(-1, 1)
    if mutant == "row_label_is_objective":
        label_loss = loss
    out = full.clone() if mutant == "pad_cols_kept" else torch.zeros_like(full)
    out[:, :V] = d
    return loss, label_loss, ((R._first_argmax(x) == lab) & valid).to(F32), float(ntok), \
        (out if keep_f32 else out.to(BF16))


# --------------------------------------------------------------------------- comparators
def close_distill_dlogits(got, ref, V, scale, what):
    """ref_tail.close_dlogits under the `distill_dlogits` entry: bf16 dlogits
    [M, ldl] against the float64 [M, V] gradient, every element: |got - ref|
    <= 2^-8 |ref| + tol * scale; PAD rows and the columns [V, ldl) exactly 0."""
    if got.dtype != BF16:
        R._fail(what, f"dtype {got.dtype}")
    g = got.to(F64)
    if not bool(torch.isfinite(g).all()):
        R._fail(what, "non-finite gradient")
    if g.shape[1] > V and bool((g[:, V:] != 0).any()):
        R._fail(what, "padded columns [V, ldl) not zero")
    pad = ~(ref != 0).any(-1)
    if bool((g[pad] != 0).any()):
        R._fail(what, "PAD row gradient not zero")
    excess = ((g[:, :V] - ref).abs() - R.BF16_ULP * ref.abs()).clamp_min(0) / scale
    worst = float(excess.max())
    R._note("distill_dlogits", worst)
    if worst > R.tol("distill_dlogits"):
        i = int(excess.argmax())
        R._fail(what, f"[distill_dlogits] element ({i // V}, {i % V}): got {g[:, :V].flatten()[i].item()!r} "
                      f"ref {ref.flatten()[i].item()!r}, excess {worst:.3e} > "
                      f"{R.tol('distill_dlogits'):.3e} (x scale)")
    return worst


def check(out, V, ref, lg, workers, what):
    """out = (row_loss, row_label, row_correct, ntok, dlogits bf16 [M, ldl])
    against ref = ref_xent_distill(...)."""
    loss, label_loss, correct, ntok, d = ref
    assert out[3] == ntok, f"{what}: ntok {out[3]} vs {ntok}"
    sc = R.row_loss_scale(lg[:, :V])
    R.close_f32(out[0], loss, "distill_row_loss", what + " row_loss", scale=sc)
    R.close_f32(out[1], label_loss, "row_loss", what + " row_label", scale=sc)
    R.exact(out[2].to(F32), correct.to(F32), what + " row_correct")
    close_distill_dlogits(out[4], d, V, R.xent_scale(ntok, workers), what + " dlogits")


# --------------------------------------------------------------------------- cases
# (V, ldl, element offset of the student): the register arm at NCH 1..4 with
# both edges, the generic arm by row length, by stride and by alignment
SHAPES = [(5, 8, 0), (250, 256, 0), (2041, 2048, 0), (2049, 2056, 0), (5000, 5056, 0),
          (7010, 7040, 0), (8192, 8192, 0), (8193, 8200, 0), (33, 34, 0), (7010, 7040, 2)]
EIGHT_TEACHERS = [(250, 256, 0), (7010, 7040, 0)]
ALPHAS = (0.5, 1.0)
SMOOTHING = (0.0, 0.1)
WORKERS = (1.0, 2.0)
WEIGHTS = {1: None, 2: (1.0, 3.0), 3: (3.0, 1.0, 2.0), 8: None}  # non-uniform with 2 and 3 teachers
CASES = [(V, ldl, off, T) for V, ldl, off in SHAPES for T in (1, 2, 3)] + \
        [(V, ldl, off, 8) for V, ldl, off in EIGHT_TEACHERS]


def expected_arm(V, ldl, offset=0):
    """Every teacher stride of teacher_rows is a multiple of 8 when ldl is."""
    if ldl % 8 == 0 and ldl <= 8192 and offset % 8 == 0:
        return f"reg{-(-ldl // 2048)}"
    return "generic"


def teacher_ld(V, ldl, m):
    """Teacher m's row stride: V rounded up to 8 (even m), ldl + 64 (odd m)."""
    return (V + 7) // 8 * 8 if m % 2 == 0 else ldl + 64


def teacher_rows(V, ldl, T, seed=0):
    """The student of ref_tail.xent_rows(V, ldl) and T bf16 teachers [M,
    teacher_ld]. Row r of teacher m is of kind (r + m) % 5: N(0, 3^2); peaked
    (one logit 34 above N(0, 1)); +-80 (needs the max subtraction); N(0, 3^2)
    with its maximum away from the label; the student's own row. Columns
    [V, ldt) are poisoned: NaN in the even rows, 3e38 in the odd ones."""
    lg, lab = R.xent_rows(V, ldl)
    M = lg.shape[0]
    g = torch.Generator().manual_seed(7000 * V + 13 * ldl + T + seed)
    teachers = []
    for m in range(T):
        ldt = teacher_ld(V, ldl, m)
        z = torch.empty(M, ldt)
        for r in range(M):
            kind = (r + m) % 5
            if kind == 0:
                row = torch.randn(V, generator=g) * 3.0
            elif kind == 1:
                row = torch.randn(V, generator=g)
                row[int(torch.randint(0, V, (1,), generator=g))] = 34.0
            elif kind == 2:
                row = (torch.rand(V, generator=g) * 2 - 1) * 80
                row[V // 2], row[V // 3] = 80.0, -80.0
            elif kind == 3:
                row = torch.randn(V, generator=g) * 3.0
                row[(int(lab[r]) + 1 + int(torch.randint(0, V - 1, (1,), generator=g))) % V] = R.TIE
            else:
                row = lg[r, :V].float()
            z[r, :V] = row
        z[0::2, V:] = float("nan")
        z[1::2, V:] = 3e38
        teachers.append(z.to(BF16))
    return lg, lab, teachers
