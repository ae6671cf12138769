"""Float64 reference, cases and tolerances of the R-Drop paired-row loss
(ops.kernels.loss.xent_rdrop, csrc/kernels/rdrop.hip), in the discipline of
tests/ref_tail.py: from the bf16 logits and f32-rounded scalars, in float64.
The float32 evaluation is ops.kernels.loss.rdrop_rows (xent_rdrop's CPU arm).

Logits row i (copy 1) and row i + M (copy 2) form a pair with the label y;
xa, xb its logits over the first V columns, p = softmax(xa), r = softmax(xb),
s the smoothing, ntok the label count of both copies:
    row_label[a] = (1 - s)(lse_a - xa[y]) + s (lse_a - mean xa)        (same for b)
    d[v]         = (xa[v] - lse_a) - (xb[v] - lse_b)
    KLab = sum_v p[v] d[v]          KLba = -sum_v r[v] d[v]
    row_loss[a]  = row_label[a] + (alpha / 2) KLab,  row_loss[b] = row_label[b] + (alpha / 2) KLba
    row_correct  = first-index argmax of the row == y
    dlogits[a] = (p - target + (alpha / 2)(p (d - KLab) + p - r)) / (max(ntok, 1) workers)
    dlogits[b] = (r - target + (alpha / 2)(r (-d - KLba) + r - p)) / (max(ntok, 1) workers)
    target     = (1 - s) onehot(y) + s / V
PAD pairs (label 0): 0 everywhere and two zero gradient rows.
"""
import torch

import ref_tail as R
from ref_tail import BF16, F32, F64, PAD

# Same form as ref_tail.E32 (tol = ref_tail.MARGIN x E32): E32 is the worst
# ratio of the f32 evaluation against ref_rdrop over exactly the cases of
# tests/test_gpu_rdrop.py (SHAPES x ALPHAS x SMOOTHING x WORKERS), measured on
# the CPU; `kernel` the HIP kernel's on the MI355X over the same cases. With
# S = |lse| + max|x| of a row (ref_tail.row_loss_scale), d being a difference
# of two such differences, both scales grow with alpha:
#   row_loss scale = S_own + (alpha / 2)(S_a + S_b)
#   gradient scale = (1 + (alpha / 2)(S_a + S_b)) / (max(ntok, 1) workers)
#   entry                E32        kernel     what
E32 = {
    "rdrop_row_loss":  3.5e-7,   # 8.1e-8   the objective per row: |got - ref| <= tol (|ref| + row_loss scale)
    "rdrop_dlogits":   4.5e-7,   # 5.2e-9   ref_tail.close_dlogits' form: 2^-8 |ref| + tol x gradient scale
}
R.register(E32)

# (V, ldl, element offset): every NCH of the register arm, the first shape
# beyond it, the odd-stride and the misaligned generic arm
SHAPES = [(5, 8, 0), (250, 256, 0), (2049, 2056, 0), (7010, 7040, 0), (8192, 8192, 0), (8193, 8200, 0),
          (33, 34, 0), (7010, 7040, 2)]
ALPHAS, SMOOTHING, WORKERS = (1.0, 5.0), (0.0, 0.1), (1.0, 2.0)


def pair_rows(V, ldl):
    """bf16 [2 M, ldl], int64 labels [2 M]: copy 1 is ref_tail.xent_rows (PAD
    rows, poisoned padding); row r of copy 2 is of kind r % 4: + N(0, 0.1^2)
    noise; the same bits; peaked 34 above N(0, 1) on another column than copy
    1's maximum (large KL); +-80 (needs the max subtraction)."""
    lg, lab = R.xent_rows(V, ldl)
    g = torch.Generator().manual_seed(9000 * V + 17 * ldl)
    z = lg.clone().float()
    for r in range(lg.shape[0]):
        if r % 4 == 0:
            z[r, :V] += torch.randn(V, generator=g) * 0.1
        elif r % 4 == 2:
            z[r, :V] = torch.randn(V, generator=g)
            z[r, (int(lg[r, :V].float().argmax()) + 1 + int(torch.randint(0, max(V - 1, 1), (1,), generator=g))) % V] = 34.0
        elif r % 4 == 3:
            z[r, :V] = (torch.rand(V, generator=g) * 2 - 1) * 80
            z[r, V // 2], z[r, V // 3] = 80.0, -80.0
    return torch.cat([lg, z.to(BF16)]), torch.cat([lab, lab])


def ref_rdrop(logits2, labels, workers, smoothing, alpha):
    """logits2 [2 M, V] (bf16 values), labels [2 M]. Returns (row_loss,
    row_label, row_correct, ntok, dlogits [2 M, V]) in float64."""
    x = logits2.to(F64)
    M, V = x.shape[0] // 2, x.shape[1]
    lab = labels[:M].to(torch.int64)
    s, wk, h = R._f32r(smoothing), R._f32r(workers), 0.5 * R._f32r(alpha)
    valid = (lab != PAD).to(F64)
    ntok = 2.0 * float(valid.sum())
    la, lb = (t - torch.logsumexp(t, -1, keepdim=True) for t in (x[:M], x[M:]))
    p, r, d = la.exp(), lb.exp(), la - lb
    kl = torch.cat([(p * d).sum(-1), -(r * d).sum(-1)]) * valid.repeat(2)
    hard = (1 - s) * torch.zeros_like(la).scatter_(1, lab.view(-1, 1), 1.0) + s / V
    label = torch.cat([-(hard * la).sum(-1), -(hard * lb).sum(-1)]) * valid.repeat(2)
    correct = ((R._first_argmax(x) == lab.repeat(2)).to(F64)) * valid.repeat(2)
    sc = (valid / (max(ntok, 1.0) * wk)).view(-1, 1)
    da = (p - hard + h * (p * (d - kl[:M].view(-1, 1)) + p - r)) * sc
    db = (r - hard + h * (r * (-d - kl[M:].view(-1, 1)) + r - p)) * sc
    return label + h * kl, label, correct, ntok, torch.cat([da, db])


def check(out, V, ref, lg2, alpha, workers, what):
    """out = (row_loss, row_label, row_correct, ntok, dlogits bf16 [2 M, ldl]
    or f32 [2 M, V]) against ref = ref_rdrop(...)."""
    loss, label, correct, ntok, d = ref
    assert out[3] == ntok, f"{what}: ntok {out[3]} vs {ntok}"
    S = R.row_loss_scale(lg2[:, :V])
    both = 0.5 * R._f32r(alpha) * (S[:S.shape[0] // 2] + S[S.shape[0] // 2:]).repeat(2)
    R.close_f32(out[0], loss, "rdrop_row_loss", what + " row_loss", scale=S + both)
    R.close_f32(out[1], label, "row_loss", what + " row_label", scale=S)
    R.exact(out[2].to(F32), correct.to(F32), what + " row_correct")
    g = out[4].to(F64)
    assert bool(torch.isfinite(g).all()), f"{what}: non-finite gradient"
    assert not bool((g[:, V:] != 0).any()), f"{what}: padded columns [V, ldl) not zero"
    assert not bool((g[~(d != 0).any(-1)] != 0).any()), f"{what}: PAD row gradient not zero"
    ulp = R.BF16_ULP if out[4].dtype == BF16 else 0.0
    excess = ((g[:, :V] - d).abs() - ulp * d.abs()).clamp_min(0) / ((1.0 + both) * R.xent_scale(ntok, workers)).view(-1, 1)
    R._note("rdrop_dlogits", float(excess.max()))
    assert float(excess.max()) <= R.tol("rdrop_dlogits"), \
        f"{what}: [rdrop_dlogits] excess {float(excess.max()):.3e} > {R.tol('rdrop_dlogits'):.3e} at {int(excess.argmax())}"
