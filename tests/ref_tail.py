"""Float64 references, comparators, case builders and mutants for the tail of
the training step: the fused cross-entropy (csrc/kernels/xent.hip), its
statistics and token count, Adam with the Noam schedule
(csrc/kernels/adam.hip) and the f32 -> bf16 shadow conversion. No GPU needed;
every function works on whatever device its inputs live on.

The references start from exactly what the kernels get (bf16-rounded logits,
f32 buffers, f32-rounded hyperparameters) and evaluate in float64. The
`*_f32` functions are the straightforward float32 PyTorch evaluation of the
same formulas; with `mutant=...` they are deliberately wrong in one line.
tests/test_loss_optim_refs_cpu.py shows that the comparators accept the
former and reject every mutant, so tests/test_gpu_loss_optim.py, which puts the
HIP kernels through the same comparators, cannot pass vacuously.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16

# --------------------------------------------------------------------------- tolerances
# Every f32 output is compared elementwise as
#     |got - ref| <= tol * (|ref| + scale),     tol = 8 * E32,
# that is rtol = tol and atol = tol * scale, with `scale` the magnitude of the
# operands the value is formed from (given at each comparator below), so that
# a value which is a small difference of large operands is not held to a
# relative error its inputs cannot give.
#
# E32 is the worst such ratio of the float32 PyTorch evaluation (`*_f32`
# below) against the float64 reference over all cases of
# tests/test_gpu_loss_optim.py, measured on the CPU by
# test_loss_optim_refs_cpu.py::test_e32_table_is_measured. The margin of 8 is
# for the kernels' __expf / __logf / rsqrtf / powf (a few ulp where libm is
# at most 1) and their other summation order. `kernel` is the worst ratio of
# the HIP kernels on the MI355X over the same cases, in the same unit (0: the
# whole error of the weights lay within close_p's ulp term).
#
#   entry             E32        kernel     what
E32 = {
    "row_loss":     6.7e-8,   # 6.7e-8   per-row loss; scale = |lse| + max|x_row|
    "stats_loss":   1.1e-7,   # 1.1e-7   xent_stats loss; scale = 0 (a sum of non-negatives)
    "dlogits":      2.2e-6,   # 8.4e-7   atol_g: error of the f32 gradient before its bf16 rounding, / scale
    "noam":         1.1e-7,   # (host)   train/schedule.noam_lr; scale = 0
    "adam_m":       6.6e-8,   # 5.8e-8   first moment; scale = (1 - b1) (|m_old| + |g * grad_scale|)
    "adam_v":       5.8e-8,   # 6.0e-8   second moment; scale = (1 - b2) (v_old + (g * grad_scale)^2)
    "adam_dp":      4.1e-7,   # 3.8e-7   one step's weight update; see close_p / dp_ratio
    "adam_m_traj":  6.2e-8,   # 7.1e-8   first moment during 20 steps from zero; scale: ref_trajectory
    "adam_v_traj":  3.2e-8,   # 2.5e-8   second moment during the same steps
    "adam_dp_traj": 1.6e-7,   # 0        the 20 steps' accumulated update; see close_p / dp_ratio
}
MARGIN = 8.0
BF16_ULP = 2.0 ** -8  # one bf16 ulp (8 significand bits): twice the round-to-nearest bound


# tables of the same form and discipline kept by other modules (tests/ref_norm.py)
EXTRA: dict = {}


def register(table: dict) -> None:
    """Add another module's measured entries; none may shadow an entry above."""
    assert not set(table) & set(E32), sorted(set(table) & set(E32))
    EXTRA.update(table)


def tol(key: str) -> float:
    return MARGIN * (E32[key] if key in E32 else EXTRA[key])


# worst observed ratio err / (|ref| + scale) per entry since import (the unit of E32)
WORST: dict = {}


def _note(key: str, ratio: float) -> None:
    WORST[key] = max(WORST.get(key, 0.0), ratio)


def report() -> str:
    return "  ".join(f"{k}={v:.2e}/{tol(k):.2e}" for k, v in sorted(WORST.items()))


class Mismatch(AssertionError):
    pass


def _fail(what, msg):
    raise Mismatch(f"{what}: {msg}")


def ulp32(x: torch.Tensor) -> torch.Tensor:
    """Spacing of float32 at |x| (float64 tensor)."""
    a = x.to(F32).abs()
    return (torch.nextafter(a, torch.full_like(a, math.inf)) - a).to(F64)


def close_f32(got, ref, key, what, scale=0.0):
    """Elementwise |got - ref| <= tol(key) * (|ref| + scale); returns the worst ratio."""
    got, ref = got.to(F64), ref.to(F64)
    if got.shape != ref.shape:
        _fail(what, f"shape {tuple(got.shape)} vs {tuple(ref.shape)}")
    if not bool(torch.isfinite(got).all()):
        _fail(what, "non-finite values")
    den = ref.abs() + scale
    err = (got - ref).abs()
    ratio = torch.where(err > 0, err / den.clamp_min(1e-300), torch.zeros_like(err))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    _note(key, worst)
    if worst > tol(key):
        i = int(ratio.argmax())
        _fail(what, f"[{key}] ratio {worst:.3e} > {tol(key):.3e} at {i}: got {got.flatten()[i].item()!r} "
                    f"ref {ref.flatten()[i].item()!r}")
    return worst


def _p_ulps(p_old, dp_ref, steps):
    return steps * torch.maximum(ulp32(p_old), ulp32(p_old - dp_ref))


def dp_ratio(dp_got, p_old, dp_ref, steps=1):
    """Worst |dp_got - dp_ref| / (|dp_ref| + steps * ulp32(p)) of an update
    that is known by itself: the unit of E32["adam_dp*"]."""
    p_old, dp_ref = p_old.to(F64), dp_ref.to(F64)
    return float(((dp_got.to(F64) - dp_ref).abs() / (dp_ref.abs() + _p_ulps(p_old, dp_ref, steps))).max())


def close_p(got_p, p_old, dp_ref, what, key="adam_dp", steps=1):
    """The weight, measured against the update and not the weight:
    |got - (p_old - dp_ref)| <= tol * |dp_ref| + steps * ulp32(p). Each step
    rounds the stored weight once (<= ulp / 2), so `steps` ulp is twice the
    bound of what the f32 store alone adds. E32 of these entries is
    dp_ratio() of the f32 evaluation's update; what is recorded of a weight
    is the part of its error that the ulp term does not cover, in that unit."""
    got, p_old, dp_ref = got_p.to(F64), p_old.to(F64), dp_ref.to(F64)
    if not bool(torch.isfinite(got).all()):
        _fail(what, "non-finite weights")
    u = _p_ulps(p_old, dp_ref, steps)
    err = (got - (p_old - dp_ref)).abs()
    ratio = float(((err - u).clamp_min(0) / (dp_ref.abs() + u)).max())
    _note(key, ratio)
    over = err - tol(key) * dp_ref.abs() - u
    if bool((over > 0).any()):
        i = int(over.argmax())
        _fail(what, f"[{key}] weight {i}: err {err.flatten()[i].item():.3e}, update "
                    f"{dp_ref.flatten()[i].item():.3e}, ulp {u.flatten()[i].item():.3e}")
    return ratio


def close_dlogits(got, ref, V, scale, what):
    """bf16 dlogits [M, ldl] against the float64 [M, V] gradient, every
    element: |got - ref| <= 2^-8 |ref| + atol_g * scale; rows whose reference
    is all zero (PAD rows) and the columns [V, ldl) exactly +-0."""
    if got.dtype != BF16:
        _fail(what, f"dtype {got.dtype}")
    g = got.to(F64)
    if not bool(torch.isfinite(g).all()):
        _fail(what, "non-finite gradient")
    if g.shape[1] > V and bool((g[:, V:] != 0).any()):
        _fail(what, "padded columns [V, ldl) not zero")
    pad = ~(ref != 0).any(-1)
    if bool((g[pad] != 0).any()):
        _fail(what, "PAD row gradient not zero")
    err = (g[:, :V] - ref).abs()
    excess = (err - BF16_ULP * ref.abs()).clamp_min(0) / scale
    worst = float(excess.max())
    _note("dlogits", worst)
    if worst > tol("dlogits"):
        i = int(excess.argmax())
        _fail(what, f"[dlogits] element ({i // V}, {i % V}): got {g[:, :V].flatten()[i].item()!r} "
                    f"ref {ref.flatten()[i].item()!r}, excess {worst:.3e} > {tol('dlogits'):.3e} (x scale)")
    return worst


def exact(got, ref, what):
    """Same shape, same dtype, and bitwise the same values (floats by their bit
    patterns: NaN equals the same NaN, +0 differs from -0)."""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    if got.shape != ref.shape or got.dtype != ref.dtype:
        _fail(what, f"{got.dtype}{tuple(got.shape)} vs {ref.dtype}{tuple(ref.shape)}")
    if got.is_floating_point():
        it = {2: torch.int16, 4: torch.int32, 8: torch.int64}[got.element_size()]
        same = got.contiguous().view(it) == ref.contiguous().view(it)
    else:
        same = got == ref
    if not bool(same.all()):
        i = int((~same).flatten().nonzero()[0])
        _fail(what, f"{int((~same).sum())} elements differ, first at {i}: "
                    f"{got.flatten()[i].item()!r} vs {ref.flatten()[i].item()!r}")


def close_accuracy(got: float, correct: float, ntok: float, what):
    """accuracy == float32(correct) / float32(max(ntok, 1)) to 1 ulp."""
    want = torch.tensor(correct, dtype=F32) / torch.tensor(max(ntok, 1.0), dtype=F32)
    u = float(ulp32(want.to(F64)))
    if not abs(got - float(want)) <= u:
        _fail(what, f"accuracy {got!r} vs {float(want)!r}")


# --------------------------------------------------------------------------- cross-entropy
PAD = 0


def _f32r(x: float) -> float:
    """The float32 the kernels receive for a Python float argument."""
    return float(torch.tensor(x, dtype=F32))


def _first_argmax(x, last=False):
    V = x.shape[-1]
    idx = torch.arange(V, device=x.device).expand_as(x)
    hit = x == x.max(-1, keepdim=True).values
    if last:
        return torch.where(hit, idx, torch.full_like(idx, -1)).max(-1).values
    return torch.where(hit, idx, torch.full_like(idx, V)).min(-1).values


def ref_xent(logits, labels, workers, smoothing):
    """logits [M, V] (the first V columns, bf16 values), labels [M]. Returns
    (row_loss [M], row_correct [M], ntok, dlogits [M, V]) in float64:
    loss = (1 - s) * (lse - x_label) + s * (lse - mean x); dlogits =
    (softmax - s / V - (1 - s) * onehot) / (max(ntok, 1) * workers); PAD rows
    give 0, 0 and a zero gradient row; correct = first-index argmax == label."""
    x = logits.to(F64)
    M, V = x.shape
    lab = labels.to(torch.int64)
    s, w = _f32r(smoothing), _f32r(workers)
    valid = lab != PAD
    ntok = float(valid.sum())
    lse = torch.logsumexp(x, -1)
    xl = x.gather(1, lab.view(-1, 1)).squeeze(1)
    loss = ((1 - s) * (lse - xl) + s * (lse - x.sum(-1) / V)) * valid
    correct = ((_first_argmax(x) == lab) & valid).to(F64)
    scale = 1.0 / (max(ntok, 1.0) * w)
    onehot = torch.zeros_like(x).scatter_(1, lab.view(-1, 1), 1.0)
    d = (torch.exp(x - lse.view(-1, 1)) - s / V - (1 - s) * onehot) * scale * valid.view(-1, 1)
    return loss, correct, ntok, d


def xent_scale(ntok, workers):
    return 1.0 / (max(ntok, 1.0) * _f32r(workers))


def row_loss_scale(logits_v):
    """|lse| + max|x| per row: what a row's loss is a difference of."""
    x = logits_v.to(F64)
    return torch.logsumexp(x, -1).abs() + x.abs().max(-1).values


XENT_MUTANTS = ("lse_over_ldl", "no_smoothing_offset", "smoothing_mean_over_ldl", "last_argmax",
                "no_workers", "pad_row_grad", "pad_cols_kept")


def xent_f32(logits, V, labels, workers, smoothing, mutant=None, keep_f32=False):
    """The float32 PyTorch evaluation on the padded bf16 logits [M, ldl].
    Returns (row_loss, row_correct, ntok, dlogits bf16 [M, ldl])."""
    assert mutant is None or mutant in XENT_MUTANTS
    ldl = logits.shape[1]
    full = logits.to(F32)
    x = full[:, :V]
    lab = labels.to(torch.int64)
    s = torch.tensor(smoothing, dtype=F32)
    w = torch.tensor(workers, dtype=F32)
    valid = lab != PAD
    ntok = valid.sum().to(F32)
    lse = torch.logsumexp(full if mutant == "lse_over_ldl" else x, -1)
    xl = x.gather(1, lab.view(-1, 1)).squeeze(1)
    nmean = ldl if mutant == "smoothing_mean_over_ldl" else V
    loss = ((1 - s) * (lse - xl) + s * (lse - x.sum(-1) / nmean)) * valid
    correct = ((_first_argmax(x, last=mutant == "last_argmax") == lab) & valid).to(F32)
    scale = 1 / (ntok.clamp_min(1.0) * (1.0 if mutant == "no_workers" else w))
    off = 0.0 if mutant == "no_smoothing_offset" else s / nmean
    onehot = torch.zeros_like(x).scatter_(1, lab.view(-1, 1), 1.0)
    d = (torch.exp(x - lse.view(-1, 1)) - off - (1 - s) * onehot) * scale
    if mutant != "pad_row_grad":
        d = d * valid.view(-1, 1)
    out = full.clone() if mutant == "pad_cols_kept" else torch.zeros_like(full)
    out[:, :V] = d
    if keep_f32:
        return loss, correct, float(ntok), out
    return loss, correct, float(ntok), out.to(BF16)


# (V, ldl): every dispatch arm of tdg_xent. The register kernel
# xent_reg_kernel<NCH>, NCH = ceil(ldl / 2048), runs when ldl % 8 == 0, the
# base is 16-byte aligned and ldl <= 8192; the two-pass xent_kernel otherwise.
XENT_SHAPES = [
    (5, 8), (250, 256), (2041, 2048),             # NCH 1 and its upper edge
    (2049, 2056), (4096, 4096),                   # NCH 2 at both edges, V == ldl
    (5000, 5056),                                 # NCH 3
    (6145, 6152), (7010, 7040), (8192, 8192),     # NCH 4
    (8193, 8200),                                 # generic: just past the limit
    (33, 34), (1001, 1002),                       # generic: ldl % 8 != 0, odd V, one / several iterations
    (32000, 32000),                               # generic: a realistic vocabulary (16 rows)
]
XENT_SMOOTHING = (0.0, 0.1)
XENT_WORKERS = (1.0, 2.0)
XENT_BOTH_LABEL_DTYPES = [(250, 256), (7010, 7040), (8193, 8200)]
TIE = 20.0  # above every N(0, 3^2) draw of these sizes; exact in bf16


def xent_expected_arm(V, ldl):
    if ldl % 8 == 0 and ldl <= 8192:
        return f"reg{-(-ldl // 2048)}"
    return "generic"


def xent_rows(V, ldl, M=40, seed=0):
    """About M rows of bf16 logits [M, ldl] and int64 labels [M] for a
    vocabulary of V: random N(0, 3^2) rows with about 1 in 7 PAD, then the
    special rows that fit V. Columns [V, ldl) are poisoned: NaN in the even
    rows, 3e38 in the odd ones."""
    g = torch.Generator().manual_seed(1000 * V + ldl + seed)
    rows, labs = [], []

    def rnd(std=3.0):
        return torch.randn(V, generator=g) * std

    def lab():
        return int(torch.randint(1, V, (1,), generator=g))

    def add(x, l):
        rows.append(x)
        labs.append(l)

    # ties of the maximum at (a, b): in one thread's pair / 16-byte chunk; in
    # the same thread's next iteration (generic: c + 512, register: c + 2048);
    # in different waves (generic: 128 columns per wave, register: 512); at V - 1
    # ((10, 522) is also two waves of the register kernel, (12, 700) of both)
    pairs = [(2, 3), (10, 10 + 512), (10, 10 + 2048), (12, 700), (1, V - 1)]
    for a, b in pairs:
        if not (0 < a < b < V):
            continue
        for l in (a, b):  # label on the first tie: correct, on the last: not
            x = rnd()
            x[a] = x[b] = TIE
            add(x, l)
    x = rnd()  # maximum and label in the last column
    x[V - 1] = TIE
    add(x, V - 1)
    x = (torch.rand(V, generator=g) * 2 - 1) * 80  # needs the max subtraction
    x[V // 2], x[V // 3] = 80.0, -80.0
    add(x, lab())
    x = rnd(1.0)  # label logit 30 above the rest: loss ~ 0
    l = lab()
    x[l] = 34.0
    add(x, l)
    add(torch.full((V,), 1.5), lab())  # constant: argmax is column 0
    while len(rows) < M:
        add(rnd(), PAD if len(rows) % 6 == 2 else lab())  # (14 special rows at most: row 14 is PAD)
    order = torch.randperm(len(rows), generator=g).tolist()
    lg = torch.empty(len(rows), ldl)
    lg[:, :V] = torch.stack([rows[i] for i in order])
    lg[0::2, V:] = float("nan")
    lg[1::2, V:] = 3e38
    return lg.to(BF16), torch.tensor([labs[i] for i in order], dtype=torch.int64)


def ref_xent_stats(row_loss, row_correct, ntok, workers):
    """(loss, accuracy, correct) of xent_stats in float64 from the f32 rows."""
    n = max(float(ntok), 1.0)
    correct = float(row_correct.to(F64).sum())
    return float(row_loss.to(F64).sum()) / n / _f32r(workers), correct / n, correct


def xent_stats_f32(row_loss, row_correct, ntok, workers):
    n = torch.tensor(max(float(ntok), 1.0), dtype=F32)
    return (float(row_loss.to(F32).sum() / n / torch.tensor(workers, dtype=F32)),
            float(row_correct.to(F32).sum() / n))


def stats_rows(M, seed=0):
    """Row losses and 0/1 correct flags as xent writes them (PAD rows 0, 0)."""
    g = torch.Generator().manual_seed(77 * M + seed)
    valid = torch.rand(M, generator=g) > 1 / 7
    rl = (torch.rand(M, generator=g) * 9 + 0.01) * valid
    rc = (torch.rand(M, generator=g) < 0.4).to(F32) * valid
    return rl.to(F32), rc, float(valid.sum())


STATS_M = (1, 3, 257, 4096, 4099, 4100, 8196)
COUNT_M = (1, 255, 256, 257, 100000)


# --------------------------------------------------------------------------- Adam
@dataclass(frozen=True)
class AdamCfg:
    beta1: float = 0.9
    beta2: float = 0.98
    eps: float = 1e-9
    lr_const: float = 0.0
    d_model: float = 128.0
    warmup: float = 4000.0
    grad_scale: float = 1.0
    weight_decay: float = 0.0
    sched: int = 1

    def args(self):
        """Positional arguments of kernels.adam / adam_chunks after `step`."""
        return (self.beta1, self.beta2, self.eps, self.lr_const, self.d_model, self.warmup,
                self.grad_scale, self.weight_decay, self.sched)


def ref_noam(step, d_model, warmup):
    """d^-0.5 * min(step * warmup^-1.5, step^-0.5) in float64 (0 at step 0)."""
    step, d, w = float(step), _f32r(d_model), _f32r(warmup)
    fall = math.inf if step <= 0 else step ** -0.5
    return d ** -0.5 * min(step * w ** -1.5, fall)


def ref_adam_step(p, g, m, v, iterations, cfg: AdamCfg):
    """One Keras-semantics step in float64 (header of adam.hip): lr =
    noam(iterations) before the increment, t = iterations + 1, decoupled
    lr * wd * p, g * grad_scale in both moments. Returns (p, m, v, dp)."""
    p, g, m, v = (x.to(F64) for x in (p, g, m, v))
    b1, b2, eps = _f32r(cfg.beta1), _f32r(cfg.beta2), _f32r(cfg.eps)
    gs, wd = _f32r(cfg.grad_scale), _f32r(cfg.weight_decay)
    lr = ref_noam(iterations, cfg.d_model, cfg.warmup) if cfg.sched else _f32r(cfg.lr_const)
    t = iterations + 1
    lr_t = lr * math.sqrt(1 - b2 ** t) / (1 - b1 ** t)
    gk = g * gs
    m = m + (gk - m) * (1 - b1)
    v = v + (gk * gk - v) * (1 - b2)
    dp = lr_t * m / (v.sqrt() + eps) + lr * wd * p
    return p - dp, m, v, dp


ADAM_MUTANTS = ("p_untouched", "sign_flipped", "lr_for_lr_t", "t_is_iterations", "sched_at_next",
                "eps_in_sqrt", "no_scale_in_v", "wd_by_lr_t", "fall_is_rise")


def noam_f32(step, cfg: AdamCfg, mutant=None):
    T = lambda x: torch.tensor(x, dtype=F32)
    if not cfg.sched:
        return T(cfg.lr_const)
    s = T(float(step))
    rise = s * T(cfg.warmup) ** T(-1.5)
    fall = torch.rsqrt(s) if step > 0 else T(math.inf)
    if mutant == "fall_is_rise":
        fall = rise
    return torch.rsqrt(T(cfg.d_model)) * torch.minimum(rise, fall)


def adam_f32(p, g, m, v, iterations, cfg: AdamCfg, mutant=None):
    """The float32 PyTorch evaluation. Returns (p, m, v, dp)."""
    assert mutant is None or mutant in ADAM_MUTANTS
    T = lambda x: torch.tensor(x, dtype=F32, device=p.device)
    b1, b2 = T(cfg.beta1), T(cfg.beta2)
    lr = noam_f32(iterations + (1 if mutant == "sched_at_next" else 0), cfg, mutant).to(p.device)
    t = T(float(iterations if mutant == "t_is_iterations" else iterations + 1))
    lr_t = lr * torch.sqrt(1 - b2 ** t) / (1 - b1 ** t)
    if mutant == "lr_for_lr_t":
        lr_t = lr
    gk = g * T(cfg.grad_scale)
    m = m + (gk - m) * (1 - b1)
    gv = g if mutant == "no_scale_in_v" else gk
    v = v + (gv * gv - v) * (1 - b2)
    den = torch.sqrt(v + T(cfg.eps)) if mutant == "eps_in_sqrt" else torch.sqrt(v) + T(cfg.eps)
    dp = lr_t * m / den + (lr_t if mutant == "wd_by_lr_t" else lr) * T(cfg.weight_decay) * p
    if mutant == "p_untouched":
        return p.clone(), m, v, dp
    if mutant == "sign_flipped":
        return p + dp, m, v, dp
    return p - dp, m, v, dp


def adam_inputs(n, seed=0, zero_moments=False, device="cpu"):
    """p = 0.05 * randn as real weights are (ulp32(p) << |dp|); gradients
    and moments of magnitudes 1e-6 .. 1 elementwise, so that eps = 1e-9 matters
    in some denominators and not in others. The incoming first moment has
    the gradient's sign: m + (g - m) * (1 - b1) then does not cancel, the
    update keeps the relative accuracy of its operands, and the comparison
    against |dp| stays sharp (a cancelled moment would put E32 at 1e-4)."""
    g_ = torch.Generator(device=device).manual_seed(4242 + 7 * n + seed)
    R = lambda: torch.randn(n, generator=g_, device=device)
    p = 0.05 * R()
    mag = 10.0 ** (-6 * torch.rand(n, generator=g_, device=device))
    g = R() * mag
    if zero_moments:
        return p, g, torch.zeros(n, device=device), torch.zeros(n, device=device)
    m = 0.3 * R().abs() * mag * torch.sign(g)
    v = (0.5 + torch.rand(n, generator=g_, device=device)) * mag * mag
    return p, g, m, v


def fresh_grad(n, k, seed=0):
    """Gradient of step k: a fresh magnitude every step, around a size
    (1e-6 .. 1) and with a sign that each element keeps, so that neither the
    moments nor the accumulated update cancel (see adam_inputs)."""
    g0 = torch.Generator().manual_seed(4243 + n + seed)
    base = torch.sign(torch.randn(n, generator=g0)) * 10.0 ** (-6 * torch.rand(n, generator=g0))
    g_ = torch.Generator().manual_seed(99991 * (k + 1) + n + seed)
    return base * (0.1 + torch.randn(n, generator=g_).abs())


def check_adam(got, p, g, m, v, iterations, cfg, what, key="adam_dp"):
    """got = (p, m, v) after one step from (p, g, m, v): p through the update, m, v."""
    pr, mr, vr, dp = ref_adam_step(p, g, m, v, iterations, cfg)
    gk = g.to(F64) * _f32r(cfg.grad_scale)
    if cfg.sched and iterations == 0:  # Keras' first step: lr = 0, the weights do not move
        exact(got[0], p, what + " p at lr = 0")
    close_p(got[0], p, dp, what + " p", key)
    # a moment is x + (y - x) * (1 - b): the rounding of the bracket reaches it times (1 - b)
    ob1, ob2 = 1 - _f32r(cfg.beta1), 1 - _f32r(cfg.beta2)
    close_f32(got[1], mr, "adam_m", what + " m", scale=ob1 * (m.to(F64).abs() + gk.abs()))
    close_f32(got[2], vr, "adam_v", what + " v", scale=ob2 * (v.to(F64) + gk * gk))
    return pr, mr, vr, dp


ADAM_ITERATIONS = (0, 1, 10, 3999, 4000, 4001, 100000)
ADAM_SCHEDULES = ((128.0, 4000.0), (512.0, 100.0))
ADAM_OPTIONS = {
    "weight_decay": (AdamCfg(weight_decay=0.01, sched=0, lr_const=1e-2), 10),
    "grad_scale": (AdamCfg(grad_scale=0.5), 10),
}
TRAJ_START, TRAJ_STEPS = 3990, 20
ADAM_CAPPED_N = 4 * (2 * 8192 * 256 + 1001)  # 16 781 220: the paired loop, then the odd tail


def ref_trajectory(p, cfg, n, steps=TRAJ_STEPS, start=TRAJ_START):
    """Float64 Adam from zero moments over fresh gradients: yields per step
    (k, g_k, gmax, p, m, v), gmax = max_j<=k |g_j| elementwise. A moment
    inherits the rounding errors of every earlier step, which are relative
    to the operands of those steps, so gmax (and gmax^2 for v) is the scale
    its error is measured in."""
    pr = p.to(F64)
    mr = torch.zeros(n, dtype=F64)
    vr = torch.zeros(n, dtype=F64)
    gmax = torch.zeros(n, dtype=F64)
    for k in range(steps):
        g = fresh_grad(n, k)
        gmax = torch.maximum(gmax, g.to(F64).abs() * _f32r(cfg.grad_scale))
        pr, mr, vr, _ = ref_adam_step(pr, g, mr, vr, start + k, cfg)
        yield k, g, gmax, pr, mr, vr


def chunk_rows(start, end):
    """As train/optim.Adam._chunk_table builds them: (start, n, slot -1, no e4m3 copy)."""
    return [(c0, min(4096, end - c0), -1, 0) for c0 in range(start, end, 4096)]


# --------------------------------------------------------------------------- to_bf16
TO_BF16_N = (1, 255, 4099, 2097157)


def to_bf16_inputs(n, seed=0):
    """f32 values with exact round-to-even ties in both directions, +-0, +-inf
    and the largest finite f32 among random ones."""
    g = torch.Generator().manual_seed(31 * n + seed)
    x = torch.randn(n, generator=g) * 10.0 ** (8 * torch.rand(n, generator=g) - 4)
    bits = [0x3F808000, 0x3F818000,  # 1 + 2^-8: tie, rounds down to even; 1 + 3 * 2^-8: tie, rounds up
            0xBF808000, 0xBF818000, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000,
            0x7F7FFFFF, 0xFF7FFFFF,  # largest finite: rounds to inf
            0x3F807FFF, 0x3F808001]  # one f32 ulp either side of a tie
    sp = torch.tensor([b - (1 << 32) if b >> 31 else b for b in bits], dtype=torch.int32).view(F32)
    k = min(n, len(bits))
    idx = torch.randperm(n, generator=g)[:k]
    x[idx] = sp[:k]
    return x
