"""The references, comparators and cases of tests/ref_tail.py, without a GPU:
the float32 PyTorch evaluation of cross-entropy and Adam passes every case
that tests/test_gpu_loss_optim.py puts the HIP kernels through, every mutant
is rejected, the float64 Adam reference is torch.optim.Adam, and the project's
own CPU paths (train/optim.Adam, train/schedule.noam_lr, the model's
log_softmax loss) agree with the references under the same comparators."""
import functools
import math

import pytest
import torch

import ref_tail as R
from ref_tail import F32, F64, AdamCfg


def _rejected(fn):
    try:
        fn()
    except R.Mismatch:
        return True
    return False


# --------------------------------------------------------------------------- cross-entropy
def _check_xent(out, V, ref, lg, workers, what):
    """The checks of the GPU test on one (row_loss, row_correct, ntok, dlogits)."""
    loss, correct, ntok, d = ref
    R.close_f32(out[0], loss, "row_loss", what + " row_loss", scale=R.row_loss_scale(lg[:, :V]))
    R.exact(out[1].to(F32), correct.to(F32), what + " row_correct")
    if out[2] != ntok:
        raise R.Mismatch(f"{what}: ntok {out[2]} vs {ntok}")
    R.close_dlogits(out[3], d, V, R.xent_scale(ntok, workers), what + " dlogits")


def _xent_settings(V, ldl):
    M = 16 if V == 32000 else 40
    lg, lab = R.xent_rows(V, ldl, M)
    for s in R.XENT_SMOOTHING:
        for w in R.XENT_WORKERS:
            yield lg, lab, s, w, R.ref_xent(lg[:, :V], lab, w, s)


def _mutant_applies(mut, V, ldl, s, w):
    """Where the mutant changes the maths by more than the comparators allow."""
    return {"lse_over_ldl": ldl > V,
            "no_smoothing_offset": s > 0 and V <= 2048,  # s / V against atol_g
            "smoothing_mean_over_ldl": s > 0 and ldl > V,
            "last_argmax": True,
            "no_workers": w != 1.0,
            "pad_row_grad": True,
            "pad_cols_kept": ldl > V}[mut]


@functools.lru_cache(maxsize=None)
def _xent_verdicts(V, ldl):
    """{mutant: [(rejected, expected)]} over the settings of one shape; the
    f32 evaluation itself must pass."""
    out = {m: [] for m in R.XENT_MUTANTS}
    for lg, lab, s, w, ref in _xent_settings(V, ldl):
        what = f"V={V} ldl={ldl} s={s} w={w}"
        _check_xent(R.xent_f32(lg, V, lab, w, s), V, ref, lg, w, what)
        for m in R.XENT_MUTANTS:
            got = R.xent_f32(lg, V, lab, w, s, mutant=m)
            out[m].append((_rejected(lambda: _check_xent(got, V, ref, lg, w, what)),
                           _mutant_applies(m, V, ldl, s, w), what))
    return out


@pytest.mark.parametrize("V,ldl", R.XENT_SHAPES)
def test_xent_f32_accepted_mutants_rejected(V, ldl):
    for m, res in _xent_verdicts(V, ldl).items():
        for rejected, expected, what in res:
            assert rejected or not expected, f"mutant {m} accepted at {what}"


def test_every_xent_mutant_rejected_somewhere():
    for m in R.XENT_MUTANTS:
        assert any(r for sh in [(5, 8), (250, 256), (1001, 1002)] for r, _, _ in _xent_verdicts(*sh)[m]), m


def test_xent_rows_hold_what_they_promise():
    for V, ldl in R.XENT_SHAPES:
        lg, lab = R.xent_rows(V, ldl, 16 if V == 32000 else 40)
        x = lg[:, :V].float()
        assert bool((lab == 0).any()) and bool(((lab > 0) & (lab < V)).sum() >= 8)
        assert bool(torch.isnan(lg[0::2, V:].float()).all()) and bool((lg[1::2, V:].float() > 1e38).all())
        top = x.max(-1, keepdim=True).values
        ties = (x == top).sum(-1)
        valid = lab != 0
        first, last = R._first_argmax(x), R._first_argmax(x, last=True)
        assert bool(((ties == 2) & (first == lab)).any()) and bool(((ties == 2) & (last == lab)).any())
        assert bool((ties == V).any())                         # the constant row
        assert bool((valid & (lab == V - 1) & (first == V - 1)).any())
        assert bool((x.max(-1).values - x.min(-1).values == 160).any())
        assert float(R.ref_xent(x, lab, 1.0, 0.0)[0][valid].min()) < 1e-8  # the loss ~ 0 row
    arms = {R.xent_expected_arm(V, ldl) for V, ldl in R.XENT_SHAPES}
    assert arms == {"reg1", "reg2", "reg3", "reg4", "generic"}


def test_xent_all_pad_reference():
    lg, lab = R.xent_rows(250, 256)
    lab = torch.zeros_like(lab)
    loss, correct, ntok, d = R.ref_xent(lg[:, :250], lab, 2.0, 0.1)
    assert ntok == 0 and not loss.any() and not correct.any() and not d.any()
    _check_xent(R.xent_f32(lg, 250, lab, 2.0, 0.1), 250, (loss, correct, ntok, d), lg, 2.0, "all PAD")
    assert R.ref_xent_stats(loss, correct, ntok, 2.0) == (0.0, 0.0, 0.0)


@pytest.mark.parametrize("M", R.STATS_M)
def test_xent_stats_f32(M):
    rl, rc, ntok = R.stats_rows(M)
    for w in R.XENT_WORKERS:
        loss, acc, correct = R.ref_xent_stats(rl, rc, ntok, w)
        got = R.xent_stats_f32(rl, rc, ntok, w)
        R.close_f32(torch.tensor(got[0]), torch.tensor(loss), "stats_loss", f"stats M={M}")
        R.close_accuracy(got[1], correct, ntok, f"stats M={M}")


@pytest.mark.parametrize("smoothing", [0.0, 0.1])
def test_model_cpu_loss_path(smoothing):
    """transformer.py's log_softmax branch against ref_xent."""
    from tensorflow_distributed_on_gke_amd.models.layers import RunCtx
    from tensorflow_distributed_on_gke_amd.models.transformer import Transformer, model_config

    cfg = model_config("tiny", d_model=32, heads=4, d_ff=64, src_vocab=50, tgt_vocab=40, dropout=0.0,
                       label_smoothing=smoothing)
    m = Transformer(cfg).build("cpu", seed=3)
    g = torch.Generator().manual_seed(5)
    src = torch.randint(4, 50, (3, 9), generator=g)
    tgt = torch.randint(4, 40, (3, 8), generator=g)
    src[1, 6:] = 0
    tgt[2, 5:] = 0
    workers = 2.0
    out = m.loss_and_backward(src, tgt, RunCtx(training=True, dropout=0.0, store=m.store), workers=workers)
    lg = m.logits(src, tgt[:, :-1]).reshape(-1, 40)
    lab = tgt[:, 1:].reshape(-1)
    loss, correct, ntok, d = R.ref_xent(lg, lab, workers, smoothing)
    want, acc, ncorrect = R.ref_xent_stats(loss, correct, ntok, workers)
    R.close_f32(out[0].view(1), torch.tensor([want]), "row_loss", "model loss",
                scale=float(R.row_loss_scale(lg).mean()) / workers)
    R.close_accuracy(float(out[1]), ncorrect, ntok, "model accuracy")
    # the final bias gradient is the column sum of dlogits
    gb = m.final.b.grad.double()
    assert float((gb - d.sum(0)).abs().max()) <= 1e-6 * float(d.abs().sum(0).max())


# --------------------------------------------------------------------------- Adam
def _one_step_cases():
    for d, w in R.ADAM_SCHEDULES:
        for it in R.ADAM_ITERATIONS:
            yield f"noam d={d:g} w={w:g} it={it}", AdamCfg(d_model=d, warmup=w), it
    for name, (cfg, it) in R.ADAM_OPTIONS.items():
        yield name, cfg, it


def _adam_mutant_applies(mut, cfg, it):
    lr_on = cfg.sched == 0 or it > 0
    return {"p_untouched": lr_on, "sign_flipped": lr_on,
            "lr_for_lr_t": lr_on and it <= 10,     # later both bias corrections are 1 in f32
            "t_is_iterations": it <= 10,            # (0 / 0 at iterations = 0)
            "sched_at_next": cfg.sched == 1 and it <= 4000,
            "eps_in_sqrt": lr_on,
            "no_scale_in_v": cfg.grad_scale != 1.0,
            "wd_by_lr_t": cfg.weight_decay != 0.0,
            "fall_is_rise": cfg.sched == 1 and it > cfg.warmup}[mut]


N1 = 4096 + 8


@functools.lru_cache(maxsize=None)
def _adam_verdicts():
    out = {m: [] for m in R.ADAM_MUTANTS}
    p, g, m_, v = R.adam_inputs(N1)
    for what, cfg, it in _one_step_cases():
        R.check_adam(R.adam_f32(p, g, m_, v, it, cfg)[:3], p, g, m_, v, it, cfg, what)
        for mut in R.ADAM_MUTANTS:
            got = R.adam_f32(p, g, m_, v, it, cfg, mutant=mut)[:3]
            out[mut].append((_rejected(lambda: R.check_adam(got, p, g, m_, v, it, cfg, what)),
                             _adam_mutant_applies(mut, cfg, it), what))
    return out


def test_adam_f32_accepted_mutants_rejected():
    for mut, res in _adam_verdicts().items():
        assert any(r for r, _, _ in res), f"mutant {mut} never rejected"
        for rejected, expected, what in res:
            assert rejected or not expected, f"mutant {mut} accepted at {what}"


def _f32_trajectory(p, cfg, n, mutant=None):
    """Returns dp_ratio of the f32 trajectory's accumulated update."""
    p32, m32, v32 = p.clone(), torch.zeros(n), torch.zeros(n)
    total = torch.zeros(n, dtype=F64)
    for k, g, gmax, pr, mr, vr in R.ref_trajectory(p, cfg, n):
        p32, m32, v32, dp = R.adam_f32(p32, g, m32, v32, R.TRAJ_START + k, cfg, mutant)
        total += dp.double()
        R.close_f32(m32, mr, "adam_m_traj", f"step {k} m", scale=gmax)
        R.close_f32(v32, vr, "adam_v_traj", f"step {k} v", scale=gmax * gmax)
    R.close_p(p32, p, p.double() - pr, "trajectory p", "adam_dp_traj", steps=R.TRAJ_STEPS)
    return R.dp_ratio(total, p, p.double() - pr, steps=R.TRAJ_STEPS)


def test_adam_trajectory_f32():
    cfg = AdamCfg()
    p = R.adam_inputs(N1, zero_moments=True)[0]
    _f32_trajectory(p, cfg, N1)
    for mut in ("p_untouched", "sign_flipped", "sched_at_next", "eps_in_sqrt", "fall_is_rise"):
        assert _rejected(lambda: _f32_trajectory(p, cfg, N1, mut)), mut


def test_adam_edges_f32():
    cfg = AdamCfg()
    for n in (4, N1):
        p = R.adam_inputs(n)[0]
        z = torch.zeros(n)
        got = R.adam_f32(p, z, z, z, 10, cfg)
        R.exact(got[0], p, "g = 0: p")
        assert not got[1].any() and not got[2].any()
        R.check_adam(got[:3], p, z, z, z, 10, cfg, "g = 0")
        p, g, m, v = R.adam_inputs(n)
        R.check_adam(R.adam_f32(p, g, m, v, 10, cfg)[:3], p, g, m, v, 10, cfg, f"n={n}")


def test_adam_capped_grid_size_f32():
    n = R.ADAM_CAPPED_N
    assert n % 4 == 0 and n // 4 == 2 * 8192 * 256 + 1001 and n > 8388608
    cfg = AdamCfg()
    p, g, m, v = R.adam_inputs(n)
    R.check_adam(R.adam_f32(p, g, m, v, 10, cfg)[:3], p, g, m, v, 10, cfg, "capped grid size")


def test_adam_reference_is_torch_adam():
    """eps = 0, constant lr, no decay: the float64 reference is
    torch.optim.Adam(eps=0) in float64 over 5 steps, to 1e-12 relative."""
    n = 512
    cfg = AdamCfg(eps=0.0, sched=0, lr_const=1e-2)
    g_ = torch.Generator().manual_seed(1)
    p0 = torch.randn(n, generator=g_) * 0.05
    w = torch.nn.Parameter(p0.double().clone())
    opt = torch.optim.Adam([w], lr=R._f32r(cfg.lr_const), betas=(R._f32r(0.9), R._f32r(0.98)), eps=0.0)
    pr, mr, vr = p0.double(), torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
    for k in range(5):
        g = torch.randn(n, generator=g_)
        w.grad = g.double().clone()
        opt.step()
        pr, mr, vr, _ = R.ref_adam_step(pr, g, mr, vr, k, cfg)
        rel = ((pr - w.detach()).abs() / w.detach().abs()).max().item()
        assert rel <= 1e-12, (k, rel)
        st = opt.state[w]
        assert ((mr - st["exp_avg"]).abs() <= 1e-12 * mr.abs()).all()
        assert ((vr - st["exp_avg_sq"]).abs() <= 1e-12 * vr.abs()).all()


@pytest.mark.parametrize("d,w", R.ADAM_SCHEDULES)
def test_noam_schedule(d, w):
    from tensorflow_distributed_on_gke_amd.train.schedule import NoamSchedule, noam_lr

    assert R.ref_noam(0, d, w) == 0.0 and noam_lr(0, int(d), w) == 0.0
    peak = R.ref_noam(w, d, w)
    assert abs(peak - d ** -0.5 * w ** -0.5) <= 1e-15
    _noam_accepted(d, w)
    for it in R.ADAM_ITERATIONS:
        cfg = AdamCfg(d_model=d, warmup=w)
        if it > w:
            assert _rejected(lambda: R.close_f32(R.noam_f32(it, cfg, "fall_is_rise").view(1),
                                                 torch.tensor([R.ref_noam(it, d, w)]), "noam", "mutant"))


def _noam_accepted(d, w):
    from tensorflow_distributed_on_gke_amd.train.schedule import NoamSchedule, noam_lr

    peak = R.ref_noam(w, d, w)
    for it in R.ADAM_ITERATIONS + (int(w) - 1, int(w), int(w) + 1):
        ref = R.ref_noam(it, d, w)
        assert ref <= peak * (1 + 1e-15)
        for got in (noam_lr(it, int(d), w), NoamSchedule(int(d), w)(it)):
            R.close_f32(torch.tensor([got], dtype=F64), torch.tensor([ref]), "noam", f"noam_lr({it})")
        cfg = AdamCfg(d_model=d, warmup=w)
        R.close_f32(R.noam_f32(it, cfg).view(1), torch.tensor([ref]), "noam", f"noam_f32({it})")


def _cpu_optimizer(p, g, m, v, it, cfg):
    from tensorflow_distributed_on_gke_amd.models.params import ParamStore, const
    from tensorflow_distributed_on_gke_amd.train.optim import Adam

    s = ParamStore()
    s.add("w", (p.numel(),), const(0.0))
    s.finalize("cpu")
    assert s.total == p.numel()
    s.flat.copy_(p)
    s.flat_grad.copy_(g)
    opt = Adam(s, int(cfg.d_model), cfg.warmup, cfg.beta1, cfg.beta2, cfg.eps,
               lr=None if cfg.sched else cfg.lr_const, weight_decay=cfg.weight_decay)
    opt.m.copy_(m)
    opt.v.copy_(v)
    opt.step.fill_(it)
    return s, opt


def test_optim_adam_cpu_path():
    """train/optim.Adam on the CPU under the comparators of the kernels."""
    n = 4096
    p, g, m, v = R.adam_inputs(n)
    for what, cfg, it in _one_step_cases():
        s, opt = _cpu_optimizer(p, g, m, v, it, cfg)
        opt.apply(grad_scale=cfg.grad_scale)
        R.check_adam((s.flat, opt.m, opt.v), p, g, m, v, it, cfg, "optim.Adam " + what)
        assert opt.iterations == it + 1 and not s.flat_grad.any()
    # two ranges of one step: the first keeps `iterations`, the second sees the same step
    cfg = AdamCfg()
    s, opt = _cpu_optimizer(p, g, m, v, 10, cfg)
    opt.apply_range(0, 2048, inc_step=False)
    assert opt.iterations == 10
    opt.apply_range(2048, n, inc_step=True)
    assert opt.iterations == 11
    R.check_adam((s.flat, opt.m, opt.v), p, g, m, v, 10, cfg, "optim.Adam ranges")


# --------------------------------------------------------------------------- to_bf16 inputs
def test_to_bf16_inputs_hold_the_edges():
    x = R.to_bf16_inputs(4099)
    b = x.to(torch.bfloat16).float()
    one = torch.tensor([1.0])
    assert bool(((x == 1 + 2.0 ** -8) & (b == 1.0)).any())            # tie to even: down
    assert bool(((x == 1 + 3 * 2.0 ** -8) & (b == 1 + 2.0 ** -6)).any())  # tie to even: up
    assert bool((torch.isinf(b) & torch.isfinite(x)).any())           # largest finite -> inf
    assert bool(torch.isinf(x).any()) and bool(((x == 0) & torch.signbit(x)).any())
    assert not torch.isnan(x).any() and one.item() == 1.0
    assert R.to_bf16_inputs(1).numel() == 1


# --------------------------------------------------------------------------- the table
def _measure_e32():
    """E32 of every entry of ref_tail.E32 over the cases above (the unit of
    each entry is the comparator's own ratio)."""
    R.WORST.clear()
    dl = 0.0
    for V, ldl in R.XENT_SHAPES:
        for lg, lab, s, w, ref in _xent_settings(V, ldl):
            out = R.xent_f32(lg, V, lab, w, s)
            _check_xent(out, V, ref, lg, w, "measure")
            d32 = R.xent_f32(lg, V, lab, w, s, keep_f32=True)[3][:, :V].double()
            dl = max(dl, float((d32 - ref[3]).abs().max()) / R.xent_scale(ref[2], w))
    for M in R.STATS_M:
        test_xent_stats_f32(M)
    p, g, m, v = R.adam_inputs(N1)
    dp1 = 0.0
    for what, cfg, it in _one_step_cases():
        out = R.adam_f32(p, g, m, v, it, cfg)
        dp1 = max(dp1, R.dp_ratio(out[3], p, R.check_adam(out[:3], p, g, m, v, it, cfg, what)[3]))
    test_adam_edges_f32()
    dpt = _f32_trajectory(R.adam_inputs(N1, zero_moments=True)[0], AdamCfg(), N1)
    for d, w in R.ADAM_SCHEDULES:
        _noam_accepted(d, w)
    got = dict(R.WORST)
    got["adam_dp"], got["adam_dp_traj"] = dp1, dpt  # of the update itself (ref_tail.dp_ratio)
    got["dlogits"] = dl  # the f32 gradient before its bf16 rounding (which 2^-8 |ref| covers)
    return got


def test_e32_table_is_measured():
    """Every tolerance is 8 x an E32 that this machine reproduces: not below
    what the float32 evaluation needs, and not inflated."""
    got = _measure_e32()
    print("measured E32:", {k: f"{v:.2e}" for k, v in sorted(got.items())})
    assert set(got) == set(R.E32)
    for k, e in R.E32.items():
        # (1.5: the summation order of another host's vector unit; the f32 evaluation
        # itself is held to 8 x E32 by every test above)
        assert got[k] <= 1.5 * e, f"{k}: measured {got[k]:.3e} above the table's {e:.3e}"
        assert got[k] >= e / 4, f"{k}: the table's {e:.3e} is more than 4x the measured {got[k]:.3e}"
    assert R.MARGIN == 8.0 and all(math.isclose(R.tol(k), 8 * e) for k, e in R.E32.items())
