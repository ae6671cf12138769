"""Word-level distillation on the CPU model: the training step with a Teacher
against a torch autograd evaluation of the definition, what it must leave
alone (the plain step, the teachers), the settings, and gradient accumulation
with a teacher."""
import pytest
import torch

import ref_accum
import ref_model
from test_parallel_cpu import _fill
from tensorflow_distributed_on_gke_amd.config import check_distill, load_settings
from tensorflow_distributed_on_gke_amd.data.synthetic import SyntheticPairs
from tensorflow_distributed_on_gke_amd.models.layers import RunCtx
from tensorflow_distributed_on_gke_amd.models.transformer import Transformer, model_config
from tensorflow_distributed_on_gke_amd.ops import kernels as K
from tensorflow_distributed_on_gke_amd.train.distill import Teacher
from tensorflow_distributed_on_gke_amd.train.optim import Adam
from tensorflow_distributed_on_gke_amd.train.step import TrainStep

SRC_V, TGT_V, B, L = 300, 250, 6, 40
SMOOTH = 0.1


def _model(seed, **over):
    kw = dict(src_vocab=SRC_V, tgt_vocab=TGT_V, dropout=0.0, label_smoothing=SMOOTH)
    kw.update(over)
    return Transformer(model_config("tiny", **kw)).build("cpu", seed=seed)


def _data(seed=3):
    return SyntheticPairs(B, L, L + 1, SRC_V, TGT_V, seed=seed, min_len=5)


def _teacher(n=2, weights=(1.0, 3.0)):
    return Teacher([_model(11 + i) for i in range(n)], weights)


def _rt(m, **kw):
    return RunCtx(training=True, dropout=0.0, seed=5, ctr=torch.zeros(1, dtype=torch.int64),
                  store=m.store, **kw)


def _oracle(student, teacher, src, tgt, alpha, workers):
    """The definition in float64 autograd on the same weights: target =
    (1 - alpha) ((1 - s) onehot + s / V) + alpha sum_m w_m softmax(z_m)."""
    W = ref_model.tf_weights(student)
    tgt_in, real = tgt[:, :-1], tgt[:, 1:].reshape(-1)
    logits = ref_model.forward(W, src, tgt_in, student.cfg).reshape(-1, TGT_V)
    with torch.no_grad():
        q = sum(w * torch.softmax(ref_model.forward(ref_model.tf_weights(t), src, tgt_in, t.cfg)
                                  .reshape(-1, TGT_V), -1)
                for t, w in zip(teacher.models, teacher.weights))
    mask = (real != 0).double()
    hard = torch.nn.functional.one_hot(real, TGT_V).double() * (1 - SMOOTH) + SMOOTH / TGT_V
    target = (1 - alpha) * hard + alpha * q
    logp = torch.log_softmax(logits, -1)
    loss = (-(target * logp).sum(-1) * mask).sum() / mask.sum() / workers
    label = (-(hard * logp).sum(-1) * mask).sum() / mask.sum() / workers
    return W, loss, label


@pytest.mark.parametrize("workers", [1.0, 2.0])
def test_step_matches_autograd_of_the_definition(workers):
    m, te = _model(1), _teacher()
    src, tgt = _data().batch(0)
    lab_acc = torch.zeros(4)
    out = m.loss_and_backward(src, tgt, _rt(m), workers, teacher=te, alpha=0.5, label_accum=lab_acc)
    W, loss, label = _oracle(m, te, src, tgt, 0.5, workers)
    loss.backward()
    assert abs(out[0].item() - loss.item()) <= 1e-5 * abs(loss.item())
    assert abs(lab_acc[0].item() - label.item()) <= 1e-5 * abs(label.item())
    assert lab_acc[2] == 1 and abs(label.item() - loss.item()) > 1e-3  # another number than the objective
    ours = ref_model.internal_grads_tf(m)
    assert set(ours) == set(W)
    # (the key biases' gradient is identically zero -- softmax is invariant to
    # them -- and the f32 model leaves summation noise there: one f32 ulp of
    # the largest gradient norm is the floor)
    floor = 2.0 ** -23 * max(float(t.grad.norm()) for t in W.values())
    for k, t in W.items():
        err, ref = (ours[k] - t.grad).norm(), t.grad.norm()
        assert err <= 1e-4 * ref + floor, f"{k}: |diff| {err:.3e} vs |grad| {ref:.3e}"


def test_alpha_zero_and_no_teacher_are_the_plain_step():
    src, tgt = _data().batch(0)
    te = _teacher()
    runs = []
    for kw in ({}, dict(teacher=te, alpha=0.0), dict(teacher=None, alpha=0.5)):
        m = _model(1)
        out = m.loss_and_backward(src, tgt, _rt(m), 2.0, **kw)
        runs.append((out.clone(), m.store.flat_grad.clone()))
    for out, grad in runs[1:]:
        assert torch.equal(out, runs[0][0]) and torch.equal(grad, runs[0][1])
    m = _model(1)
    m.loss_and_backward(src, tgt, _rt(m), 2.0, teacher=te, alpha=0.5)
    assert not torch.equal(m.store.flat_grad, runs[0][1])  # and the teacher does change the step


def test_teachers_are_left_alone():
    m, te = _model(1), _teacher()
    opt = Adam(m.store, m.cfg.d_model, lr=0.05, eps=1.0)
    before = [t.store.flat.clone() for t in te.models]
    step = TrainStep(m, opt, None, workers=1, seed=5, teacher=te, distill_alpha=0.5)
    data = _data()
    start = m.store.flat.clone()
    for i in range(2):
        step(*data.batch(i))
    assert not torch.equal(m.store.flat, start)
    for t, b in zip(te.models, before):
        assert torch.equal(t.store.flat, b)
        assert not bool(t.store.flat_grad.any()), "a teacher received a gradient"
        assert all(p.master.grad is None for p in t.store.params)
    assert all(t is not s for s in step._state() for tm in te.models for t in (tm.store.flat,))
    assert step.label_accum[2] == 2 and step.accum[2] == 2
    assert abs(float(step.label_accum[0] - step.accum[0])) > 1e-3


def test_teacher_of_another_width_and_validation():
    m = _model(1)
    te = Teacher([_model(21, d_model=64, heads=4, d_ff=128)])
    src, tgt = _data().batch(0)
    out = m.loss_and_backward(src, tgt, _rt(m), 1.0, teacher=te, alpha=1.0)
    assert torch.isfinite(out).all()
    with pytest.raises(ValueError, match="vocabular"):
        TrainStep(m, Adam(m.store, 128), None, workers=1, teacher=Teacher([_model(2, tgt_vocab=99)]),
                  distill_alpha=0.5)
    with pytest.raises(ValueError, match="1 to 8"):
        Teacher([])
    with pytest.raises(ValueError, match="weights"):
        Teacher([m], [1.0, 2.0])
    with pytest.raises(ValueError, match="> 0"):
        Teacher([m], [0.0])
    with pytest.raises(ValueError, match="alpha"):
        m.loss_and_backward(src, tgt, _rt(m), 1.0, teacher=te, alpha=1.5)


def test_wrapper_cpu_branch_is_the_definition():
    """ops.kernels.xent_distill on the CPU against ref_distill's float64 reference."""
    import ref_distill as D
    V, ldl, T = 250, 256, 3
    lg, lab, te = D.teacher_rows(V, ldl, T)
    x = lg.float()
    M = x.shape[0]
    rl, rb, rc = torch.zeros(M), torch.zeros(M), torch.zeros(M)
    ntok = torch.tensor([float((lab != 0).sum())])
    K.xent_distill(x, te, V, lab, ntok, 2.0, 0.1, 0.5, D.WEIGHTS[T], rl, rc, rb)
    ref = D.ref_xent_distill(lg[:, :V], [t[:, :V] for t in te], lab, 2.0, 0.1, 0.5, D.WEIGHTS[T])
    D.check((rl, rb, rc, float(ntok), x.to(torch.bfloat16)), V, ref, lg, 2.0, "CPU branch")
    for bad in (dict(teachers=[]), dict(teachers=te * 3), dict(alpha=1.5), dict(alpha=-0.1),
                dict(weights=[1.0]), dict(weights=[1.0, -1.0, 1.0])):
        kw = dict(teachers=te, alpha=0.5, weights=None)
        kw.update(bad)
        with pytest.raises(RuntimeError, match="xent_distill"):
            K.xent_distill(x, kw["teachers"], V, lab, ntok, 2.0, 0.1, kw["alpha"], kw["weights"], rl, rc)


def test_settings_validation():
    assert check_distill(None) == ([], None, 0.0)
    assert check_distill("a/model_weights, b") == (["a/model_weights", "b"], None, 0.5)
    assert check_distill("a,b", "1,3", 1) == (["a", "b"], [1.0, 3.0], 1.0)
    assert check_distill("a", 2, 0.25) == (["a"], [2.0], 0.25)
    for args, msg in (((None, "1,2"), "without distill_teacher"),
                      ((None, None, 0.5), "without distill_teacher"),
                      (("a,b", "1"), "1 values for 2 teachers"),
                      (("a", "0"), "> 0"),
                      (("a", "x"), "numbers"),
                      (("a", None, 0.0), r"\(0, 1\]"),
                      (("a", None, 1.5), r"\(0, 1\]"),
                      (("a", None, None, "fp8"), "fp8"),
                      ((",".join("abcdefghi"),), "at most 8")):
        with pytest.raises(ValueError, match=msg):
            check_distill(*args)
    s = load_settings(None, ["distill_teacher=a,b", "distill_weights=2,1", "distill_alpha=0.75"])
    assert check_distill(s.distill_teacher, s.distill_weights, s.distill_alpha, s.dtype) == \
        (["a", "b"], [2.0, 1.0], 0.75)
    assert load_settings(None, []).distill_teacher is None
    for sets, msg in ((["distill_weights=1,2"], "without distill_teacher"),
                      (["distill_teacher=a", "distill_alpha=2"], r"\(0, 1\]"),
                      (["distill_teacher=a", "dtype=fp8"], "fp8")):
        with pytest.raises(ValueError, match=msg):
            load_settings(None, sets)


def test_two_micro_batches_with_a_teacher_match_two_replicas():
    """accum_steps = 2 under the global token mean: the update of two
    replicas, each normalised by the label count of both (ref_accum)."""
    te = _teacher()
    datas = [SyntheticPairs(B, L, L + 1, SRC_V, TGT_V, seed=3, rank=r, world=2, min_len=5) for r in range(2)]
    m = _model(1)
    opt = Adam(m.store, m.cfg.d_model, lr=0.05, eps=1.0)
    step = TrainStep(m, opt, None, workers=1, seed=5, loss_mode="global_mean", accum_steps=2,
                     teacher=te, distill_alpha=0.5)
    r = _model(1)
    ropt = Adam(r.store, r.cfg.d_model, lr=0.05, eps=1.0)
    for i in range(2):
        micro = [d.batch(i) for d in datas]
        before = step.accum.clone()
        step.update(micro)
        n_all = float(ref_accum.count_labels_ref([t for _, t in micro])[0])
        tot = 0.0
        for k, (src, tgt) in enumerate(micro):
            rt = RunCtx(training=True, dropout=0.0, seed=5, ctr=torch.zeros(1, dtype=torch.int64),
                        accumulate=k > 0)
            tot = tot + r.loss_and_backward(src, tgt, rt, 1.0, ntok_sum=_fill(n_all), teacher=te,
                                            alpha=0.5)[0].clone()
        ropt.apply()
        assert torch.allclose((step.accum - before)[0], tot, atol=1e-6)
        assert torch.allclose(m.store.flat, r.store.flat, atol=1e-6, rtol=1e-5)
    assert opt.iterations == 2
