"""The distillation training step on the GPU: against the CPU f32 model on the
GPU's bf16-rounded weights (the bounds of tests/test_gpu_model.py), captured
against eager, and what it must leave alone."""
import pytest
import torch

from tensorflow_distributed_on_gke_amd.data.synthetic import SyntheticPairs
from tensorflow_distributed_on_gke_amd.models.layers import RunCtx
from tensorflow_distributed_on_gke_amd.models.transformer import Transformer, model_config
from tensorflow_distributed_on_gke_amd.train.distill import Teacher
from tensorflow_distributed_on_gke_amd.train.optim import Adam
from tensorflow_distributed_on_gke_amd.train.step import TrainStep

pytestmark = pytest.mark.gpu
SRC_V, TGT_V, B, L = 300, 250, 6, 40
WEIGHTS = (1.0, 3.0)


def _cfg(**over):
    kw = dict(src_vocab=SRC_V, tgt_vocab=TGT_V, dropout=0.1, label_smoothing=0.1)
    kw.update(over)
    return model_config("tiny", **kw)


def _pair(seed, **over):
    """The same model on the GPU and on the CPU, the latter with the GPU's
    bf16-rounded weights."""
    cfg = _cfg(**over)
    gpu = Transformer(cfg).build("cuda", seed=seed)
    cpu = Transformer(cfg).build("cpu", seed=seed)
    cpu.store.flat.copy_(gpu.store.flat_compute.float().cpu())
    return gpu, cpu


def _data(seed=3):
    return SyntheticPairs(B, L, L + 1, SRC_V, TGT_V, seed=seed, min_len=5)


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def test_gpu_step_matches_cpu():
    gpu, cpu = _pair(11)
    tg, tc = zip(*[_pair(21 + i) for i in range(2)])
    teachers = {"cuda": Teacher(tg, WEIGHTS), "cpu": Teacher(tc, WEIGHTS)}
    src, tgt = _data().batch(0)
    outs, labs = [], []
    for m, dev in ((gpu, "cuda"), (cpu, "cpu")):
        rt = RunCtx(training=True, dropout=0.1, seed=99,
                    ctr=torch.tensor([2], dtype=torch.int64, device=dev), store=m.store)
        la = torch.zeros(4, device=dev)
        outs.append(m.loss_and_backward(src.to(dev), tgt.to(dev), rt, workers=1.0, teacher=teachers[dev],
                                        alpha=0.5, label_accum=la).cpu())
        labs.append(la.cpu())
    print("loss", outs[0][0].item(), outs[1][0].item(), "label", labs[0][0].item(), labs[1][0].item())
    assert abs(outs[0][0] - outs[1][0]) < 2e-2 * abs(outs[1][0])
    assert abs(labs[0][0] - labs[1][0]) < 2e-2 * abs(labs[1][0])
    errs = {p_g.name: _rel(p_g.grad, p_c.grad) for p_g, p_c in zip(gpu.store.params, cpu.store.params)}
    worst = max(errs, key=errs.get)
    med = sorted(errs.values())[len(errs) // 2]
    print(f"worst {worst} {errs[worst]:.3e} median {med:.3e}")
    assert errs[worst] < 0.2, f"{worst}: rel grad err {errs[worst]:.3e}"
    assert med < 0.08, f"median rel grad err {med:.3e}"


def _make(accum_steps=1, teacher_cfg=None):
    m = Transformer(_cfg()).build("cuda", seed=1)
    te = Teacher([Transformer(teacher_cfg or _cfg()).build("cuda", seed=31 + i) for i in range(2)], WEIGHTS)
    opt = Adam(m.store, m.cfg.d_model, lr=1e-3)
    step = TrainStep(m, opt, None, workers=1, seed=5, accum_steps=accum_steps, teacher=te, distill_alpha=0.5)
    return m, te, opt, step


def _run(accum_steps, graph, updates=3):
    m, te, opt, step = _make(accum_steps)
    frozen = [t.store.flat.clone() for t in te.models]
    data = _data()
    batches = [[tuple(t.cuda() for t in data.batch(u * accum_steps + k)) for k in range(accum_steps)]
               for u in range(updates)]
    if graph:
        assert step.capture(*batches[0][0])
        torch.cuda.synchronize()
        assert opt.iterations == 0 and float(step.accum.abs().sum()) == 0  # capture() trains nothing
        assert float(step.label_accum.abs().sum()) == 0
        assert sorted(k[2] for k in step.cache.entries) == (["only"] if accum_steps == 1 else ["first", "last"])
    shares = []
    for mbs in batches:
        step.update(mbs)
        shares.append(step.last.clone())
    torch.cuda.synchronize()
    assert opt.iterations == updates
    for t, f in zip(te.models, frozen):
        assert torch.equal(t.store.flat, f), "teacher weights changed"
    assert all(s.data_ptr() != t.store.flat.data_ptr() for s in step._state() for t in te.models)
    return m.store.flat.clone(), torch.stack(shares), step.accum.clone(), step.label_accum.clone()


@pytest.mark.parametrize("accum_steps", [1, 2])
def test_captured_step_equals_eager_bitwise(accum_steps):
    e = _run(accum_steps, False)
    g = _run(accum_steps, True)
    for a, b, name in zip(e, g, ("weights", "loss shares", "accum", "label_accum")):
        assert torch.equal(a, b), f"captured vs eager: {name}"
    accum, label = g[2].cpu(), g[3].cpu()
    assert accum[2] == 3 * accum_steps and label[2] == 3 * accum_steps and label[3] == accum[3]
    # another number than the objective: apart by far more than f32 rounding of either sum
    assert label[0] > 0 and abs(float(label[0] - accum[0])) > 1e-5 * float(accum[0])
    assert label[1] == accum[1]  # the accuracy is that of the student's argmax either way


def _shape_batches():
    """Updates of two batch shapes (the per-shape graph cache of text data)."""
    out = []
    for i, (b, l) in enumerate([(6, 40), (4, 24), (6, 40), (4, 24)]):
        d = SyntheticPairs(b, l, l + 1, SRC_V, TGT_V, seed=50 + i, min_len=5)
        out.append(tuple(t.cuda() for t in d.batch(0)))
    return out


def test_shape_cache_with_a_teacher_equals_eager_bitwise():
    res = []
    for graph in (False, True):
        m, te, opt, step = _make()
        batches = _shape_batches()
        if graph:
            step.bucketed = True
            assert step.capture(*batches[0])
        for b in batches:
            step(*b)
        torch.cuda.synchronize()
        if graph:
            assert step.cached_shapes == 2 and step.graph_stats["replays"] == 4
        res.append((m.store.flat.clone(), step.accum.clone(), step.label_accum.clone()))
    for a, b, name in zip(res[0], res[1], ("weights", "accum", "label_accum")):
        assert torch.equal(a, b), f"shape cache vs eager: {name}"


def test_teacher_of_another_width_runs():
    m, te, opt, step = _make(teacher_cfg=_cfg(d_model=512, heads=8, d_ff=2048))
    assert te.models[0].vocab_pad == m.vocab_pad and te.cfg.d_model != m.cfg.d_model
    data = _data()
    start = m.store.flat.clone()
    for i in range(2):
        out = step(*(t.cuda() for t in data.batch(i)))
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and torch.isfinite(m.store.flat).all()
    assert not torch.equal(m.store.flat, start)


def test_distillation_pulls_the_student_to_the_teacher():
    """alpha = 1 on a fixed batch: the objective (cross entropy against the
    teacher's distribution) falls."""
    m = Transformer(_cfg(dropout=0.0)).build("cuda", seed=1)
    te = Teacher([Transformer(_cfg(dropout=0.0)).build("cuda", seed=41)])
    opt = Adam(m.store, m.cfg.d_model, lr=1e-3)
    step = TrainStep(m, opt, None, workers=1, seed=5, teacher=te, distill_alpha=1.0)
    src, tgt = (t.cuda() for t in _data().batch(0))
    losses = [float(step(src, tgt)[0]) for _ in range(30)]
    assert losses[-1] < 0.9 * losses[0], losses[::5]
