"""The R-Drop training step on the GPU: against the CPU f32 model on the GPU's
bf16-rounded weights (the bounds of tests/test_gpu_distill_step.py), captured
against eager, rdrop_alpha = 0 against the plain step, and what the two
dropout masks do to the objective."""
import pytest
import torch

from tensorflow_distributed_on_gke_amd.data.synthetic import SyntheticPairs
from tensorflow_distributed_on_gke_amd.models.layers import RunCtx
from tensorflow_distributed_on_gke_amd.models.transformer import Transformer, model_config
from tensorflow_distributed_on_gke_amd.train.optim import Adam
from tensorflow_distributed_on_gke_amd.train.step import TrainStep

pytestmark = pytest.mark.gpu
SRC_V, TGT_V, B, L = 300, 250, 6, 40


def _cfg(**over):
    return model_config("tiny", **dict(dict(src_vocab=SRC_V, tgt_vocab=TGT_V, dropout=0.1, label_smoothing=0.1), **over))


def _data():
    return SyntheticPairs(B, L, L + 1, SRC_V, TGT_V, seed=3, min_len=5)


def test_gpu_step_matches_cpu():
    """(Both devices draw the same Philox masks: seed, counter, position.)"""
    gpu = Transformer(_cfg()).build("cuda", seed=11)
    cpu = Transformer(_cfg()).build("cpu", seed=11)
    cpu.store.flat.copy_(gpu.store.flat_compute.float().cpu())
    src, tgt = _data().batch(0)
    outs, labs = [], []
    for m, dev in ((gpu, "cuda"), (cpu, "cpu")):
        rt = RunCtx(training=True, dropout=0.1, seed=99,
                    ctr=torch.tensor([2], dtype=torch.int64, device=dev), store=m.store)
        la = torch.zeros(4, device=dev)
        outs.append(m.loss_and_backward(src.to(dev), tgt.to(dev), rt, workers=1.0, rdrop_alpha=5.0,
                                        label_accum=la).cpu())
        labs.append(la.cpu())
    print("loss", outs[0][0].item(), outs[1][0].item(), "label", labs[0][0].item(), labs[1][0].item())
    assert labs[0][3] == labs[1][3] == 2 * float((tgt[:, 1:] != 0).sum())  # both copies' labels
    assert abs(outs[0][0] - outs[1][0]) < 2e-2 * abs(outs[1][0])
    assert abs(labs[0][0] - labs[1][0]) < 2e-2 * abs(labs[1][0])
    rel = lambda a, b: ((a.float().cpu() - b.float()).norm() / (b.float().norm() + 1e-12)).item()
    errs = {p_g.name: rel(p_g.grad, p_c.grad) for p_g, p_c in zip(gpu.store.params, cpu.store.params)}
    worst, med = max(errs, key=errs.get), sorted(errs.values())[len(errs) // 2]
    print(f"worst {worst} {errs[worst]:.3e} median {med:.3e}")
    assert errs[worst] < 0.2 and med < 0.08, f"{worst}: rel grad err {errs[worst]:.3e}, median {med:.3e}"


def _run(accum_steps, graph, updates=3, dropout=0.1, **step_kw):
    m = Transformer(_cfg(dropout=dropout)).build("cuda", seed=1)
    opt = Adam(m.store, m.cfg.d_model, lr=1e-3)
    step = TrainStep(m, opt, None, workers=1, seed=5, accum_steps=accum_steps, **step_kw)
    data = _data()
    batches = [[tuple(t.cuda() for t in data.batch(u * accum_steps + k)) for k in range(accum_steps)]
               for u in range(updates)]
    if graph:
        assert step.capture(*batches[0][0])
        assert opt.iterations == 0 and float(step.accum.abs().sum()) == 0  # capture() trains nothing
    shares = []
    for mbs in batches:  # (captured: three replays)
        step.update(mbs)
        shares.append(step.last.clone())
    torch.cuda.synchronize()
    assert opt.iterations == updates
    la = step.label_accum.clone() if step.label_accum is not None else torch.zeros(0)
    return m.store.flat.clone(), torch.stack(shares), step.accum.clone(), la


@pytest.mark.parametrize("accum_steps,loss_mode", [(1, "replica_mean"), (2, "replica_mean"), (2, "global_mean")])
def test_captured_step_equals_eager_bitwise(accum_steps, loss_mode):
    e = _run(accum_steps, False, loss_mode=loss_mode, rdrop_alpha=5.0)
    g = _run(accum_steps, True, loss_mode=loss_mode, rdrop_alpha=5.0)
    for a, b, name in zip(e, g, ("weights", "loss shares", "accum", "label_accum")):
        assert torch.equal(a, b), f"captured vs eager: {name}"
    accum, label = g[2].cpu(), g[3].cpu()
    assert accum[2] == 3 * accum_steps and label[2] == 3 * accum_steps and label[3] == accum[3]
    assert label[0] > 0 and accum[0] > label[0] and label[1] == accum[1]


def test_rdrop_alpha_zero_is_the_plain_step_bitwise():
    for a, b, name in zip(_run(1, False), _run(1, False, rdrop_alpha=0.0), ("weights", "loss shares", "accum")):
        assert torch.equal(a, b), f"rdrop_alpha=0 vs plain: {name}"


def test_objective_is_the_label_loss_only_without_dropout():
    """dropout = 0: the copies coincide bitwise, the KL is exactly 0;
    dropout = 0.1: the masks differ, the objective is strictly larger."""
    _, _, accum, label = _run(1, False, updates=1, dropout=0.0, rdrop_alpha=5.0)
    assert float(label[0]) > 0 and float(accum[0]) == float(label[0])
    _, _, accum, label = _run(1, False, updates=1, rdrop_alpha=5.0)
    assert float(accum[0]) > float(label[0]) * (1 + 1e-4) > 0
