"""The training step with attention dropout on the GPU: gradients against the
CPU f32 model under the same seed and counter (the bounds of
tests/test_gpu_model.py), and fresh masks per replay of a captured step."""
import pytest
import torch

from tensorflow_distributed_on_gke_amd.data.synthetic import SyntheticPairs
from tensorflow_distributed_on_gke_amd.models.layers import RunCtx
from tensorflow_distributed_on_gke_amd.models.transformer import Transformer, model_config
from tensorflow_distributed_on_gke_amd.train.optim import Adam
from tensorflow_distributed_on_gke_amd.train.step import TrainStep

pytestmark = pytest.mark.gpu
SRC_V, TGT_V, B, L = 300, 250, 4, 40


def _cfg():
    return model_config("tiny", src_vocab=SRC_V, tgt_vocab=TGT_V, dropout=0.0, attention_dropout=0.1)


def test_gpu_gradients_match_cpu():
    gpu = Transformer(_cfg()).build("cuda", seed=11)
    cpu = Transformer(_cfg()).build("cpu", seed=11)
    cpu.store.flat.copy_(gpu.store.flat_compute.float().cpu())  # the GPU's bf16-rounded weights
    src, tgt = SyntheticPairs(B, L, L + 1, SRC_V, TGT_V, seed=3, min_len=5).batch(0)
    outs = []
    for m, dev in ((gpu, "cuda"), (cpu, "cpu")):
        rt = RunCtx(training=True, dropout=0.0, attn_dropout=0.1, seed=99,
                    ctr=torch.tensor([2], dtype=torch.int64, device=dev), store=m.store)
        outs.append(m.loss_and_backward(src.to(dev), tgt.to(dev), rt, workers=1.0).cpu())
    rel = lambda a, b: ((a.float().cpu() - b.float()).norm() / (b.float().norm() + 1e-12)).item()
    errs = {p_g.name: rel(p_g.grad, p_c.grad) for p_g, p_c in zip(gpu.store.params, cpu.store.params)}
    worst, med = max(errs, key=errs.get), sorted(errs.values())[len(errs) // 2]
    print(f"loss {outs[0][0].item()} {outs[1][0].item()} worst {worst} {errs[worst]:.3e} median {med:.3e}")
    assert abs(outs[0][0] - outs[1][0]) < 2e-2 * abs(outs[1][0])
    assert errs[worst] < 0.2 and med < 0.08, f"{worst}: rel grad err {errs[worst]:.3e}, median {med:.3e}"
    plain = cpu.loss_and_backward(src, tgt, RunCtx(training=True, dropout=0.0, store=cpu.store), workers=1.0)
    assert plain[0] != outs[1][0]  # (the reference did drop)


def test_captured_step_draws_fresh_masks():
    """lr = 0: the weights stay, so the replays of one batch differ by their
    masks alone; the counter put back gives the first loss again, bitwise."""
    m = Transformer(_cfg()).build("cuda", seed=1)
    step = TrainStep(m, Adam(m.store, m.cfg.d_model, lr=0.0), None, workers=1, seed=5)
    assert step.rt.attn_dropout == 0.1
    batch = tuple(t.cuda() for t in SyntheticPairs(B, L, L + 1, SRC_V, TGT_V, seed=3, min_len=5).batch(0))
    assert step.capture(*batch)
    ctr0 = step.rt.ctr.clone()
    losses = []
    for reset in (False, False, True):
        if reset:
            step.rt.ctr.copy_(ctr0)
        step.update([batch])
        losses.append(step.last.clone())
    torch.cuda.synchronize()
    assert not torch.equal(losses[0], losses[1]) and torch.equal(losses[0], losses[2])
