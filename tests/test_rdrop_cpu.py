"""R-Drop on the CPU: the f32 definition (ops.kernels.loss.rdrop_rows, what
cpu_head runs) against float64 autograd of the written objective, the
settings check, the refusals and the training log."""
import json

import pytest
import torch

import ref_rdrop as D
from tensorflow_distributed_on_gke_amd.config import Settings, check_rdrop, load_settings
from tensorflow_distributed_on_gke_amd.models.transformer import Transformer, model_config
from tensorflow_distributed_on_gke_amd.ops.kernels.loss import xent_rdrop
from tensorflow_distributed_on_gke_amd.parallel.dist import DistInfo
from tensorflow_distributed_on_gke_amd.train.distill import Teacher
from tensorflow_distributed_on_gke_amd.train.loop import Trainer
from tensorflow_distributed_on_gke_amd.train.optim import Adam
from tensorflow_distributed_on_gke_amd.train.step import TrainStep


@pytest.mark.parametrize("alpha,smoothing,workers", [(1.0, 0.0, 1.0), (5.0, 0.1, 2.0)])
def test_cpu_gradient_is_autograd_of_the_objective(alpha, smoothing, workers):
    """NLL_1 + NLL_2 + (alpha / 2)(KL(p||r) + KL(r||p)) over ntok * workers,
    differentiated by float64 autograd, against the CPU arm of xent_rdrop."""
    V, ldl = 250, 256
    lg2, lab2 = D.pair_rows(V, ldl)
    M = lg2.shape[0] // 2
    x = lg2[:, :V].double().requires_grad_(True)
    lab, valid = lab2[:M], (lab2[:M] != 0).double()
    ntok = 2.0 * float(valid.sum())
    la, lb = torch.log_softmax(x[:M], -1), torch.log_softmax(x[M:], -1)
    s = D.R._f32r(smoothing)  # what the kernel and the reference get
    hard = torch.nn.functional.one_hot(lab, V).double() * (1 - s) + s / V
    kl = (la.exp() * (la - lb)).sum(-1) + (lb.exp() * (lb - la)).sum(-1)
    obj = ((-(hard * (la + lb)).sum(-1) + 0.5 * alpha * kl) * valid).sum() / (ntok * workers)
    obj.backward()
    ref = D.ref_rdrop(lg2[:, :V], lab2, workers, smoothing, alpha)
    assert float((ref[4] - x.grad).abs().max()) < 1e-12  # the reference's formulas are that gradient
    assert abs(float(ref[0].sum()) / (ntok * workers) - float(obj.detach())) < 1e-12
    out = lg2.float()
    rl, rb, rc = (torch.empty(2 * M) for _ in range(3))
    xent_rdrop(out, V, lab2, torch.tensor([ntok]), workers, smoothing, alpha, rl, rc, rb)
    D.check((rl, rb, rc, ntok, out), V, ref, lg2, alpha, workers, f"cpu arm a={alpha}")


def test_check_rdrop_and_the_step_refuse():
    assert check_rdrop(0) == 0.0 and check_rdrop(5) == 5.0 and check_rdrop(0.0, "fp8", True) == 0.0
    assert load_settings(None, ["rdrop_alpha=5"]).rdrop_alpha == 5.0 and Settings().rdrop_alpha == 0.0
    for bad in (-1.0, float("inf"), float("nan"), "5", True, None):
        with pytest.raises(ValueError, match="rdrop_alpha"):
            check_rdrop(bad)
    with pytest.raises(ValueError, match="dtype=fp8"):
        load_settings(None, ["rdrop_alpha=1", "dtype=fp8"])
    with pytest.raises(ValueError, match="distill_teacher"):
        load_settings(None, ["rdrop_alpha=1", "distill_teacher=a"])
    cfg = model_config("tiny", src_vocab=300, tgt_vocab=250)
    m, t = (Transformer(cfg).build("cpu", seed=s) for s in (1, 2))
    opt = Adam(m.store, cfg.d_model)
    with pytest.raises(ValueError, match="fp8"):
        TrainStep(m, opt, None, workers=1, fp8_state=object(), rdrop_alpha=1.0)
    with pytest.raises(ValueError, match="distill_teacher"):
        TrainStep(m, opt, None, workers=1, teacher=Teacher([t]), distill_alpha=0.5, rdrop_alpha=1.0)
    with pytest.raises(ValueError, match="rdrop_alpha"):
        TrainStep(m, opt, None, workers=1, rdrop_alpha=-1.0)


def test_cpu_run_logs_label_loss(tmp_path):
    """Two epochs with dropout: the record keeps the objective as the loss and
    adds label_loss below it."""
    s = Settings(preset="tiny", local_batch_size=4, src_len=10, tgt_len=10, src_vocab=300, tgt_vocab=300,
                 steps_per_epoch=3, validation_steps=1, log_every=1, snapshot_every_epochs=0, epochs=2,
                 learning_rate=0.001, dropout=0.1, rdrop_alpha=1.0, temporary_directory=str(tmp_path / "tmp"),
                 storage_root=str(tmp_path / "snap"), metrics_file=str(tmp_path / "m.jsonl"))
    logs = []
    tr = Trainer(s, DistInfo(rank=0, world=1, local_rank=0, device=torch.device("cpu")), log=logs.append)
    tr.fit()
    recs = [json.loads(line) for line in open(s.metrics_file)]
    epochs = [r for r in recs if r["kind"] == "epoch"]
    assert len(epochs) == 2 and all(0 < r["label_loss"] < r["train_loss"] for r in epochs)
    assert all("label_loss" in r for r in recs if r["kind"] == "train")
    assert any("R-Drop: alpha 1.0" in l for l in logs) and any(" label_loss " in l for l in logs)
