"""Distillation end to end through the command line on the CPU: `train --set
distill_teacher=A,B` trains, logs `label_loss`, and leaves a checkpoint that
`test --weights` loads as an ordinary single model; bad settings are refused
before any training."""
import json
import os
import subprocess
import sys

import pytest
import torch

from tensorflow_distributed_on_gke_amd.__main__ import main
from tensorflow_distributed_on_gke_amd.checkpoint import bundle
from tensorflow_distributed_on_gke_amd.config import load_settings
from tensorflow_distributed_on_gke_amd.train.loop import RESUME_DIR, RESUME_PREFIX, build_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = os.path.join(ROOT, "configuration", "settings.yaml")
MODEL_SETS = ["preset=tiny", "src_vocab=300", "tgt_vocab=300", "max_len=64"]


@pytest.fixture(scope="module")
def teachers(tmp_path_factory):
    d = tmp_path_factory.mktemp("teachers")
    m = build_model(load_settings(overrides=MODEL_SETS), "cpu")
    a, b = str(d / "a" / "model_weights"), str(d / "b")
    bundle.save_weights(m.store, a)
    g = torch.Generator().manual_seed(0)
    m.store.flat.add_(torch.randn(m.store.flat.shape, generator=g) * 0.05)
    bundle.save_weights(m.store, os.path.join(b, "model_weights"))
    return a, b  # a prefix and a snapshot directory, as warm_start takes them


def _train(tmp, *sets):
    cmd = [sys.executable, "-m", "tensorflow_distributed_on_gke_amd", "train", "--config", CONFIG,
           "--nproc", "1", "--device", "cpu"]
    base = MODEL_SETS + ["steps_per_epoch=3", "log_every=1", "local_batch_size=4", "src_len=10", "tgt_len=10",
                         "snapshot_every_epochs=0", "dropout=0", "validation_steps=1", "learning_rate=0.001",
                         "worker_count=1", "metrics_file=m.jsonl", "epochs=1", "label_smoothing=0.1",
                         f"temporary_directory={tmp}/tmp"]
    for kv in base + list(sets):
        cmd += ["--set", kv]
    env = dict(os.environ, PYTHONPATH=ROOT)
    env.pop("RANK", None)
    return subprocess.run(cmd, cwd=tmp, env=env, capture_output=True, text=True, timeout=300)


def test_train_cli_distills_and_the_checkpoint_is_a_single_model(teachers, tmp_path, capsys):
    a, b = teachers
    r = _train(tmp_path, f"distill_teacher={a},{b}", "distill_weights=2,1", "distill_alpha=0.5")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "distillation: 2 teacher(s)" in r.stdout and "alpha 0.5" in r.stdout
    assert "Epoch 1 Batch 2 " in r.stdout and "label_loss" in r.stdout
    recs = [json.loads(line) for line in open(tmp_path / "m.jsonl")]
    epoch = [x for x in recs if x["kind"] == "epoch"]
    assert len(epoch) == 1 and epoch[0]["label_loss"] > 0
    assert abs(epoch[0]["label_loss"] - epoch[0]["train_loss"]) > 1e-4  # the objective is another number
    assert all("label_loss" in x for x in recs if x["kind"] == "train")
    # a plain run logs no label_loss, and its validation loss is the same kind of number
    plain = tmp_path / "plain"
    plain.mkdir()
    r0 = _train(plain)
    assert r0.returncode == 0, r0.stdout + r0.stderr
    assert "label_loss" not in r0.stdout
    assert all("label_loss" not in json.loads(line) for line in open(plain / "m.jsonl"))
    # the student's checkpoint is an ordinary single model
    prefix = str(tmp_path / "tmp" / RESUME_DIR / RESUME_PREFIX)
    argv = ["test", "--config", CONFIG, "--device", "cpu", "--max-length", "6"]
    for kv in MODEL_SETS:
        argv += ["--set", kv]
    assert main(argv + ["--weights", prefix, "--sentence", "olá"]) == 0
    assert "->" in capsys.readouterr().out


@pytest.mark.parametrize("sets,msg", [(("distill_weights=1,2",), "without distill_teacher"),
                                      (("distill_teacher=a,b", "distill_weights=1"), "1 values for 2 teachers"),
                                      (("distill_teacher=a", "distill_alpha=1.5"), "(0, 1]"),
                                      (("distill_teacher=a", "dtype=fp8"), "dtype=fp8")])
def test_train_cli_refuses_bad_distill_settings(tmp_path, sets, msg):
    r = _train(tmp_path, *sets)
    assert r.returncode != 0 and msg in r.stderr, r.stdout + r.stderr
    assert "Epoch 1" not in r.stdout
