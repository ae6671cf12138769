"""Gradient accumulation on CPU (accum_steps = N micro-batches per optimizer
update, train/step.py TrainStep.update).

A micro-batch is one more replica: an update of W ranks x N micro-batches
must be the update one process computes for W * N replicas with the project's
own accumulate idiom (tests/test_parallel_cpu.py: sequential
loss_and_backward(accumulate=r > 0) calls and one opt.apply()). Tolerances are
that file's: weights atol 1e-6 / rtol 1e-5, losses atol 1e-6."""
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.multiprocessing as mp

import ref_accum
from test_parallel_cpu import ADAM, CFG, STEPS, _data, _fill, _free_port, _single_process_reference

from tensorflow_distributed_on_gke_amd.config import Settings, load_settings
from tensorflow_distributed_on_gke_amd.data.synthetic import SyntheticPairs
from tensorflow_distributed_on_gke_amd.models.layers import RunCtx
from tensorflow_distributed_on_gke_amd.models.transformer import Transformer, model_config
from tensorflow_distributed_on_gke_amd.train.optim import Adam
from tensorflow_distributed_on_gke_amd.train.step import TrainStep, micro_positions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = dict(atol=1e-6, rtol=1e-5)


def _build(seed=1):
    m = Transformer(model_config("tiny", **CFG)).build("cpu", seed=seed)
    return m, Adam(m.store, m.cfg.d_model, **ADAM)


def _labels(tgt) -> int:
    return int((tgt[:, 1:] != 0).sum())


def _run_updates(updates, accum_steps, loss_mode):
    """TrainStep on one rank over `updates` (lists of micro-batches): final
    weights and each update's loss (the growth of the metric accumulator)."""
    m, opt = _build()
    step = TrainStep(m, opt, None, workers=1, seed=5, loss_mode=loss_mode, accum_steps=accum_steps)
    losses = []
    for mbs in updates:
        before = step.accum.clone()
        step.update(mbs)
        d = step.accum - before
        assert d[2] == len(mbs)  # one metric record per micro-batch
        losses.append(d[0].clone())
    assert opt.iterations == len(updates)
    return m.store.flat.clone(), torch.stack(losses), step


def _reference_losses(world, global_mean=False):
    """The accumulate idiom of test_parallel_cpu._single_process_reference,
    keeping every replica's loss share: their sum is the update's loss."""
    m, opt = _build()
    datas = [_data(r, world) for r in range(world)]
    out = []
    for i in range(STEPS):
        n_all = float(sum(_labels(datas[r].batch(i)[1]) for r in range(world)))
        tot = 0.0
        for r in range(world):
            rt = RunCtx(training=True, dropout=0.0, seed=5, ctr=torch.zeros(1, dtype=torch.int64),
                        accumulate=r > 0)
            if global_mean:
                o = m.loss_and_backward(*datas[r].batch(i), rt, 1.0, ntok_sum=_fill(n_all))
            else:
                o = m.loss_and_backward(*datas[r].batch(i), rt, float(world))
            tot = tot + o[0].clone()
        out.append(tot)
        opt.apply()
    return m.store.flat, torch.stack(out)


def test_micro_positions():
    assert micro_positions(1) == ["only"]
    assert micro_positions(2) == ["first", "last"]
    assert micro_positions(4) == ["first", "middle", "middle", "last"]


def test_one_rank_four_micro_batches_match_four_replicas():
    datas = [_data(r, 4) for r in range(4)]
    updates = [[datas[r].batch(i) for r in range(4)] for i in range(STEPS)]
    flat, losses, step = _run_updates(updates, 4, "replica_mean")
    assert not step.global_mean and step.workers == 4.0
    ref_flat, _ = _single_process_reference(4)
    assert not torch.equal(flat, _build()[0].store.flat)
    assert torch.allclose(flat, ref_flat, **TOL)
    ref_flat2, ref_loss = _reference_losses(4)
    assert torch.equal(ref_flat, ref_flat2)  # the same idiom, all shares kept
    assert torch.allclose(losses, ref_loss, atol=1e-6)


def test_one_rank_global_mean_equals_the_whole_batch():
    """N = 4 micro-batches of 2 sentences under global_mean = one batch of the
    same 8 sentences; with unequal label counts replica_mean is another update."""
    data = SyntheticPairs(8, 10, 11, 60, 50, seed=3, min_len=3)
    whole = [data.batch(i) for i in range(STEPS)]
    split = [[(s[2 * k:2 * k + 2].contiguous(), t[2 * k:2 * k + 2].contiguous()) for k in range(4)]
             for s, t in whole]
    assert all(len({_labels(t) for _, t in mbs}) > 1 for mbs in split), "label counts must differ"
    flat_g, loss_g, step = _run_updates(split, 4, "global_mean")
    assert step.global_mean and step.workers == 1.0  # live on a single rank
    flat_1, loss_1, one = _run_updates([[b] for b in whole], 1, "global_mean")
    assert not one.global_mean
    assert torch.allclose(flat_g, flat_1, **TOL)
    assert torch.allclose(loss_g, loss_1, atol=1e-6)
    flat_r, _, _ = _run_updates(split, 4, "replica_mean")
    assert not torch.allclose(flat_r, flat_g, **TOL)  # the modes differ


def test_update_takes_exactly_accum_steps_micro_batches():
    m, opt = _build()
    step = TrainStep(m, opt, None, workers=1, accum_steps=2)
    b = _data(0, 1).batch(0)
    with pytest.raises(ValueError, match="accum_steps=2"):
        step.update([b])
    with pytest.raises(ValueError, match="update"):
        step(*b)
    with pytest.raises(ValueError):
        TrainStep(m, opt, None, workers=1, accum_steps=0)
    with pytest.raises(ValueError):
        TrainStep(m, opt, None, workers=1, accum_steps=33)


def test_cpu_label_total_is_the_reference_count():
    m, opt = _build()
    step = TrainStep(m, opt, None, workers=1, loss_mode="global_mean", accum_steps=3)
    mbs = [_data(r, 3).batch(0) for r in range(3)]
    step._begin_update(mbs)
    total, counts = ref_accum.count_labels_ref([t for _, t in mbs])
    assert torch.equal(step._ntok_total, total)
    assert int(counts.sum()) == sum(_labels(t) for _, t in mbs)
    t = torch.tensor([[5, 0, 3, 0], [0, 7, 0, 0]])
    assert ref_accum.count_labels_ref([t, t[:1]])[1].tolist() == [2, 1]  # position 0 is no label


# ------------------------------------------------------------------ two ranks
def _worker(rank, world, port, out, accum, loss_mode):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from tensorflow_distributed_on_gke_amd.train import step as step_mod
    step_mod.DP_OVERLAP_OPT = "tail"
    torch.set_num_threads(2)
    from tensorflow_distributed_on_gke_amd.parallel import dist as tdist
    from tensorflow_distributed_on_gke_amd.parallel.ddp import DataParallel

    tdist.init_distributed("cpu")
    m = Transformer(model_config("tiny", **CFG)).build("cpu", seed=1 + rank)
    opt = Adam(m.store, m.cfg.d_model, **ADAM)
    ddp = DataParallel(m.store, bucket_mb=0.05)
    ddp.broadcast_params(0)
    g = m.store.flat_grad
    lo, hi = g.data_ptr(), g.data_ptr() + g.numel() * 4
    seen = []  # (gradient collective?, issued in the update's last micro-batch?)
    real = ddp.all_reduce_async
    holder = {}

    def spy(t):
        seen.append((lo <= t.data_ptr() < hi, holder["step"].last_micro))
        return real(t)

    ddp.all_reduce_async = spy
    step = holder["step"] = TrainStep(m, opt, ddp, workers=world, seed=5, loss_mode=loss_mode,
                                      accum_steps=accum)
    assert ddp.opt is opt  # per-span Adam at the tail, as in production
    replicas = world * accum
    datas = [_data(r, replicas) for r in range(replicas)]
    spans, early, scalars, losses = [], 0, [], []
    for i in range(STEPS):
        seen.clear()
        before = step.accum.clone()
        # micro-batch k of rank r is replica r * accum + k of the reference
        step.update([datas[rank * accum + k].batch(i) for k in range(accum)])
        ddp.verify_replicas()  # bitwise equal after every update
        spans.append(sum(1 for grad, _ in seen if grad))
        early += sum(1 for grad, last in seen if grad and not last)
        scalars.append(sum(1 for grad, _ in seen if not grad))
        losses.append((step.accum - before)[0].clone())
        assert len(ddp.last_buckets) == spans[-1]
    assert opt.iterations == STEPS
    torch.save({"flat": m.store.flat.clone(), "spans": spans, "early": early, "scalars": scalars,
                "loss": torch.stack(losses)}, f"{out}.{rank}")
    ddp.close()
    tdist.barrier()
    tdist.shutdown()


def _spawn(tmp_path, name, accum, loss_mode):
    out = str(tmp_path / name)
    mp.start_processes(_worker, args=(2, _free_port(), out, accum, loss_mode), nprocs=2, join=True,
                       start_method="spawn")
    return [torch.load(f"{out}.{r}", weights_only=True) for r in range(2)]


@pytest.mark.parametrize("loss_mode", ["replica_mean", "global_mean"])
def test_two_ranks_two_micro_batches_match_four_replicas(tmp_path, loss_mode):
    r0, r1 = _spawn(tmp_path, "acc", 2, loss_mode)
    assert torch.equal(r0["flat"], r1["flat"])
    gm = loss_mode == "global_mean"
    ref_flat, _ = _single_process_reference(4, global_mean=gm)
    assert torch.allclose(r0["flat"], ref_flat, **TOL)
    _, ref_loss = _reference_losses(4, global_mean=gm)
    # (each rank holds its own two replicas' shares)
    assert torch.allclose(r0["loss"] + r1["loss"], ref_loss, atol=1e-6)
    # no gradient collective before the last micro-batch; as many spans per
    # update as a plain step issues
    assert r0["early"] == 0 and r1["early"] == 0
    b0, _ = _spawn(tmp_path, "plain", 1, loss_mode)
    assert r0["spans"] == b0["spans"] and min(r0["spans"]) > 3
    # the label-count all-reduce: once per update, on the update's total
    assert r0["scalars"] == [1 if gm else 0] * STEPS


# ------------------------------------------------------------------ settings, loop, CLI
def test_accum_steps_setting_is_validated():
    assert Settings().accum_steps == 1
    assert load_settings(None, ["accum_steps=1"]).accum_steps == 1
    assert load_settings(None, ["accum_steps=32"]).accum_steps == 32
    for bad in ("0", "-1", "33", "2.5", "two"):
        with pytest.raises(ValueError):
            load_settings(None, [f"accum_steps={bad}"])
    with pytest.raises(ValueError, match="fp8"):
        load_settings(None, ["accum_steps=2", "dtype=fp8"])
    assert load_settings(None, ["accum_steps=1", "dtype=fp8"]).dtype == "fp8"


def _trainer(tmp_path, **kw):
    from tensorflow_distributed_on_gke_amd.parallel.dist import DistInfo
    from tensorflow_distributed_on_gke_amd.train.loop import Trainer
    s = Settings(preset="tiny", local_batch_size=4, src_len=10, tgt_len=10, src_vocab=300, tgt_vocab=300,
                 steps_per_epoch=7, validation_steps=1, log_every=1, snapshot_every_epochs=0,
                 learning_rate=0.001, dropout=0.0, temporary_directory=str(tmp_path / "tmp"),
                 storage_root=str(tmp_path / "snap"), **kw)
    logs = []
    tr = Trainer(s, DistInfo(rank=0, world=1, local_rank=0, device=torch.device("cpu")), log=logs.append)
    taken = []
    nxt = tr.train_data.next

    def spy(out=None):
        taken.append(tr.train_data._next)
        return nxt(out)

    tr.train_data.next = spy
    return tr, taken, logs


def test_loop_data_order_counts_and_resume(tmp_path):
    """steps_per_epoch = 7 batches, N = 3: two updates per epoch from batches
    0-5 of the epoch, the 7th skipped, the next epoch at its own first batch;
    steps count updates; a resumed run continues at the data position of the
    restored update count."""
    tr, taken, logs = _trainer(tmp_path, accum_steps=3, epochs=2)
    tr.fit()
    assert taken == [0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12]
    assert tr.opt.iterations == 4 and tr.global_step == 4
    assert sum(1 for line in logs if " Batch " in line) == 4
    assert not any(" Batch 2 " in line for line in logs)
    tr2, taken2, logs2 = _trainer(tmp_path, accum_steps=3, epochs=3)
    tr2.fit()
    assert any("Resuming from" in line and "at epoch 3, iteration 4" in line for line in logs2), logs2
    assert taken2 == [14, 15, 16, 17, 18, 19]
    assert tr2.opt.iterations == 6 and tr2.global_step == 6
    # N = 1 walks every batch, as before
    tr1, taken1, _ = _trainer(tmp_path / "plain", epochs=2)
    tr1.fit()
    assert taken1 == list(range(14)) and tr1.opt.iterations == 14


def test_backward_fault_fires_in_the_last_micro_batch(tmp_path, monkeypatch):
    """kill_point=backward with N = 2: the injected exit comes in the backward
    of update kill_at_step's LAST micro-batch (the one with collectives)."""
    from tensorflow_distributed_on_gke_amd.train import loop as loop_mod
    tr, taken, logs = _trainer(tmp_path, accum_steps=2, epochs=1, kill_at_step=2, kill_point="backward",
                               kill_rank=0, resume=False)
    seen = []

    class _Exit(Exception):
        pass

    def fake_exit(code):
        seen.append((code, tr.step_fn.rt.accumulate, tr.step_fn.last_micro, len(taken), tr.global_step))
        raise _Exit()

    monkeypatch.setattr(loop_mod.os, "_exit", fake_exit)
    with pytest.raises(Exception):
        tr.fit()
    # update 2 = batches 2 and 3, both fetched; its second micro-batch accumulates
    assert seen == [(17, True, True, 4, 1)], seen
    assert any("exiting in the backward of step 2" in line for line in logs)


def test_loop_metrics_are_those_of_the_replica_run(tmp_path):
    """The logged loss / accuracy of an N = 3 update are the sum of the
    micro-batches' shares and the mean of their accuracies."""
    tr, _, logs = _trainer(tmp_path, accum_steps=3, epochs=1, metrics_file=str(tmp_path / "m.jsonl"))
    tr.fit()
    recs = [json.loads(line) for line in open(tmp_path / "m.jsonl")]
    train = [r for r in recs if r["kind"] == "train"]
    assert [r["step"] for r in train] == [1, 2] and [r["batch"] for r in train] == [0, 1]
    # the same first update by hand, from the initial weights
    tr0, _, _ = _trainer(tmp_path / "ref", accum_steps=3, epochs=1)
    rt = RunCtx(training=True, dropout=0.0, seed=0, ctr=torch.zeros(1, dtype=torch.int64))
    outs = [tr0.model.loss_and_backward(*tr0.train_data.batch(k), rt, 3.0).clone() for k in range(3)]
    assert train[0]["loss"] == pytest.approx(float(sum(o[0] for o in outs)), abs=1e-6)
    assert train[0]["accuracy"] == pytest.approx(float(sum(o[1] for o in outs)) / 3, abs=1e-6)


def _cli(tmp, *sets):
    cmd = [sys.executable, "-m", "tensorflow_distributed_on_gke_amd", "train", "--config",
           os.path.join(ROOT, "configuration", "settings.yaml"), "--nproc", "1", "--device", "cpu"]
    base = ["preset=tiny", "steps_per_epoch=7", "log_every=1", "local_batch_size=4", "src_len=10",
            "tgt_len=10", "src_vocab=300", "tgt_vocab=300", "snapshot_every_epochs=0", "dropout=0",
            "validation_steps=1", "learning_rate=0.001", "worker_count=1", "metrics_file=m.jsonl"]
    for kv in base + list(sets):
        cmd += ["--set", kv]
    env = dict(os.environ, PYTHONPATH=ROOT)
    env.pop("RANK", None)
    return subprocess.run(cmd, cwd=tmp, env=env, capture_output=True, text=True, timeout=300)


def _epochs(path):
    return [r for r in map(json.loads, open(path)) if r["kind"] == "epoch"]


def test_train_cli_accum_steps(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir()
    b.mkdir()
    r = _cli(a, "accum_steps=3", "epochs=1")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Epoch 1 Batch 1 " in r.stdout and "Epoch 1 Batch 2 " not in r.stdout
    r = _cli(a, "accum_steps=3", "epochs=2")  # resumes after epoch 1
    assert r.returncode == 0, r.stdout + r.stderr
    assert "at epoch 2, iteration 2" in r.stdout  # opt.iterations counts updates
    assert "Epoch 1 Batch" not in r.stdout and "Epoch 2 Batch 1 " in r.stdout
    steps = [x["step"] for x in map(json.loads, open(a / "m.jsonl")) if x["kind"] == "train"]
    assert steps == [1, 2, 3, 4]  # both runs append to one file: updates, not batches
    # the resumed epoch saw the batches an uninterrupted run sees
    r = _cli(b, "accum_steps=3", "epochs=2", "resume=false")
    assert r.returncode == 0, r.stdout + r.stderr
    resumed, straight = _epochs(a / "m.jsonl")[-1], _epochs(b / "m.jsonl")[-1]
    assert resumed["epoch"] == straight["epoch"] == 2
    assert resumed["train_loss"] == pytest.approx(straight["train_loss"], abs=1e-6)
    assert resumed["test_loss"] == pytest.approx(straight["test_loss"], abs=1e-6)


@pytest.mark.parametrize("sets,msg", [(("accum_steps=0",), "accum_steps must be"),
                                      (("accum_steps=2", "dtype=fp8"), "dtype=fp8")])
def test_train_cli_refuses_bad_accum_settings(tmp_path, sets, msg):
    r = _cli(tmp_path, "epochs=1", *sets)
    assert r.returncode != 0 and msg in r.stderr, r.stdout + r.stderr
    assert "Epoch 1" not in r.stdout
