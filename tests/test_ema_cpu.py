"""Weight EMA and checkpoint averaging on the CPU path: the settings, the
update against the float64 contract of ref_ema.py (step by step), the skip
rule, the in-place swap, resume, `average`, `test --ema`, the training loop's
EMA line / records / snapshot, and two gloo ranks whose averages must stay
bitwise equal."""
import glob
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import ref_ema
from tensorflow_distributed_on_gke_amd.__main__ import main
from tensorflow_distributed_on_gke_amd.checkpoint import bundle
from tensorflow_distributed_on_gke_amd.config import load_settings
from tensorflow_distributed_on_gke_amd.data.synthetic import SyntheticPairs
from tensorflow_distributed_on_gke_amd.models.transformer import Transformer, model_config
from tensorflow_distributed_on_gke_amd.train.ema import WeightEma
from tensorflow_distributed_on_gke_amd.train.optim import Adam

CFG = dict(src_vocab=60, tgt_vocab=50, dropout=0.0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(seed=1, **kw):
    return Transformer(model_config("tiny", **{**CFG, **kw})).build("cpu", seed=seed)


def _grads(n, steps, scale=0.1, seed=11):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g) * scale for _ in range(steps)]


def _bits(t):
    return t.detach().view(torch.int32)


def _live(store, t):
    """The parameters' elements of a flat buffer (checkpoints do not carry the
    alignment padding between them)."""
    return torch.cat([t[p.offset:p.offset + p.numel] for p in store.params])


# ---------------------------------------------------------------- settings
def test_settings_parse_ema_keys():
    s = load_settings()
    assert s.ema_decay == 0.0 and s.ema_warmup is False and s.ema_eval is True  # off by default
    s = load_settings(overrides=["ema_decay=0.999", "ema_warmup=true", "ema_eval=false"])
    assert s.ema_decay == 0.999 and s.ema_warmup is True and s.ema_eval is False


@pytest.mark.parametrize("bad", ["1.0", "-0.1", "1.5", "nan"])
def test_settings_refuse_out_of_range_decay(bad):
    with pytest.raises(ValueError):
        load_settings(overrides=[f"ema_decay={bad}"])
    m = _model()
    with pytest.raises(ValueError):
        Adam(m.store, m.cfg.d_model, ema_decay=float(bad))
    with pytest.raises(ValueError):
        WeightEma(m.store, float(bad))


def test_adam_has_no_ema_by_default():
    m = _model()
    assert Adam(m.store, m.cfg.d_model).ema is None
    assert Adam(m.store, m.cfg.d_model, ema_decay=0.5).ema is not None


# ---------------------------------------------------------------- the update
@pytest.mark.parametrize("warmup", [False, True], ids=["plain", "warmup"])
def test_cpu_ema_meets_contract_step_by_step(warmup):
    m = _model()
    decay = 0.999
    ema = WeightEma(m.store, decay, warmup=warmup)
    ema.avg.fill_(float("nan"))  # the first update reads nothing of it
    g = torch.Generator().manual_seed(5)
    steps = 12  # past count 9 -> 10, where the warm-up ramp is still below the decay
    for k in range(steps):
        m.store.flat.add_(torch.randn(m.store.total, generator=g) * 0.01)
        before = ema.avg.clone()
        ema.update()
        assert ema.updates == k + 1
        ref_ema.check_one_step(ema.avg, m.store.flat, before, decay, warmup, k, f"cpu step {k}")
        if k == 0:
            assert torch.equal(_bits(ema.avg), _bits(m.store.flat))
    # the ramp really was in force (d_eff < decay), and differs from no warm-up
    assert float(ref_ema.d_eff32(decay, True, 9)) == pytest.approx(10.0 / 19.0)
    assert float(ref_ema.d_eff32(decay, True, 10 ** 6)) == pytest.approx(decay)


def test_cpu_ema_ranges_share_one_count():
    ma, mb = _model(), _model()
    ea, eb = WeightEma(ma.store, 0.9), WeightEma(mb.store, 0.9)
    n = ma.store.total
    cut = (n // 2) // 64 * 64
    for k in range(3):
        for mod in (ma, mb):
            mod.store.flat.mul_(1.01)
        ea.update()
        eb.update(start=0, end=cut, inc_count=False)
        eb.update(start=cut, end=n, inc_count=True)
        assert ea.updates == eb.updates == k + 1
        assert torch.equal(_bits(ea.avg), _bits(eb.avg))


def test_cpu_skipped_step_leaves_ema_and_count():
    m = _model()
    n = m.store.total
    g1, g2, g3 = _grads(n, 3)
    opt = Adam(m.store, m.cfg.d_model, lr=0.01, skip_nonfinite=True, ema_decay=0.9)
    m.store.flat_grad.copy_(g1)
    opt.apply()
    assert opt.ema.updates == 1 and torch.equal(_bits(opt.ema.avg), _bits(m.store.flat))
    before = opt.ema.avg.clone()
    g2[n // 3] = float("inf")
    m.store.flat_grad.copy_(g2)
    opt.apply()
    assert opt.iterations == 1 and opt.clip_counters()["skipped_steps"] == 1
    assert opt.ema.updates == 1 and torch.equal(_bits(opt.ema.avg), _bits(before))
    m.store.flat_grad.copy_(g3)
    opt.apply()
    assert opt.iterations == 2 and opt.ema.updates == 2
    ref_ema.check_one_step(opt.ema.avg, m.store.flat, before, 0.9, False, 1, "after the skipped step")


def test_cpu_ema_in_data_parallel_ranges_updates_once():
    """apply_range per span + advance_step (the data-parallel form) does not
    update the EMA by itself: DataParallel.finish() does, once."""
    m = _model()
    n = m.store.total
    opt = Adam(m.store, m.cfg.d_model, lr=0.01, ema_decay=0.9)
    m.store.flat_grad.copy_(_grads(n, 1)[0])
    cut = (n // 2) // 64 * 64
    opt.apply_range(0, cut, inc_step=False)
    opt.apply_range(cut, n, inc_step=False)
    opt.advance_step()
    assert opt.ema.updates == 0
    opt.update_ema()
    assert opt.ema.updates == 1 and torch.equal(_bits(opt.ema.avg), _bits(m.store.flat))


# ---------------------------------------------------------------- swap
def test_swapped_restores_bitwise_and_refuses_updates():
    m = _model()
    n = m.store.total
    opt = Adam(m.store, m.cfg.d_model, lr=0.01, ema_decay=0.5)
    with pytest.raises(RuntimeError):
        with opt.ema.swapped():  # nothing averaged yet
            pass
    for g in _grads(n, 2):
        m.store.flat_grad.copy_(g)
        opt.apply()
    flat, avg = m.store.flat.clone(), opt.ema.avg.clone()
    assert not torch.equal(flat, avg)
    ptr = (m.store.flat.data_ptr(), opt.ema.avg.data_ptr())
    with opt.ema.swapped():
        assert torch.equal(_bits(m.store.flat), _bits(avg)) and torch.equal(_bits(opt.ema.avg), _bits(flat))
        assert ptr == (m.store.flat.data_ptr(), opt.ema.avg.data_ptr())  # contents move, not buffers
        with pytest.raises(RuntimeError, match="swapped"):
            opt.ema.update()
        with pytest.raises(RuntimeError, match="swapped"):
            opt.apply()
        with pytest.raises(RuntimeError, match="swapped"):
            opt.apply_range(0, n)
    assert torch.equal(_bits(m.store.flat), _bits(flat)) and torch.equal(_bits(opt.ema.avg), _bits(avg))
    assert opt.ema.updates == 2 and opt.iterations == 2
    # an exception inside still exchanges back
    with pytest.raises(KeyError):
        with opt.ema.swapped():
            raise KeyError("x")
    assert torch.equal(_bits(m.store.flat), _bits(flat)) and not opt.ema.in_swap
    opt.ema.update()


# ---------------------------------------------------------------- resume
def test_resume_round_trips_ema_and_count(tmp_path):
    m = _model()
    n = m.store.total
    opt = Adam(m.store, m.cfg.d_model, lr=0.01, ema_decay=0.9)
    for g in _grads(n, 3):
        m.store.flat_grad.copy_(g)
        opt.apply()
    prefix = str(tmp_path / "resume" / "model_weights")
    bundle.save_weights(m.store, prefix)
    bundle.save_training_state(m.store, opt, prefix, {"epoch": 2})
    keys = set(bundle.read_bundle(prefix + "_optimizer"))
    wkeys = set(bundle.read_bundle(prefix))
    assert {"ema/" + k for k in wkeys} <= keys and "training_state/ema_updates" in keys

    m2 = _model(seed=7)
    o2 = Adam(m2.store, m2.cfg.d_model, lr=0.01, ema_decay=0.9)
    bundle.load_weights(m2.store, prefix)
    extra = bundle.load_training_state(m2.store, o2, prefix)
    assert extra["epoch"] == 2 and extra["ema_updates"] == 3
    assert o2.ema.updates == 3 and o2.iterations == 3
    assert torch.equal(_bits(_live(m.store, o2.ema.avg)), _bits(_live(m.store, opt.ema.avg)))
    assert torch.equal(_bits(_live(m.store, o2.m)), _bits(_live(m.store, opt.m)))

    # EMA entries in the state, EMA off: ignored
    o3 = Adam(m2.store, m2.cfg.d_model, lr=0.01)
    bundle.load_training_state(m2.store, o3, prefix)
    assert o3.ema is None and o3.iterations == 3

    # a state written without an EMA: count 0, so the first update copies
    plain = str(tmp_path / "plain" / "model_weights")
    bundle.save_training_state(m2.store, o3, plain, {"epoch": 1})
    assert not any(k.startswith("ema/") for k in bundle.read_bundle(plain + "_optimizer"))
    extra = bundle.load_training_state(m2.store, o2, plain)
    assert "ema_updates" not in extra and o2.ema.updates == 0
    o2.ema.avg.fill_(float("nan"))
    o2.ema.update()
    assert torch.equal(_bits(o2.ema.avg), _bits(m2.store.flat))


# ---------------------------------------------------------------- average
def test_average_of_three_bundles_is_the_float64_mean(tmp_path, capsys):
    prefixes, tens = [], []
    for i in range(3):
        m = _model(seed=20 + i)
        p = str(tmp_path / f"w{i}" / "model_weights")
        bundle.save_weights(m.store, p)
        prefixes.append(p)
        tens.append(bundle.read_bundle(p))
    out = str(tmp_path / "avg" / "model_weights")
    assert main(["average", "--inputs", *prefixes, "--output", out]) == 0
    got = bundle.read_bundle(out)
    assert list(got) == list(tens[0]) and len(got) > 10  # same keys, same order
    assert list(bundle.bundle_entries(out)) == list(bundle.bundle_entries(prefixes[0]))
    for k, a in got.items():
        want = ((tens[0][k].astype(np.float64) + tens[1][k] + tens[2][k]) / 3).astype(np.float32)
        assert a.dtype == np.float32 and np.array_equal(a, want), k
    # loadable: by the model, and through a snapshot directory as an input
    m = _model(seed=3)
    assert bundle.load_weights(m.store, out) == []
    assert main(["average", "--inputs", str(tmp_path / "w0"), prefixes[1], "--output",
                 str(tmp_path / "avg2" / "model_weights")]) == 0


def test_average_refuses_mismatched_bundles(tmp_path):
    a, b, c = (str(tmp_path / x / "model_weights") for x in "abc")
    m = _model()
    bundle.save_weights(m.store, a)
    t = bundle.read_bundle(a)
    k0 = next(iter(t))
    bundle.write_bundle(b, {k: v for k, v in t.items() if k != k0})  # a key missing
    with pytest.raises(ValueError, match="different keys"):
        main(["average", "--inputs", a, b, "--output", str(tmp_path / "o" / "w")])
    bundle.save_weights(_model(src_vocab=61).store, c)  # another embedding shape
    with pytest.raises(ValueError, match="float32"):
        main(["average", "--inputs", a, c, "--output", str(tmp_path / "o" / "w")])
    assert not os.path.exists(str(tmp_path / "o" / "w") + ".index")


# ---------------------------------------------------------------- test --ema
TEST_SETS = ["preset=tiny", "src_vocab=300", "tgt_vocab=300", "max_len=64"]


def _test_cli(*args):
    argv = ["test", "--config", os.path.join(ROOT, "configuration", "settings.yaml"), "--device", "cpu",
            "--max-length", "6", "--sentence", "olá"]
    for kv in TEST_SETS:
        argv += ["--set", kv]
    return main(argv + list(args))


def test_test_ema_loads_the_ema_bundle_and_errors_without(tmp_path, monkeypatch, capsys):
    s = load_settings(overrides=TEST_SETS)
    from tensorflow_distributed_on_gke_amd.train.loop import build_model
    m = build_model(s, "cpu")
    ema = WeightEma(m.store, 0.5)
    ema.update()
    ema.avg.mul_(0.5)  # (an average that differs from the weights)
    prefix = str(tmp_path / "snap" / "model_weights")
    bundle.save_weights(m.store, prefix)

    with pytest.raises(FileNotFoundError, match="model_weights_ema"):
        _test_cli("--weights", prefix, "--ema")

    assert bundle.save_ema_weights(m.store, ema, prefix) == prefix + "_ema"
    assert list(bundle.read_bundle(prefix + "_ema")) == list(bundle.read_bundle(prefix))
    # the directory's state file still names the raw weights
    assert bundle.resolve_prefix(str(tmp_path / "snap")) == prefix
    loaded = []
    real = bundle.load_weights

    def spy(store, p, *a, **kw):
        r = real(store, p, *a, **kw)
        loaded.append((p, store.flat.clone()))
        return r

    monkeypatch.setattr(bundle, "load_weights", spy)
    assert _test_cli("--weights", prefix, "--ema") == 0
    assert _test_cli("--weights", str(tmp_path / "snap"), "--ema") == 0  # directory form
    assert _test_cli("--weights", prefix) == 0
    assert [p for p, _ in loaded] == [prefix + "_ema", prefix + "_ema", prefix]
    assert torch.equal(_live(m.store, loaded[0][1]), _live(m.store, m.store.flat) * 0.5)
    assert "->" in capsys.readouterr().out


# ---------------------------------------------------------------- training loop
def _train_cli(tmp, *sets):
    mf = os.path.join(tmp, "metrics.jsonl")
    cmd = [sys.executable, "-m", "tensorflow_distributed_on_gke_amd", "train", "--config",
           os.path.join(ROOT, "configuration", "settings.yaml"), "--device", "cpu"]
    for kv in ["preset=tiny", "steps_per_epoch=3", "log_every=50", "local_batch_size=2", "src_len=8",
               "tgt_len=8", "src_vocab=300", "tgt_vocab=300", "max_len=64", "snapshot_every_epochs=1",
               "validation_steps=1", "epochs=1", f"metrics_file={mf}", *sets]:
        cmd += ["--set", kv]
    r = subprocess.run(cmd, cwd=tmp, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(mf) as f:
        return r.stdout, [json.loads(line) for line in f]


def test_train_logs_ema_line_writes_ema_snapshot_and_decodes_from_it(tmp_path, capsys):
    (tmp_path / "off").mkdir()
    (tmp_path / "on").mkdir()
    out_off, off = _train_cli(str(tmp_path / "off"))
    out_on, on = _train_cli(str(tmp_path / "on"), "ema_decay=0.999")
    extra = {"ema_test_loss", "ema_test_acc"}
    eo, en = off[-1], on[-1]
    assert eo["kind"] == en["kind"] == "epoch"
    assert not extra & set(eo) and set(en) == set(eo) | extra
    for a, b in zip(off, on):  # the run itself is the same with the EMA on
        assert all(b[k] == a[k] for k in ("train_loss", "test_loss") if k in a)
    # the reference's epoch line is unchanged; the EMA line follows it
    ref_lines = [ln for ln in out_on.splitlines() if ln.startswith("Epoch 1 Loss")]
    assert ref_lines == [ln for ln in out_off.splitlines() if ln.startswith("Epoch 1 Loss")] and ref_lines
    ema_lines = [ln for ln in out_on.splitlines() if ln.startswith("EMA Test Loss")]
    assert ema_lines == [f"EMA Test Loss {en['ema_test_loss']:.4f} Test Accuracy {en['ema_test_acc']:.4f}"]
    assert "EMA" not in out_off
    # after 3 steps at decay 0.999 the average is nearly the first step's weights
    assert en["ema_test_loss"] != en["test_loss"]
    assert not glob.glob(str(tmp_path / "off" / "**" / "model_weights_ema.index"), recursive=True)
    found = glob.glob(str(tmp_path / "on" / "snapshots" / "**" / "model_weights_ema.index"), recursive=True)
    assert len(found) == 1
    prefix = found[0][:-len("_ema.index")]
    raw, avg = bundle.read_bundle(prefix), bundle.read_bundle(prefix + "_ema")
    assert list(raw) == list(avg) and len(raw) == len(bundle.read_bundle(prefix + "_ema"))
    assert any(not np.array_equal(raw[k], avg[k]) for k in raw)
    # resume state: the EMA travels with the optimizer slots
    st = bundle.read_bundle(str(tmp_path / "on" / "temporary" / "resume" / "model_weights_optimizer"))
    assert int(st["training_state/ema_updates"].item()) == 3
    assert _test_cli("--weights", prefix, "--ema") == 0
    assert "->" in capsys.readouterr().out


# ---------------------------------------------------------------- two gloo ranks
STEPS = 3
DECAY = 0.9


def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    torch.set_num_threads(2)
    from tensorflow_distributed_on_gke_amd.parallel import dist as tdist
    from tensorflow_distributed_on_gke_amd.parallel.ddp import DataParallel
    from tensorflow_distributed_on_gke_amd.train.step import TrainStep

    tdist.init_distributed("cpu")
    m = Transformer(model_config("tiny", **CFG)).build("cpu", seed=1 + rank)
    opt = Adam(m.store, m.cfg.d_model, lr=0.05, eps=1.0, ema_decay=DECAY, ema_warmup=True)
    ddp = DataParallel(m.store, bucket_mb=0.05)
    ddp.broadcast_params(0)
    step = TrainStep(m, opt, ddp, workers=world, seed=5)
    assert ddp.opt is opt and ddp.ema is opt.ema
    data = SyntheticPairs(4, 10, 11, 60, 50, seed=3, rank=rank, world=world, min_len=3)
    for i in range(STEPS):
        before = opt.ema.avg.clone()
        step(*data.batch(i))
        ddp.verify_replicas()
        assert opt.ema.updates == i + 1 == opt.iterations
        ref_ema.check_one_step(opt.ema.avg, m.store.flat, before, DECAY, True, i, f"rank {rank} step {i}")
    res = {"avg": opt.ema.avg.clone(), "flat": m.store.flat.clone(), "count": opt.ema.updates,
           "nb": len(ddp.last_buckets)}
    # one rank's average perturbed by one bit: every rank sees the divergence
    if rank == 1:
        _bits(opt.ema.avg)[m.store.total // 2] ^= 1
    try:
        ddp.verify_replicas()
        res["raised"] = ""
    except RuntimeError as e:
        res["raised"] = str(e)
    torch.save(res, f"{out}.{rank}")
    ddp.close()
    tdist.barrier()
    tdist.shutdown()


def test_dp2_ema_replicas_identical_and_divergence_detected(tmp_path):
    world = 2
    out = str(tmp_path / "res")
    mp.start_processes(_worker, args=(world, _free_port(), out), nprocs=world, join=True,
                       start_method="spawn")
    r0 = torch.load(out + ".0", weights_only=True)
    r1 = torch.load(out + ".1", weights_only=True)
    assert r0["nb"] > 3  # several spans, each with its own Adam range
    assert torch.equal(_bits(r0["avg"]), _bits(r1["avg"])) and torch.equal(r0["flat"], r1["flat"])
    assert r0["count"] == r1["count"] == STEPS
    assert not torch.equal(r0["avg"], r0["flat"])
    assert "replica divergence" in r0["raised"] and "replica divergence" in r1["raised"]
