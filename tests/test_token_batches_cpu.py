"""Token-budget text batches on the CPU (data/text.py plan_token_batches /
epoch_token_batches, TextPairs' batch_tokens mode, data/corpus.py on the CPU
device, the batch_tokens / length_bucket settings, and a two-rank gloo epoch).

The plan algorithm is fixed by its specification (sorted length keys walked in
groups of `world` pairs, a batch closed when one more row per rank would
exceed the budget), so the invariants below hold for any input, and the fill
floor on the stated length distribution (0.75; the algorithm gives 0.828 for
world 1 and 0.810 for world 2, fixed-size batches 0.244) only catches a broken
packer."""
import json
import os
import random
import socket

import pytest
import torch
import torch.multiprocessing as mp

from tensorflow_distributed_on_gke_amd.config import Settings, check_batch_tokens, load_settings
from tensorflow_distributed_on_gke_amd.data.corpus import DeviceCorpus
from tensorflow_distributed_on_gke_amd.data.text import (PAD, TextPairs, WordPieceTokenizer, bucket_lengths,
                                                        epoch_token_batches, pad_rows, plan_token_batches,
                                                        read_pairs)

MAX_LEN = 100


def _lengths(n=4000, seed=0):
    r = random.Random(seed)
    src, tgt = [], []
    for _ in range(n):
        k = min(120, int(r.expovariate(1 / 18)) + 2)
        t = max(2, k + r.randint(-3, 3))
        src.append(k + 2)
        tgt.append(t + 2)
    return src, tgt


def _batches(plan, ids):
    return [ids[plan.starts[b]:plan.starts[b] + plan.rows[b]] for b in range(plan.steps_per_epoch)]


@pytest.mark.parametrize("world", [1, 2, 8])
@pytest.mark.parametrize("bucket", [1, 8, 32])
def test_plan_invariants(world, bucket):
    src, tgt = _lengths(1003, seed=world * 100 + bucket)  # 1003: a remainder for world 2 and 8
    budget = 1024
    plan = plan_token_batches(src, tgt, budget, world, bucket, MAX_LEN)
    assert plan.steps_per_epoch == len(plan.rows) > 1
    epochs = [epoch_token_batches(plan, seed=3, epoch=e) for e in range(3)]
    for ids, order in epochs:
        assert sorted(order) == list(range(plan.steps_per_epoch))
        assert len(set(ids)) == len(ids) == plan.used  # each pair at most once
        assert 0 <= len(src) - len(ids) <= world - 1
        for b, g in enumerate(_batches(plan, ids)):
            rows, S, T = plan.rows[b], plan.S[b], plan.T[b]
            rpr = rows // world
            assert len(g) == rows and rows % world == 0 and rpr >= 1
            if rpr > 1:
                assert rpr * (S + T - 1) <= budget
            assert (S, T) == bucket_lengths(max(src[j] for j in g), max(tgt[j] for j in g), bucket, MAX_LEN)
            assert S % bucket == 0 or S == MAX_LEN or S > MAX_LEN
            assert (T - 1) % bucket == 0 or T == MAX_LEN or T > MAX_LEN
            assert all(src[j] <= S and tgt[j] <= T for j in g)
            # rank slices: disjoint, and their union is the global batch
            parts = [ids[slice(*plan.rank_slice(b, r))] for r in range(world)]
            assert all(len(p) == rpr for p in parts)
            assert [j for p in parts for j in p] == g
    # boundaries and shapes are the plan's (one object for all epochs); membership differs
    assert epochs[0][0] != epochs[1][0] and epochs[1][0] != epochs[2][0]
    assert epochs[0][1] != epochs[1][1]
    # seeds
    assert epoch_token_batches(plan, 3, 1) == epochs[1]
    assert epoch_token_batches(plan, 4, 1) != epochs[1]
    # the plan depends on the multiset of keys only
    perm = list(range(len(src)))
    random.Random(1).shuffle(perm)
    p2 = plan_token_batches([src[j] for j in perm], [tgt[j] for j in perm], budget, world, bucket, MAX_LEN)
    assert (p2.starts, p2.rows, p2.S, p2.T) == (plan.starts, plan.rows, plan.S, plan.T)
    # validation data: no shuffle at all, the same every epoch
    v0, v1 = (epoch_token_batches(plan, 3, e, shuffle=False) for e in (0, 1))
    assert v0 == v1 and v0[1] == list(range(plan.steps_per_epoch))
    assert [plan.keys[j] for j in v0[0]] == sorted(plan.keys)[:plan.used]


@pytest.mark.parametrize("world", [1, 2])
def test_pair_longer_than_the_budget_trains_alone(world):
    src = [5, 6, 7, 8, 90, 90][: 4 + world]
    tgt = [6, 6, 8, 9, 95, 95][: 4 + world]
    plan = plan_token_batches(src, tgt, 64, world, 8, MAX_LEN)
    assert plan.rows[-1] == world  # one row per rank
    assert plan.processed(plan.steps_per_epoch - 1) // world > 64
    assert (plan.S[-1], plan.T[-1]) == bucket_lengths(90, 95, 8, MAX_LEN)
    assert plan.used == len(src)
    assert all(plan.rows[b] // world * (plan.S[b] + plan.T[b] - 1) <= 64
               for b in range(plan.steps_per_epoch - 1))


@pytest.mark.parametrize("world", [1, 2])
def test_fill_on_the_stated_distribution(world):
    src, tgt = _lengths(4000, seed=0)
    plan = plan_token_batches(src, tgt, 4096, world, 8, 1000)
    ids, _ = epoch_token_batches(plan, 0, 0)
    real = sum(src[j] + tgt[j] - 1 for j in ids)
    processed = sum(plan.processed(b) for b in range(plan.steps_per_epoch))
    fill = real / processed
    print(f"world {world}: fill {fill:.3f} over {plan.steps_per_epoch} batches")
    assert fill >= 0.75


# ---------------------------------------------------------------- TextPairs
@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    rng = random.Random(0)
    words = [f"w{i}" for i in range(120)]
    p = tmp_path_factory.mktemp("tok") / "c.tsv"
    with open(p, "w") as f:
        for _ in range(203):
            n = min(40, int(rng.expovariate(1 / 8)) + 1)
            src = " ".join(rng.choice(words) for _ in range(n))
            tgt = " ".join(rng.choice(words) for _ in range(max(1, n + rng.randint(-3, 3))))
            f.write(f"{src}\t{tgt}\n")
    pairs = read_pairs(str(p))
    st = WordPieceTokenizer.train((s for s, _ in pairs), 200)
    tt = WordPieceTokenizer.train((t for _, t in pairs), 200)
    return str(p), st, tt


@pytest.mark.parametrize("world", [1, 2])
def test_text_pairs_token_mode(corpus, world):
    p, st, tt = corpus
    ranks = [TextPairs(p, st, tt, 64, r, world, seed=2, bucket=8, batch_tokens=256) for r in range(world)]
    d = ranks[0]
    assert d.steps_per_epoch == d.plan.steps_per_epoch > 3
    assert all(r.steps_per_epoch == d.steps_per_epoch for r in ranks)
    seen = []
    shapes = set()
    for step in range(d.steps_per_epoch):
        parts = [r.batch(step) for r in ranks]
        b = d.batch_index(step)
        for s, t in parts:
            assert s.dtype == t.dtype == torch.int64
            assert s.shape == (d.plan.rows[b] // world, d.plan.S[b])
            assert t.shape == (d.plan.rows[b] // world, d.plan.T[b])
        src = torch.cat([s for s, _ in parts])
        tgt = torch.cat([t for _, t in parts])
        g = d.batch_ids(step)
        assert torch.equal(src, pad_rows([d.src[j] for j in g], d.plan.S[b]))
        assert torch.equal(tgt, pad_rows([d.tgt[j] for j in g], d.plan.T[b]))
        real, processed = d.last_counts
        # (a decoder-input position is real when its label, the next token, is not PAD)
        assert real == int((src != PAD).sum()) + int((tgt[:, 1:] != PAD).sum())
        assert processed == src.numel() + tgt[:, :-1].numel() == d.plan.processed(b)
        seen += g
        shapes.add(tuple(src.shape))
    assert len(set(seen)) == len(seen) and 0 <= len(d) - len(seen) <= world - 1
    assert len({s[0] for s in shapes}) > 1  # several row counts
    # epochs wrap around with new membership and the same shapes in another order
    n = d.steps_per_epoch
    assert sorted(d.batch_index(n + i) for i in range(n)) == list(range(n))
    assert [d.batch_ids(i) for i in range(n)] != [d.batch_ids(n + i) for i in range(n)]
    # seek / next follow batch()
    k = n + 2
    want = ranks[-1].batch(k)
    ranks[-1].seek(k)
    got = ranks[-1].next()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # validation data: the same batches every epoch, in sorted order
    v = TextPairs(p, st, tt, 64, 0, world, seed=2, bucket=8, batch_tokens=256, shuffle=False)
    assert [v.batch_ids(i) for i in range(n)] == [v.batch_ids(n + i) for i in range(n)]
    assert [v.batch_index(i) for i in range(n)] == list(range(n))


def test_text_pairs_fixed_mode_is_unchanged(corpus):
    """batch_tokens=0: today's batches, rebuilt here from the documented
    pipeline (buffered shuffle, global batches, pad to the batch's longest)."""
    from tensorflow_distributed_on_gke_amd.data.text import buffered_shuffle
    p, st, tt = corpus
    for bucket in (1, 16):
        d = TextPairs(p, st, tt, 8, 1, 2, seed=4, shuffle_buffer=50, bucket=bucket, batch_tokens=0)
        assert d.plan is None and d.steps_per_epoch == len(d) // 16
        for step in (0, 5, d.steps_per_epoch + 3):
            epoch, i = divmod(step, d.steps_per_epoch)
            order = buffered_shuffle(len(d), 50, 4 * 1_000_003 + epoch)
            g = order[i * 16:(i + 1) * 16]
            S, T = bucket_lengths(max(len(d.src[j]) for j in g), max(len(d.tgt[j]) for j in g), bucket, 1000)
            s, t = d.batch(step)
            assert torch.equal(s, pad_rows([d.src[j] for j in g[8:]], S))
            assert torch.equal(t, pad_rows([d.tgt[j] for j in g[8:]], T))
            assert d.last_counts is None


@pytest.mark.parametrize("world", [1, 2])
def test_cpu_device_corpus_equals_pad_rows(corpus, world):
    p, st, tt = corpus
    host = TextPairs(p, st, tt, 64, world - 1, world, seed=2, bucket=8, batch_tokens=256)
    dev = TextPairs(p, st, tt, 64, world - 1, world, seed=2, bucket=8, batch_tokens=256, corpus="cpu")
    assert isinstance(dev.corpus, DeviceCorpus) and host.corpus is None
    for step in range(host.steps_per_epoch + 2):
        (s0, t0), (s1, t1) = host.batch(step), dev.batch(step)
        assert s1.dtype == t1.dtype == torch.int64
        assert torch.equal(s0, s1) and torch.equal(t0, t1)
        assert host.last_counts == dev.last_counts


def test_cpu_device_corpus_gather_edges():
    rows_s = [[5], [], [7, 8, 9, 10], [11, 12]]
    rows_t = [[2, 3], [4], [], [6, 6, 6]]
    c = DeviceCorpus(rows_s, rows_t, "cpu")
    idx = torch.tensor([3, 3, 0, 1, 2, -1, 4], dtype=torch.int32)
    s, t = c.gather(idx, 3, 2)
    ok = [3, 3, 0, 1, 2]
    assert torch.equal(s[:5], pad_rows([rows_s[j][:3] for j in ok], 3))  # row 2 is cut at L
    assert torch.equal(t[:5], pad_rows([rows_t[j][:2] for j in ok], 2))
    assert bool((s[5:] == PAD).all()) and bool((t[5:] == PAD).all())  # ids outside the store
    (s32,) = c.gather(idx[:4], 5, dtype=torch.int32)
    assert s32.dtype == torch.int32 and torch.equal(s32.long(), pad_rows([rows_s[j] for j in ok[:4]], 5))


# ---------------------------------------------------------------- settings
def test_settings_defaults_and_validation():
    s = Settings()
    assert (s.batch_tokens, s.length_bucket, s.corpus_on_device) == (0, 8, True)
    assert load_settings(None, ["data=text", "batch_tokens=4096", "length_bucket=16",
                                "corpus_on_device=false"]).batch_tokens == 4096
    assert check_batch_tokens(0, "synthetic", 8) == 0
    for bad in (["batch_tokens=4096"],  # data=synthetic
                ["data=text", "batch_tokens=-1"],
                ["data=text", "batch_tokens=1.5"],
                ["data=text", "batch_tokens=64", "length_bucket=0"],
                ["length_bucket=-8"]):
        with pytest.raises(ValueError):
            load_settings(None, bad)
    for n in (True, 2.0, "64", None, -3):
        with pytest.raises(ValueError, match="batch_tokens"):
            check_batch_tokens(n, "text", 8)
    for b in (0, 1.0, True, None):
        with pytest.raises(ValueError, match="length_bucket"):
            check_batch_tokens(64, "text", b)
    with pytest.raises(ValueError, match="data=text"):
        check_batch_tokens(64, "synthetic", 8)


def test_trainer_refuses_batch_tokens_without_text():
    from tensorflow_distributed_on_gke_amd.parallel.dist import DistInfo
    from tensorflow_distributed_on_gke_amd.train.loop import Trainer
    info = DistInfo(rank=0, world=1, local_rank=0, device=torch.device("cpu"))
    with pytest.raises(ValueError, match="data=text"):
        Trainer(Settings(preset="tiny", batch_tokens=512), info)


# ---------------------------------------------------------------- training
def _records(path):
    with open(path) as f:
        return [json.loads(line) for line in f if line.strip()]


def test_records_unchanged_when_off_and_extended_when_on(corpus, tmp_path):
    from tensorflow_distributed_on_gke_amd.parallel.dist import DistInfo
    from tensorflow_distributed_on_gke_amd.train.loop import Trainer
    p, _, _ = corpus
    info = DistInfo(rank=0, world=1, local_rank=0, device=torch.device("cpu"))
    recs = {}
    for bt in (0, 256):
        logs = []
        s = Settings(preset="tiny", data="text", train_file=p, src_vocab=200, tgt_vocab=200,
                     local_batch_size=16, epochs=1, log_every=4, snapshot_every_epochs=0, resume=False,
                     dropout=0.0, batch_tokens=bt, accum_steps=2 if bt else 1,
                     temporary_directory=str(tmp_path / f"tmp{bt}"),
                     metrics_file=str(tmp_path / f"m{bt}.jsonl"))
        tr = Trainer(s, info, log=logs.append)
        tr.fit()
        recs[bt] = ([r for r in _records(s.metrics_file) if r["kind"] == "epoch"][0], logs, tr)
    off, logs_off, _ = recs[0]
    assert "fill" not in off and "real_tokens_per_s" not in off
    assert not any("token-budget" in line or "fill" in line for line in logs_off)
    on, logs_on, tr = recs[256]
    assert 0.0 < on["fill"] <= 1.0 and 0.0 < on["real_tokens_per_s"] <= on["tokens_per_s"]
    assert on["real_tokens_per_s"] == pytest.approx(on["fill"] * on["tokens_per_s"], rel=1e-9)
    assert any("local_batch_size=16 is ignored" in line for line in logs_on)
    assert any("real tokens/s, fill" in line for line in logs_on)
    assert tr.settings.steps_per_epoch == tr.train_data.plan.steps_per_epoch
    assert tr.settings.validation_steps == tr.val_data.plan.steps_per_epoch
    assert tr.global_step == tr.settings.steps_per_epoch // 2  # accum_steps=2: updates


def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gloo_worker(rank, world, port, corpus_path, tmp):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    os.environ.pop("TDG_DIST_BACKEND", None)
    torch.set_num_threads(2)
    from tensorflow_distributed_on_gke_amd.parallel import dist as tdist
    from tensorflow_distributed_on_gke_amd.train.loop import Trainer

    info = tdist.init_distributed("cpu")
    s = Settings(preset="tiny", data="text", train_file=corpus_path, src_vocab=200, tgt_vocab=200,
                 epochs=2, log_every=4, snapshot_every_epochs=0, learning_rate=0.003, worker_count=2,
                 dropout=0.0, resume=False, batch_tokens=256, length_bucket=8, loss_mode="global_mean",
                 check_replicas_every=1, temporary_directory=os.path.join(tmp, f"tmp{rank}"),
                 metrics_file=os.path.join(tmp, "metrics.jsonl"))
    logs = []
    tr = Trainer(s, info, log=logs.append)
    tr.fit()
    plan = tr.train_data.plan
    torch.save({"steps": tr.global_step, "spe": plan.steps_per_epoch, "used": plan.used,
                "pairs": len(tr.train_data), "flat": tr.model.store.flat.clone(), "logs": logs},
               os.path.join(tmp, f"res.{rank}"))
    tdist.barrier()
    tdist.shutdown()


def test_two_rank_gloo_epoch_with_token_batches(corpus, tmp_path):
    """Two gloo ranks on the CPU train two epochs of token-budget batches with
    the replica check after every step."""
    p, _, _ = corpus
    mp.start_processes(_gloo_worker, args=(2, _free_port(), p, str(tmp_path)), nprocs=2, join=True,
                       start_method="spawn")
    r0 = torch.load(tmp_path / "res.0", weights_only=True)
    r1 = torch.load(tmp_path / "res.1", weights_only=True)
    assert r0["steps"] == r1["steps"] == 2 * r0["spe"] and r0["spe"] == r1["spe"] > 3
    assert 0 <= r0["pairs"] - r0["used"] <= 1
    assert torch.equal(r0["flat"], r1["flat"])
    epochs = [x for x in _records(tmp_path / "metrics.jsonl") if x["kind"] == "epoch"]
    assert len(epochs) == 2
    for e in epochs:
        assert 0.0 < e["fill"] <= 1.0
        assert 0.0 < e["real_tokens_per_s"] < float("inf")
        assert e["train_loss"] == e["train_loss"]
    assert any("token-budget batches: batch_tokens=256" in line for line in r0["logs"])
    assert not any("token-budget batches" in line for line in r1["logs"])  # the chief logs
