"""Batch assembly on the GPU from a device-resident corpus (csrc/kernels/batch.hip,
data/corpus.py) and token-budget batches in the training step and loop.

The gather kernel's result is defined bitwise: row b of a side's output is the
first min(len, L) tokens of store row idx[b], then PAD -- what data/text.py
pad_rows builds on the host -- so every comparison here is torch.equal. The
shapes are the smallest at which the kernel's indexing can go wrong: one wave
handles one row in strides of 64 columns, four rows per workgroup, so L in
{1, 7, 33, 64} covers a partial stride, exactly one stride and (with the
second side's L + 2) a second stride, and B in {1, 3, 65} a partial workgroup
and more than one. The token store is followed by non-zero sentinel tokens, so
a read past a row's end (or past the store's) shows in the output.

The captured-step test runs the first batches of a token-budget plan (several
row counts as well as several padded lengths) through the bucketed graph cache
and requires bitwise the eager step's losses and weights."""
import random

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 7777


def _K():
    from tensorflow_distributed_on_gke_amd.ops import kernels as K
    return K


def _store(rows, pad_to=64):
    """(tokens with sentinels after the logical end, offsets) on the GPU."""
    from tensorflow_distributed_on_gke_amd.data.corpus import flatten_rows
    flat, off = flatten_rows(rows)
    tail = torch.full((pad_to,), SENTINEL, dtype=torch.int32)
    return torch.cat([flat, tail]).to(DEV), off.to(DEV)


def _rows(L, n=41, seed=0):
    """n rows of 0..L tokens: lengths 0, 1 and L present, starts at every
    residue mod 4 (L > 1), the last row one short of L."""
    r = random.Random(seed * 131 + L)
    lens = [0, 1, L, L, 1, 1, 0, L] + [r.randint(0, L) for _ in range(n - 9)] + [max(0, L - 1)]
    rows = [[r.randint(4, 30000) for _ in range(k)] for k in lens]
    return rows


def _idx(B, n):
    # the last store row first, then descending with every third id repeated
    ids = []
    j = n - 1
    while len(ids) < B:
        ids.append(j % n)
        if len(ids) % 3 == 0 and len(ids) < B:
            ids.append(j % n)
        j -= 1
    return ids[:B]


@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
@pytest.mark.parametrize("B", [1, 3, 65])
@pytest.mark.parametrize("L", [1, 7, 33, 64])
def test_gather_equals_pad_rows(L, B, dtype):
    from tensorflow_distributed_on_gke_amd.data.text import pad_rows
    K = _K()
    S, T = L, L + 2
    src_rows, tgt_rows = _rows(L, seed=1), _rows(L, seed=2)
    n = len(src_rows)
    if L > 1:
        starts = [sum(len(r) for r in src_rows[:i]) % 4 for i in range(n) if src_rows[i]]
        assert set(starts) == {0, 1, 2, 3}
    (ts, os_), (tt, ot) = _store(src_rows), _store(tgt_rows)
    ids = _idx(B, n)
    assert ids[0] == n - 1 and (B < 4 or ids[2] == ids[3])  # the last store row; a repeat
    idx = torch.tensor(ids, dtype=torch.int32, device=DEV)
    want_s = pad_rows([src_rows[j] for j in ids], S).to(dtype)
    want_t = pad_rows([tgt_rows[j] for j in ids], T).to(dtype)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    # two sides, S != T
    out_s = torch.full((B, S), -5, dtype=dtype, device=DEV)
    out_t = torch.full((B, T), -5, dtype=dtype, device=DEV)
    K.gather_rows(idx, [ts, tt], [os_, ot], [out_s, out_t], bad)
    assert torch.equal(out_s.cpu(), want_s) and torch.equal(out_t.cpu(), want_t)
    # one side
    one = torch.full((B, T), -5, dtype=dtype, device=DEV)
    K.gather_rows(idx, [tt], [ot], [one], bad)
    assert torch.equal(one.cpu(), want_t)
    assert int(bad.item()) == 0


def test_gather_minimal_shape():
    """B = 1, L = 1, rows of length 1 and 0, and a null counter."""
    K = _K()
    tok, off = _store([[9], [], [11]])
    for j, want in ((0, 9), (1, 0), (2, 11)):
        out = torch.full((1, 1), -5, dtype=torch.int64, device=DEV)
        K.gather_rows(torch.tensor([j], dtype=torch.int32, device=DEV), [tok], [off], [out], None)
        assert out.tolist() == [[want]]


def test_guard_paths_cut_and_count():
    from tensorflow_distributed_on_gke_amd.data.text import pad_rows
    K = _K()
    rows = [[5, 6, 7, 8, 9, 10], [4], [12, 13, 14]]
    tok, off = _store(rows)
    n = len(rows)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    ids = [0, 1, 2, -1, n, 2 ** 31 - 1, -2 ** 31, 0]
    idx = torch.tensor(ids, dtype=torch.int32, device=DEV)
    L = 3
    want = pad_rows([rows[j][:L] if 0 <= j < n else [] for j in ids], L)
    for counter in (bad, None):
        out = torch.full((len(ids), L), -5, dtype=torch.int64, device=DEV)
        K.gather_rows(idx, [tok], [off], [out], counter)
        assert torch.equal(out.cpu(), want)
    # rows 0 (twice) are longer than L; four ids lie outside [0, n)
    assert int(bad.item()) == 2 + 4
    # two sides count per side: the second side cuts nothing at L = 6
    bad.zero_()
    o1 = torch.empty(len(ids), L, dtype=torch.int64, device=DEV)
    o2 = torch.empty(len(ids), 6, dtype=torch.int64, device=DEV)
    K.gather_rows(idx, [tok, tok], [off, off], [o1, o2], bad)
    assert int(bad.item()) == (2 + 4) + 4
    assert torch.equal(o2.cpu(), pad_rows([rows[j] if 0 <= j < n else [] for j in ids], 6))
    # offsets that point past the token buffer are refused row by row, not followed
    wild = off.clone()
    wild[1:] += 10 ** 12
    bad.zero_()
    out = torch.full((2, L), -5, dtype=torch.int64, device=DEV)
    K.gather_rows(idx[:2], [tok], [wild], [out], bad)
    assert int(bad.item()) == 2 and bool((out == 0).all())
    # the counter is what check_gather_rows raises on
    c = K.gather_bad_counter(torch.device(DEV))
    K.gather_rows(idx[3:4], [tok], [off], [out[:1]], c)
    with pytest.raises(ValueError, match="gathered batch rows"):
        K.check_gather_rows()
    assert K.gather_bad_rows() == 0  # reset by the check


def test_unsupported_arguments_launch_nothing():
    K = _K()
    tok, off = _store([[5, 6], [7]])
    idx = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    outs = [torch.full((2, 2), -5, dtype=torch.int64, device=DEV) for _ in range(3)]
    for args, rc in (((idx, [], [], []), -1),
                     ((idx, [tok] * 3, [off] * 3, outs), -1),
                     ((idx[:0], [tok], [off], [outs[0][:0]]), -2),
                     ((idx, [tok], [off], [outs[0][:, :0].contiguous()]), -3),
                     ((idx, [tok, tok], [off, off], [outs[0], outs[1][:, :0].contiguous()]), -3)):
        with pytest.raises(RuntimeError, match=rf"rc={rc}\)"):
            K.gather_rows(*args, None)
    torch.cuda.synchronize()
    assert all(bool((o == -5).all()) for o in outs)


# ---------------------------------------------------------------- a generated corpus
@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    from tensorflow_distributed_on_gke_amd.data.text import WordPieceTokenizer, read_pairs
    rng = random.Random(0)
    words = [f"w{i}" for i in range(300)]
    p = tmp_path_factory.mktemp("gather") / "c.tsv"
    with open(p, "w") as f:
        for _ in range(400):
            n = min(120, int(rng.expovariate(1 / 18)) + 2)
            src = " ".join(rng.choice(words) for _ in range(n))
            tgt = " ".join(rng.choice(words) for _ in range(max(2, n + rng.randint(-3, 3))))
            f.write(f"{src}\t{tgt}\n")
    pairs = read_pairs(str(p))
    st = WordPieceTokenizer.train((s for s, _ in pairs), 400)
    tt = WordPieceTokenizer.train((t for _, t in pairs), 400)
    return str(p), st, tt


@pytest.mark.parametrize("world,rank", [(1, 0), (2, 1)])
def test_host_and_device_assembly_agree(corpus, world, rank):
    from tensorflow_distributed_on_gke_amd.data.text import TextPairs
    K = _K()
    p, st, tt = corpus
    kw = dict(seed=3, bucket=8, batch_tokens=1024)
    host = TextPairs(p, st, tt, 64, rank, world, **kw)
    dev = TextPairs(p, st, tt, 64, rank, world, corpus=torch.device(DEV), **kw)
    assert dev.corpus.on_gpu and host.steps_per_epoch == dev.steps_per_epoch > 4
    K.gather_bad_rows(reset=True)
    got = [dev.batch(i) for i in range(dev.steps_per_epoch)]
    for i, (s1, t1) in enumerate(got):
        s0, t0 = host.batch(i)
        assert s1.is_cuda and s1.dtype == t1.dtype == torch.int64
        assert torch.equal(s0, s1.cpu()) and torch.equal(t0, t1.cpu())
    assert K.gather_bad_rows() == 0
    K.check_gather_rows()


def _run_plan_batches(batches, bucketed):
    from tensorflow_distributed_on_gke_amd.models.transformer import Transformer, model_config
    from tensorflow_distributed_on_gke_amd.ops import tuning
    from tensorflow_distributed_on_gke_amd.train.optim import Adam
    from tensorflow_distributed_on_gke_amd.train.step import TrainStep

    tuning.AUTOTUNE = False  # identical GEMM configs in both runs
    cfg = model_config("tiny", d_model=256, heads=4, d_ff=1024, src_vocab=500, tgt_vocab=400, dropout=0.1)
    m = Transformer(cfg).build(DEV, seed=4)
    opt = Adam(m.store, cfg.d_model, lr=0.003)
    step = TrainStep(m, opt, None, workers=1, seed=6)
    if bucketed:
        step.bucketed = True
        step.graph_cache = 64
        assert step.capture(*batches[0])
    losses = [step(*b).clone() for b in batches]
    torch.cuda.synchronize()
    assert opt.iterations == len(batches)
    return m.store.flat.clone(), torch.stack(losses), step


def test_token_batches_graph_replay_matches_eager(corpus):
    """Captured steps keyed by the full batch shape: a stream of token-budget
    batches of several row counts B and several (S, T), each repeated once so
    that captures are also replayed, equals the eager step bitwise (bf16)."""
    from tensorflow_distributed_on_gke_amd.data.text import TextPairs
    p, st, tt = corpus
    d = TextPairs(p, st, tt, 64, 0, 1, seed=3, bucket=8, batch_tokens=1024, corpus=torch.device(DEV))
    first = [d.batch(i) for i in range(10)]
    assert len({s.shape[0] for s, _ in first}) > 2
    assert len({(s.shape[1], t.shape[1]) for s, t in first}) > 2
    batches = first + first[:4]
    f_e, l_e, _ = _run_plan_batches(batches, False)
    f_g, l_g, step = _run_plan_batches(batches, True)
    shapes = {(tuple(s.shape), tuple(t.shape)) for s, t in first}
    assert step.captured and step.cached_shapes == len(shapes)
    assert step.graph_stats["replays"] >= 4
    assert torch.isfinite(l_e).all()
    assert torch.equal(l_e, l_g), (l_e, l_g)
    assert torch.equal(f_e, f_g)


def test_training_loop_token_batches_on_device(corpus, tmp_path):
    """`train --set data=text --set hip_graph=true --set batch_tokens=2048`."""
    import json

    from tensorflow_distributed_on_gke_amd.config import Settings
    from tensorflow_distributed_on_gke_amd.parallel.dist import DistInfo
    from tensorflow_distributed_on_gke_amd.train.loop import Trainer
    K = _K()
    p, _, _ = corpus
    s = Settings(preset="tiny", data="text", train_file=p, src_vocab=400, tgt_vocab=400,
                 local_batch_size=16, epochs=1, log_every=8, snapshot_every_epochs=0, resume=False,
                 hip_graph=True, batch_tokens=2048, temporary_directory=str(tmp_path / "tmp"),
                 metrics_file=str(tmp_path / "m.jsonl"))
    logs = []
    info = DistInfo(rank=0, world=1, local_rank=0, device=torch.device(DEV))
    K.gather_bad_rows(reset=True)
    tr = Trainer(s, info, log=logs.append)
    assert tr.train_data.corpus is not None and tr.train_data.corpus.on_gpu
    hist = tr.fit()
    assert tr.step_fn.captured and tr.step_fn.bucketed and tr.step_fn.cached_shapes > 1
    assert K.gather_bad_rows() == 0
    plan = tr.train_data.plan
    assert tr.global_step == plan.steps_per_epoch == s.steps_per_epoch
    assert sum(plan.rows) == plan.used >= len(tr.train_data) - (info.world - 1)
    assert hist and hist[0].train_loss == hist[0].train_loss
    with open(s.metrics_file) as f:
        rec = [r for r in map(json.loads, f) if r["kind"] == "epoch"][0]
    assert 0.0 < rec["fill"] <= 1.0 and 0.0 < rec["real_tokens_per_s"] <= rec["tokens_per_s"]
    assert any("batches assembled on the device" in line for line in logs), logs
