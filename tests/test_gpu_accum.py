"""Gradient accumulation on the GPU (accum_steps = N micro-batches per
optimizer update, train/step.py TrainStep.update): the real step with
rt.accumulate set -- every gradient writer's beta = 1 path -- eager and as
captured micro-batches, on one GPU and with two gloo ranks on it; the
update-wide label count (xent.hip count_labels_multi_kernel); clipping and the
non-finite skip on the accumulated gradient. Dropout is 0 and autotuning off
throughout. Shapes are tiny-preset models at B <= 4, L <= 40, plus one 1-layer
model at d_model 512 / 8 heads (the ragged 256x256 weight-gradient launch and
the fused L <= 128 attention kernels with beta = 1)."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

import ref_accum

pytestmark = pytest.mark.gpu
DEV = "cuda"
ADAM = dict(lr=0.01, eps=1.0)  # eps = 1: the update ~linear in the gradient (tests/test_gpu_dp.py)
MODELS = {"tiny": dict(src_vocab=300, tgt_vocab=250),
          "d512": dict(layers=1, d_model=512, heads=8, d_ff=2048, src_vocab=1000, tgt_vocab=1000)}
EMB = ("encoder/embedding/embeddings", "decoder/embedding/embeddings")


def _batch(B, S, T1, V1, V2, seed, pad=(0, 0)):
    """Right-padded token batch; row b keeps S - pad[0] - b source and
    T1 - pad[1] - 2b target tokens."""
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(4, V1, (B, S), generator=g)
    tgt = torch.randint(4, V2, (B, T1), generator=g)
    for b in range(B):
        src[b, S - pad[0] - b:] = 0
        tgt[b, T1 - pad[1] - 2 * b:] = 0
    return src.to(DEV), tgt.to(DEV)


def _make(model="tiny", accum_steps=1, loss_mode="replica_mean", seed=3, **opt_kw):
    from tensorflow_distributed_on_gke_amd.models.transformer import Transformer, model_config
    from tensorflow_distributed_on_gke_amd.ops import tuning
    from tensorflow_distributed_on_gke_amd.train.optim import Adam
    from tensorflow_distributed_on_gke_amd.train.step import TrainStep

    tuning.AUTOTUNE = False  # identical GEMM configs in every run
    cfg = model_config("tiny", dropout=0.0, **MODELS[model])
    m = Transformer(cfg).build(DEV, seed=seed)
    opt = Adam(m.store, cfg.d_model, **{**ADAM, **opt_kw})
    return m, opt, TrainStep(m, opt, None, workers=1, seed=5, loss_mode=loss_mode, accum_steps=accum_steps)


def _labels(tgt) -> int:
    return int((tgt[:, 1:] != 0).sum())


def _ulp(x):
    x = x.abs()
    return torch.nextafter(x, torch.full_like(x, float("inf"))) - x


# ------------------------------------------------------------------ old + new, bitwise
@pytest.mark.parametrize("model", ["tiny", "d512"])
def test_duplicated_batch_equals_one_step_bitwise(model):
    """One update on [X, X] (replica_mean, N = 2) against one plain step on X.
    Every backward step is linear in dlogits, scaling by 1/2 commutes with
    every f32 and bf16 rounding and g/2 + g/2 = g exactly: gradient and
    weights must be bitwise equal, which checks "old + new" in every
    accumulate path of the real step. The exception is the two embedding
    tables, summed in 2^-32 fixed point (FX_SCALE, embed.hip): rounding g/2 to
    that grid does not commute, so there the bound per element is
    (occurrences of the token in X) * 2^-30 plus one f32 ulp."""
    V = MODELS[model]
    X = _batch(4, 40, 33, V["src_vocab"], V["tgt_vocab"], seed=1, pad=(3, 2))
    m1, o1, s1 = _make(model)
    m2, o2, s2 = _make(model, accum_steps=2)
    assert s2.workers == 2.0 and not o2.zero_grad  # gradient zeroing stays off
    s1(*X)
    l1 = s1.last.clone()
    s2.update([X, X])
    torch.cuda.synchronize()
    assert o1.iterations == o2.iterations == 1
    assert int(s2.rt.ctr.item()) == 2  # the dropout stream advances per micro-batch
    assert torch.equal(s2.accum[:3].cpu(), torch.tensor([float(l1[0]), 2 * float(l1[1]), 2.0]))
    occ = {EMB[0]: torch.bincount(X[0].flatten(), minlength=V["src_vocab"]),
           EMB[1]: torch.bincount(X[1][:, :-1].flatten(), minlength=V["tgt_vocab"])}
    lr = ADAM["lr"]
    bad = []
    for p1, p2 in zip(m1.store.params, m2.store.params):
        w1, w2 = p1.master, p2.master
        if p1.name in EMB:
            bound = occ[p1.name].to(torch.float32).view(-1, 1) * 2.0 ** -30 + _ulp(p1.grad)
            err = (p1.grad - p2.grad).abs()
            print(f"{p1.name}: max gradient difference {err.max().item():.3e}, "
                  f"largest bound {bound.max().item():.3e}")
            assert bool((err <= bound).all()), p1.name
            assert float(p1.grad.abs().max()) > 1e3 * float(bound.max())  # the bound is tight
            # Adam at its first step with eps = 1 moves a weight by
            # lr * g / (|g| + 1): at most lr per unit of gradient
            assert bool(((w1 - w2).abs() <= lr * bound + 2 * _ulp(w1)).all()), p1.name
        elif not (torch.equal(p1.grad, p2.grad) and torch.equal(w1, w2)):
            bad.append(p1.name)
    assert not bad, f"not bitwise equal after [X, X]: {bad}"
    assert not torch.equal(m2.store.flat, _make(model)[0].store.flat)  # it trained


# ------------------------------------------------------------------ the accumulate idiom
def _micro_batches(V, update, n=3):
    """n micro-batches of different shapes and label counts."""
    shapes = [(4, 40, 33), (3, 24, 40), (4, 33, 17), (2, 40, 25)]
    return [_batch(*shapes[(update + k) % len(shapes)], V["src_vocab"], V["tgt_vocab"],
                   seed=10 * update + k, pad=(2 + k, 1 + 2 * k)) for k in range(n)]


def _idiom(model, updates, global_mean, seed=3):
    """The project's accumulate idiom (tests/test_gpu_dp.py): sequential
    loss_and_backward(accumulate=k > 0) calls and one opt.apply()."""
    from tensorflow_distributed_on_gke_amd.models.layers import RunCtx
    m, opt, _ = _make(model, seed=seed)
    init = m.store.flat.clone()
    losses = []
    for mbs in updates:
        n_all = float(sum(_labels(t) for _, t in mbs))
        tot = 0.0
        for k, (src, tgt) in enumerate(mbs):
            rt = RunCtx(training=True, dropout=0.0, seed=5, store=m.store,
                        ctr=torch.zeros(1, dtype=torch.int64, device=DEV), accumulate=k > 0)
            if global_mean:
                o = m.loss_and_backward(src, tgt, rt, 1.0, ntok_sum=lambda t: (t.fill_(n_all), None)[1])
            else:
                o = m.loss_and_backward(src, tgt, rt, float(len(mbs)))
            tot = tot + o[0].clone()
        opt.apply()
        losses.append(tot)
    return m, init, torch.stack(losses).cpu()


def _check_update(flat, ref, init, losses, ref_losses, what):
    moved = (ref - init).norm()
    assert moved > 0
    rel = float((flat - ref).norm() / moved)
    print(f"{what}: |dweights| / |moved| = {rel:.3e}")
    assert rel < 1e-3, f"{what}: update differs from the accumulate idiom: rel {rel:.3e}"
    assert torch.allclose(losses, ref_losses, rtol=1e-3, atol=1e-4), (losses, ref_losses)


@pytest.mark.parametrize("loss_mode", ["replica_mean", "global_mean"])
def test_update_matches_the_accumulate_idiom(loss_mode):
    V = MODELS["tiny"]
    updates = [_micro_batches(V, u) for u in range(2)]
    assert all(len({_labels(t) for _, t in mbs}) == 3 for mbs in updates)
    m, opt, step = _make("tiny", accum_steps=3, loss_mode=loss_mode)
    assert step.global_mean == (loss_mode == "global_mean")
    losses = []
    for mbs in updates:
        before = step.accum.clone()
        step.update(mbs)
        losses.append((step.accum - before)[0])
    assert opt.iterations == 2
    ref, init, ref_losses = _idiom("tiny", updates, step.global_mean)
    _check_update(m.store.flat, ref.store.flat, init, torch.stack(losses).cpu(), ref_losses, loss_mode)
    if step.global_mean:  # with unequal label counts the other mode is another update
        other, _, _ = _idiom("tiny", updates, False)
        assert float((other.store.flat - ref.store.flat).norm() / (ref.store.flat - init).norm()) > 1e-2


# ------------------------------------------------------------------ captured micro-batches
def _graph_updates(V):
    """Four updates of N = 3; two bucket shapes, both inside one update."""
    a, b = (4, 32, 33), (3, 40, 25)
    plan = [(a, b, a), (b, b, a), (a, a, a), (b, a, b)]
    return [[_batch(*shp, V["src_vocab"], V["tgt_vocab"], seed=7 * u + k, pad=(1 + k, 2 + u))
             for k, shp in enumerate(row)] for u, row in enumerate(plan)]


def _run_updates(updates, graph, loss_mode, accum_steps=3):
    m, opt, step = _make("tiny", accum_steps=accum_steps, loss_mode=loss_mode)
    if graph:
        step.bucketed = True
        before = (m.store.flat.clone(), m.store.flat_grad.clone(), opt.m.clone())
        assert step.capture(*updates[0][0])
        torch.cuda.synchronize()
        # capture() trains nothing
        assert opt.iterations == 0 and int(step.rt.ctr.item()) == 0 and float(step.accum.abs().sum()) == 0
        assert torch.equal(m.store.flat, before[0]) and torch.equal(opt.m, before[2])
        if accum_steps > 1:  # ... nor disturbs the partial sums of an update under way
            assert torch.equal(m.store.flat_grad, before[1])
    shares = []
    for mbs in updates:
        step.update(mbs)
        shares.append(step.last.clone())
    torch.cuda.synchronize()
    assert opt.iterations == len(updates)
    return m.store.flat.clone(), torch.stack(shares), step.accum.clone(), step


@pytest.mark.parametrize("loss_mode", ["replica_mean", "global_mean"])
def test_captured_micro_batches_equal_eager_bitwise(loss_mode):
    updates = _graph_updates(MODELS["tiny"])
    f_e, l_e, a_e, _ = _run_updates(updates, False, loss_mode)
    f_g, l_g, a_g, st = _run_updates(updates, True, loss_mode)
    assert st.captured and st.graph_stats["replays"] == 12
    # one graph per (shape, position) seen: a first/middle/last, b first/middle/last
    keys = sorted((k[0], k[2]) for k in st.cache.entries)
    assert keys == sorted(((B, S), pos) for (B, S, _) in ((4, 32, 33), (3, 40, 25))
                          for pos in ("first", "middle", "last")), keys
    assert st.graph_stats["captures"] == 6 and st.graph_stats["evictions"] == 0
    assert torch.equal(l_e, l_g), (l_e, l_g)
    assert torch.equal(a_e, a_g)
    assert torch.equal(f_e, f_g)


def test_one_micro_batch_keeps_one_graph_per_shape():
    """N = 1: update() is the plain step and the cache holds one graph per
    batch shape, as it always did."""
    updates = [[mbs[0]] for mbs in _graph_updates(MODELS["tiny"])]
    f_e, l_e, _, _ = _run_updates(updates, False, "replica_mean", accum_steps=1)
    f_g, l_g, _, st = _run_updates(updates, True, "replica_mean", accum_steps=1)
    assert st.cached_shapes == 2 and st.graph_stats["captures"] == 2
    assert {k[2] for k in st.cache.entries} == {"only"}
    assert torch.equal(l_e, l_g) and torch.equal(f_e, f_g)


def test_text_training_loop_accumulates_bucketed_micro_batches(tmp_path):
    """`train --set data=text --set hip_graph=true --set accum_steps=3`: the
    loop feeds three length-bucketed batches per update, captured per shape
    and position as they arrive; steps count updates."""
    import random

    from tensorflow_distributed_on_gke_amd.config import Settings
    from tensorflow_distributed_on_gke_amd.parallel.dist import DistInfo
    from tensorflow_distributed_on_gke_amd.train.loop import Trainer
    rng = random.Random(0)
    words = [f"w{i}" for i in range(200)]
    p = tmp_path / "c.tsv"
    with open(p, "w") as f:
        for _ in range(100):
            n = min(36, int(rng.expovariate(1 / 12)) + 2)
            src = " ".join(rng.choice(words) for _ in range(n))
            tgt = " ".join(rng.choice(words) for _ in range(max(2, n + rng.randint(-3, 3))))
            f.write(f"{src}\t{tgt}\n")
    s = Settings(preset="tiny", data="text", train_file=str(p), src_vocab=300, tgt_vocab=300, dropout=0.0,
                 local_batch_size=4, epochs=1, log_every=4, snapshot_every_epochs=0, resume=False,
                 hip_graph=True, graph_bucket=16, max_len=40, accum_steps=3, loss_mode="global_mean",
                 temporary_directory=str(tmp_path / "tmp"))
    logs = []
    tr = Trainer(s, DistInfo(rank=0, world=1, local_rank=0, device=torch.device(DEV)), log=logs.append)
    hist = tr.fit()
    batches = tr.train_data.steps_per_epoch
    assert batches >= 12 and tr.global_step == tr.opt.iterations == batches // 3
    st = tr.step_fn
    assert st.captured and st.bucketed and st.global_mean
    assert st.graph_stats["replays"] == 3 * tr.global_step
    assert {k[2] for k in st.cache.entries} == {"first", "middle", "last"}
    assert len({(k[0], k[1]) for k in st.cache.entries}) > 1  # more than one bucket shape
    assert hist and hist[0].train_loss == hist[0].train_loss and 0 < hist[0].train_loss < 20
    assert 0.0 <= hist[0].train_acc <= 1.0


# ------------------------------------------------------------------ two ranks on one GPU
DP_CFG = MODELS["d512"]
DP_STEPS = 2


def _port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_batch(replica, i):
    B, S, T1 = [(4, 40, 33), (3, 32, 40)][replica % 2]
    s, t = _batch(B, S, T1, DP_CFG["src_vocab"], DP_CFG["tgt_vocab"], seed=100 * i + replica,
                  pad=(1 + replica, 2 + 3 * replica))
    return s, t


def _dp_worker(rank, world, port, out, loss_mode, graph, comm_thread):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank), TDG_DIST_BACKEND="gloo",
                      TDG_DP_GRAPH=graph or "0", TDG_DP_COMM_THREAD=comm_thread)
    from tensorflow_distributed_on_gke_amd.train import step as step_mod
    step_mod.DP_OVERLAP_OPT = "tail"
    from tensorflow_distributed_on_gke_amd.models.transformer import Transformer, model_config
    from tensorflow_distributed_on_gke_amd.ops import tuning
    from tensorflow_distributed_on_gke_amd.parallel import dist as tdist
    from tensorflow_distributed_on_gke_amd.parallel.ddp import DataParallel
    from tensorflow_distributed_on_gke_amd.train.optim import Adam
    from tensorflow_distributed_on_gke_amd.train.step import TrainStep

    tuning.AUTOTUNE = False
    N = 2
    info = tdist.init_distributed("cuda")
    m = Transformer(model_config("tiny", dropout=0.0, **DP_CFG)).build(info.device, seed=1 + rank)
    opt = Adam(m.store, m.cfg.d_model, **ADAM)
    ddp = DataParallel(m.store, bucket_mb=1.0)
    ddp.broadcast_params(0)
    g = m.store.flat_grad
    lo, hi = g.data_ptr(), g.data_ptr() + g.numel() * 4
    early = []  # gradient collectives issued (or recorded) outside an update's last micro-batch
    real, holder = ddp.all_reduce_async, {}

    def spy(t):
        if lo <= t.data_ptr() < hi and not holder["step"].last_micro:
            early.append(t.numel())
        return real(t)

    ddp.all_reduce_async = spy
    step = holder["step"] = TrainStep(m, opt, ddp, workers=world, seed=5, loss_mode=loss_mode,
                                      accum_steps=N)
    step.bucketed = True  # the two micro-batches of an update differ in shape
    losses = []
    if graph:
        assert step.capture(*_dp_batch(rank * N, 0))  # trains nothing
        assert opt.iterations == 0 and step.segments is not None
    for i in range(DP_STEPS):
        before = step.accum.clone()
        step.update([_dp_batch(rank * N + k, i) for k in range(N)])
        ddp.verify_replicas()
        losses.append((step.accum - before)[0].cpu())
    torch.cuda.synchronize()
    assert opt.iterations == DP_STEPS
    calls = {}
    if graph:
        assert step.captured
        for k, (_, segs, _) in step.cache.entries.items():
            calls.setdefault(k[2], []).append(segs.num_calls)
    torch.save({"flat": m.store.flat.cpu(), "loss": torch.stack(losses), "nb": len(ddp.last_buckets),
                "early": early, "calls": calls}, f"{out}.{rank}")
    ddp.close()
    tdist.barrier()
    tdist.shutdown()


@pytest.mark.parametrize("loss_mode,graph,comm_thread", [("replica_mean", "", "0"),
                                                         ("replica_mean", "seg", "0"),
                                                         ("global_mean", "seg", "force")])
def test_two_ranks_two_micro_batches_on_one_gpu(tmp_path, loss_mode, graph, comm_thread):
    world, N = 2, 2
    out = str(tmp_path / "res")
    mp.start_processes(_dp_worker, args=(world, _port(), out, loss_mode, graph, comm_thread), nprocs=world,
                       join=True, start_method="spawn")
    r0, r1 = (torch.load(f"{out}.{r}", weights_only=True) for r in range(world))
    assert torch.equal(r0["flat"], r1["flat"])  # replicas bitwise equal
    assert r0["nb"] > 2  # several spans from inside the last backward
    assert r0["early"] == [] and r1["early"] == []
    if graph:
        # a captured first micro-batch holds no host call: no collective, no wait
        assert r0["calls"]["first"] and all(c == 0 for c in r0["calls"]["first"]), r0["calls"]
        assert all(c >= r0["nb"] for c in r0["calls"]["last"]), r0["calls"]
    # the four-replica single-process update (the accumulate idiom)
    updates = [[_dp_batch(r, i) for r in range(world * N)] for i in range(DP_STEPS)]
    ref, init, ref_losses = _idiom("d512", updates, loss_mode == "global_mean", seed=1)
    _check_update(r0["flat"], ref.store.flat.cpu(), init.cpu(), r0["loss"] + r1["loss"], ref_losses,
                  f"{loss_mode} graph={graph!r}")


def _select_worker(rank, port, out):
    """One-rank RCCL communicator (forced data-parallel path, as
    tests/test_gpu_graph.py): eager updates, then choose_dp_mode with either
    outcome forced by the margin."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1",
                      LOCAL_RANK="0", TDG_DP_GRAPH="seg")
    from tensorflow_distributed_on_gke_amd.models.transformer import Transformer, model_config
    from tensorflow_distributed_on_gke_amd.ops import tuning
    from tensorflow_distributed_on_gke_amd.parallel import dist as tdist
    from tensorflow_distributed_on_gke_amd.parallel.ddp import DataParallel
    from tensorflow_distributed_on_gke_amd.train.optim import Adam
    from tensorflow_distributed_on_gke_amd.train.step import TrainStep

    tuning.AUTOTUNE = False
    info = tdist.init_distributed("cuda", force=True)
    V = MODELS["tiny"]
    updates = [[_batch(4, 32, 33, V["src_vocab"], V["tgt_vocab"], seed=5 * u + k, pad=(1 + k, 2 + u))
                for k in range(2)] for u in range(3)]
    res = {}
    for name, margin in (("eager", None), ("sel_eager", -10.0), ("sel_seg", 0.99)):
        m = Transformer(model_config("tiny", dropout=0.0, **V)).build(info.device, seed=3)
        opt = Adam(m.store, m.cfg.d_model, **ADAM)
        ddp = DataParallel(m.store, bucket_mb=0.02, min_mb=0.001, force=True)
        ddp.broadcast_params(0)
        step = TrainStep(m, opt, ddp, workers=1, seed=5, loss_mode="global_mean", accum_steps=2)
        if margin is not None:
            sel = step.choose_dp_mode(*updates[0][0], steps=2, rounds=1, margin=margin)
            torch.cuda.synchronize()
            # whole updates were timed, and none of them trained anything
            assert opt.iterations == 0 and int(step.rt.ctr.item()) == 0 and float(step.accum.abs().sum()) == 0
            assert sel["mode"] == ("0" if name == "sel_eager" else "seg") and sel["reason"] == "measured", sel
            assert sel["seg_ms"] > 0 and sel["eager_ms"] > 0, sel
            assert step.captured == (name == "sel_seg")
            if step.captured:
                assert sorted(k[2] for k in step.cache.entries) == ["first", "last"]
        for mbs in updates:
            step.update(mbs)
        torch.cuda.synchronize()
        assert opt.iterations == len(updates) and len(ddp.last_buckets) > 1
        res[name] = (m.store.flat.cpu(), step.accum.cpu())
        ddp.close()
    torch.save(res, out)
    tdist.shutdown()


def test_choose_dp_mode_times_whole_updates(tmp_path):
    out = str(tmp_path / "sel.pt")
    mp.start_processes(_select_worker, args=(_port(), out), nprocs=1, join=True, start_method="spawn")
    r = torch.load(out, weights_only=True)
    for k in ("sel_eager", "sel_seg"):  # after either choice training is unchanged
        assert torch.equal(r["eager"][0], r[k][0]), k
        assert torch.equal(r["eager"][1], r[k][1]), k


# ------------------------------------------------------------------ count_labels_multi
def _entries(n, seed):
    """n target batches: int32 / int64 mixed, B = 1, T1 = 2, odd T1, all-PAD."""
    g = torch.Generator().manual_seed(seed)
    shapes = [(1, 2), (3, 7), (4, 40), (1, 33), (2, 2), (5, 9)]
    out = []
    for i in range(n):
        B, T1 = shapes[i % len(shapes)]
        t = torch.randint(0, 5, (B, T1), generator=g, dtype=torch.int64)  # ~1/5 zeros, anywhere
        if i % 7 == 3:
            t.zero_()  # an all-PAD entry
        if i % 5 == 1:
            t[:, 1:] = 0  # only position 0 is set: no label at all
            t[:, 0] = 3
        out.append(t.to(torch.int32 if i % 2 else torch.int64).to(DEV))
    return out


@pytest.mark.parametrize("n", [1, 3, 32])
def test_count_labels_multi_is_exact(n):
    from tensorflow_distributed_on_gke_amd.ops import kernels as kk
    tgts = _entries(n, seed=n)
    if n > 1:
        assert {t.dtype for t in tgts} == {torch.int32, torch.int64}
    total = torch.full((1,), -1.0, dtype=torch.float32, device=DEV)
    counts = torch.full((32,), -1, dtype=torch.int32, device=DEV)
    kk.count_labels_multi(tgts, total, counts)
    want_total, want_counts = ref_accum.count_labels_ref(tgts)
    assert torch.equal(total.cpu(), want_total)
    assert torch.equal(counts[:n].cpu(), want_counts)
    assert bool((counts[n:] == -1).all())  # nothing written past the entries
    if n == 32:
        assert int(want_counts[3]) == 0 and int(want_counts[1]) == 0 and float(want_total) > 100
    # the step's static scalar (what the captured cross entropies read)
    static = kk.count_labels_multi(tgts)
    assert static.data_ptr() == kk.label_total(DEV)[0].data_ptr()
    assert torch.equal(static.cpu(), want_total)


def test_count_labels_multi_refuses_a_33rd_entry():
    from tensorflow_distributed_on_gke_amd.ops import kernels as kk
    tgts = _entries(ref_accum.MAX_ENTRIES + 1, seed=0)
    total = torch.full((1,), -1.0, dtype=torch.float32, device=DEV)
    counts = torch.full((40,), -1, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match=r"rc=-1"):
        kk.count_labels_multi(tgts, total, counts)
    torch.cuda.synchronize()
    assert float(total) == -1.0 and bool((counts == -1).all())  # nothing was launched


def test_label_count_is_one_launch_only_under_global_mean(monkeypatch):
    """global_mean with N > 1 launches the count once per update; replica_mean
    and any N = 1 run launch nothing new."""
    from tensorflow_distributed_on_gke_amd.ops import kernels as kk
    calls = []
    real = kk.count_labels_multi
    monkeypatch.setattr(kk, "count_labels_multi", lambda tgts, *a: (calls.append(len(tgts)), real(tgts, *a))[1])
    V = MODELS["tiny"]
    for accum, mode, want in ((1, "replica_mean", []), (1, "global_mean", []), (3, "replica_mean", []),
                              (3, "global_mean", [3, 3])):
        calls.clear()
        _, _, step = _make("tiny", accum_steps=accum, loss_mode=mode)
        for u in range(2):
            step.update(_micro_batches(V, u, n=accum))
        assert calls == want, (accum, mode, calls)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ clip and skip
def test_clip_norm_is_that_of_the_accumulated_gradient():
    V = MODELS["tiny"]
    mbs = _micro_batches(V, 0, n=2)
    m, opt, step = _make("tiny", accum_steps=2, global_clipnorm=0.01)
    step.update(mbs)
    got = opt.last_grad_norm()
    # (on the GPU the step leaves the consumed gradient in place)
    want = float(m.store.flat_grad.double().norm())
    twin, _, _ = _idiom("tiny", [mbs], False)
    idiom = float(twin.store.flat_grad.double().norm())
    first, _, _ = _idiom("tiny", [mbs[:1]], False)
    print(f"grad_norm {got!r}, float64 norm of the accumulated gradient {want!r}, idiom {idiom!r}")
    assert want > 20 * 0.01 and opt.clip_counters()["clipped_steps"] == 1
    assert abs(got - want) <= 1e-4 * want  # as tests/test_gpu_clip.py
    assert abs(got - idiom) <= 1e-3 * idiom
    # not the norm of one micro-batch's gradient
    assert abs(got - float(first.store.flat_grad.double().norm())) > 1e-2 * want


def test_nan_in_the_second_micro_batch_skips_the_update():
    V = MODELS["tiny"]
    m, opt, step = _make("tiny", accum_steps=2, global_clipnorm=0.01, skip_nonfinite=True, ema_decay=0.9)
    step.update(_micro_batches(V, 0, n=2))
    torch.cuda.synchronize()
    s = m.store
    watched = {"flat": s.flat, "m": opt.m, "v": opt.v, "compute": s.flat_compute, "step": opt.step,
               "ema": opt.ema.avg, "ema_count": opt.ema.count}
    before = {k: t.clone() for k, t in watched.items()}
    planted = []

    def plant(p):  # a NaN in the first gradient the second micro-batch completes
        if step.rt.accumulate and not planted:
            p.grad.view(-1)[0] = float("nan")
            planted.append(p.name)

    s.on_grad_ready(plant)
    step.update(_micro_batches(V, 1, n=2))
    torch.cuda.synchronize()
    s.clear_grad_hooks()
    assert planted
    for k, t in watched.items():
        assert torch.equal(t, before[k]), k
    assert opt.iterations == 1 and opt.clip_counters()["skipped_steps"] == 1
    step.update(_micro_batches(V, 2, n=2))  # and training goes on
    torch.cuda.synchronize()
    assert opt.iterations == 2 and bool(torch.isfinite(s.flat).all())
    assert not torch.equal(s.flat, before["flat"])
