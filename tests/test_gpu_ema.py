"""The weight EMA on the GPU: the streaming kernel (csrc/kernels/ema.hip)
against the float64 contract of ref_ema.py at every branch of its launch
geometry, the first-update copy, the skip flag, ranges sharing one count, the
warm-up ramp, the launcher's refusals; then the whole training step (eager and
captured, bf16 and fp8), that nothing else changes with it on, and two
data-parallel ranks on one GPU under the segmented graph."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

import ref_ema

pytestmark = pytest.mark.gpu

DEV = "cuda"
# ema_kernel's grid is capped at 8192 x 256 float4 lanes; each thread takes
# two lanes a grid apart per iteration, then at most one more
LANES = 8192 * 256
# one lane; five blocks, the last partly idle; between one and two grids (some
# threads take a pair, the others the single tail); beyond two grids with a
# remainder (a pair, then for some threads a tail) -- about 17 M floats
SIZES = [4, 4100, 4 * (LANES + 1000), 4 * (2 * LANES + 777)]
OFF = 12  # a multiple of 4, not of 4096
PAD = 64
DECAY = 0.999


def _bits(t):
    return t.detach().view(torch.int32)


class _Case:
    """p and e ranges of n floats at offset OFF of larger buffers; NaN around e."""

    def __init__(self, n, count, seed=0):
        g = torch.Generator(device=DEV).manual_seed(seed + n)
        self.n = n
        self.pbuf = torch.randn(OFF + n + PAD, generator=g, device=DEV)
        self.ebuf = torch.full((OFF + n + PAD,), float("nan"), device=DEV)
        self.ebuf[OFF:OFF + n] = torch.randn(n, generator=g, device=DEV) * 0.5
        self.p, self.e = self.pbuf[OFF:OFF + n], self.ebuf[OFF:OFF + n]
        self.count = torch.tensor([count], dtype=torch.int64, device=DEV)
        self.p0, self.e0 = self.pbuf.clone(), self.e.clone()

    def check_untouched_around(self):
        assert torch.equal(_bits(self.pbuf), _bits(self.p0))  # the weights are only read
        assert bool(torch.isnan(self.ebuf[:OFF]).all()) and bool(torch.isnan(self.ebuf[OFF + self.n:]).all())


@pytest.mark.parametrize("warmup", [False, True], ids=["plain", "warmup"])
@pytest.mark.parametrize("n", SIZES)
def test_ema_kernel_meets_contract(n, warmup):
    from tensorflow_distributed_on_gke_amd.ops import kernels as kk

    c = _Case(n, count=7)
    kk.ema_update(c.p, c.e, c.count, DECAY, warmup)
    torch.cuda.synchronize()
    assert c.count.item() == 8
    c.check_untouched_around()
    ref_ema.check_one_step(c.e, c.p, c.e0, DECAY, warmup, 7, f"n={n} warmup={warmup}")
    assert not torch.equal(c.e, c.e0)


@pytest.mark.parametrize("n", SIZES)
def test_ema_kernel_first_update_copies(n):
    from tensorflow_distributed_on_gke_amd.ops import kernels as kk

    c = _Case(n, count=0)
    c.e.fill_(float("nan"))  # nothing of e is read
    kk.ema_update(c.p, c.e, c.count, DECAY, True)
    torch.cuda.synchronize()
    assert torch.equal(_bits(c.e), _bits(c.p)) and c.count.item() == 1
    c.check_untouched_around()


def test_ema_kernel_skip_flag_leaves_average_and_count():
    from tensorflow_distributed_on_gke_amd.ops import kernels as kk

    for count in (0, 3):
        c = _Case(4 * (LANES + 1000), count=count)
        st = torch.tensor([0.0, float("inf"), 1.0, 1.0], device=DEV)  # (sumsq, norm, factor, skip)
        kk.ema_update(c.p, c.e, c.count, DECAY, False, True, norm_state=st)
        torch.cuda.synchronize()
        assert torch.equal(_bits(c.e), _bits(c.e0)) and c.count.item() == count
        c.check_untouched_around()
        st[3] = 0.0  # not skipped: the same call updates
        kk.ema_update(c.p, c.e, c.count, DECAY, False, True, norm_state=st)
        torch.cuda.synchronize()
        assert c.count.item() == count + 1
        ref_ema.check_one_step(c.e, c.p, c.e0, DECAY, False, count, f"state given, count {count}")


def test_ema_kernel_ranges_then_one_advance_equal_one_call():
    from tensorflow_distributed_on_gke_amd.ops import kernels as kk

    n = 4 * (LANES + 1000)
    cut = 4 * 1234 * 257
    for count in (0, 12):
        a, b = _Case(n, count=count), _Case(n, count=count)
        assert torch.equal(_bits(a.ebuf[OFF:OFF + n]), _bits(b.ebuf[OFF:OFF + n]))
        kk.ema_update(a.p, a.e, a.count, DECAY, True)
        kk.ema_update(b.p[:cut], b.e[:cut], b.count, DECAY, True, inc_count=False)
        torch.cuda.synchronize()
        assert b.count.item() == count  # every range of the step reads the same count
        kk.ema_update(b.p[cut:], b.e[cut:], b.count, DECAY, True, inc_count=True)
        torch.cuda.synchronize()
        assert a.count.item() == b.count.item() == count + 1
        assert torch.equal(_bits(a.e), _bits(b.e))
        b.check_untouched_around()


@pytest.mark.parametrize("count", [1, 9, 10 ** 6])
def test_ema_kernel_warmup_decay(count):
    """The contract at three points of the ramp, and the ramp itself: from
    e = 0 and p = 1 the update leaves exactly the kernel's 1 - d_eff, which
    may differ from the f32 reference's by the two ulps of d_eff (< 1) the
    contract grants the warm-up division."""
    from tensorflow_distributed_on_gke_amd.ops import kernels as kk

    c = _Case(4100, count=count)
    kk.ema_update(c.p, c.e, c.count, DECAY, True)
    torch.cuda.synchronize()
    ref_ema.check_one_step(c.e, c.p, c.e0, DECAY, True, count, f"warm-up count {count}")
    assert c.count.item() == count + 1
    p, e = torch.ones(8, device=DEV), torch.zeros(8, device=DEV)
    cnt = torch.tensor([count], dtype=torch.int64, device=DEV)
    kk.ema_update(p, e, cnt, DECAY, True)
    want = 1.0 - float(ref_ema.d_eff32(DECAY, True, count))
    got = e.double().cpu()
    print(f"count {count}: kernel 1 - d_eff {got[0].item()!r} reference {want!r}")
    assert bool((got == got[0]).all()) and abs(got[0].item() - want) <= 2 * 2.0 ** -24
    ramp = (1.0 + count) / (10.0 + count)
    assert abs((1.0 - got[0].item()) - min(DECAY, ramp)) <= 1e-6  # 2/11, 10/19, then the decay


def test_ema_launcher_refuses_bad_arguments():
    from tensorflow_distributed_on_gke_amd.ops import kernels as kk

    c = _Case(4100, count=2)
    calls = [(c.p[:6], c.e[:6], DECAY), (c.p[:0], c.e[:0], DECAY), (c.p, c.e, 1.0), (c.p, c.e, -0.1),
             (c.p, c.e, 1.5), (c.p, c.e, float("nan"))]
    for p, e, decay in calls:
        with pytest.raises(RuntimeError, match="rc=-1"):
            kk.ema_update(p, e, c.count, decay)
    torch.cuda.synchronize()
    assert torch.equal(_bits(c.e), _bits(c.e0)) and c.count.item() == 2  # nothing was launched
    with pytest.raises(RuntimeError):  # host-side validation of the binding
        kk.ema_update(c.p, c.e[:-4], c.count, DECAY)
    with pytest.raises(RuntimeError):
        kk.ema_update(c.pbuf[1:4097], c.ebuf[1:4097], c.count, DECAY)  # not 16-byte aligned
    with pytest.raises(RuntimeError):
        kk.ema_update(c.p, c.e, c.count.int(), DECAY)
    kk.ema_update(c.p, c.e, c.count, 0.0)  # decay 0 is in range: the average follows the weights
    torch.cuda.synchronize()
    ref_ema.check_one_step(c.e, c.p, c.e0, 0.0, False, 2, "decay 0")
    assert c.count.item() == 3


# --------------------------------------------------------------------------- training step
STEPS = 4


def _batches(dev):
    g = torch.Generator().manual_seed(7)
    out = []
    for i in range(STEPS + 1):
        src = torch.randint(4, 500, (16, 48), generator=g)
        tgt = torch.randint(4, 400, (16, 41), generator=g)
        src[:, 30 + i:] = 0
        tgt[:, 25 + 2 * i:] = 0
        out.append((src.to(dev), tgt.to(dev)))
    return out


def _make(fp8, **opt_kw):
    from tensorflow_distributed_on_gke_amd.models.transformer import Transformer, model_config
    from tensorflow_distributed_on_gke_amd.ops import tuning
    from tensorflow_distributed_on_gke_amd.train.optim import Adam
    from tensorflow_distributed_on_gke_amd.train.step import TrainStep

    tuning.AUTOTUNE = False  # identical GEMM configs in every run
    cfg = model_config("tiny", d_model=256, heads=4, d_ff=1024, src_vocab=500, tgt_vocab=400, dropout=0.1)
    m = Transformer(cfg).build(DEV, seed=3)
    opt = Adam(m.store, cfg.d_model, lr=0.003, **opt_kw)
    st = None
    if fp8:
        from tensorflow_distributed_on_gke_amd.ops.fp8 import Fp8State
        st = Fp8State(m)
    return m, opt, TrainStep(m, opt, None, workers=1, seed=11, fp8_state=st)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_step_capture_leaves_no_ema_update_behind(fp8):
    """capture() runs warm-up steps and restores the state: with the average
    and its count part of that state, the first replayed step is the first
    update -- a copy."""
    m, opt, step = _make(fp8, ema_decay=DECAY)
    bs = _batches(DEV)
    opt.ema.avg.fill_(float("nan"))
    assert step.capture(*bs[0], warmup=2) and step.graph is not None
    assert opt.ema.updates == 0 and opt.iterations == 0
    assert bool(torch.isnan(opt.ema.avg).all())
    step(*bs[0])
    torch.cuda.synchronize()
    assert opt.ema.updates == 1 and opt.iterations == 1
    assert torch.equal(_bits(opt.ema.avg), _bits(m.store.flat))


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_step_ema_meets_contract_step_by_step(fp8, graph):
    m, opt, step = _make(fp8, ema_decay=DECAY, ema_warmup=True)
    if fp8:
        assert step.fp8.weights.adam_chunks(m.store) is not None  # the fused fp8 Adam path
    bs = _batches(DEV)
    if graph:
        assert step.capture(*bs[0], warmup=2)
    for k in range(STEPS):
        before = opt.ema.avg.clone()
        step(*bs[k])
        torch.cuda.synchronize()
        assert opt.ema.updates == k + 1
        ref_ema.check_one_step(opt.ema.avg, m.store.flat, before, DECAY, True, k,
                               f"fp8={fp8} graph={graph} step {k}")
    assert opt.ema.updates == STEPS == opt.iterations
    assert not torch.equal(opt.ema.avg, m.store.flat)


def _validate(m, batch):
    from tensorflow_distributed_on_gke_amd.models.layers import RunCtx

    acc = torch.zeros(4, device=DEV)
    out = torch.zeros(2, device=DEV)
    m.loss_and_backward(*batch, RunCtx(training=False, store=None), 1.0, accum=acc, backward=False,
                        step_out=out)
    torch.cuda.synchronize()
    return float(out[0].item())


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_ema_changes_nothing_else(fp8):
    """Weights, moments and step of a captured run with the EMA on -- and a
    validation pass on the averaged weights in its middle -- are bitwise
    those of the run with it off; the swap leaves the fp8 state alone."""
    bs = _batches(DEV)
    res = {}
    for name, kw in (("off", {}), ("on", dict(ema_decay=0.9))):
        m, opt, step = _make(fp8, **kw)
        assert step.capture(*bs[0], warmup=2)
        for k in range(STEPS):
            if k == 2 and opt.ema is not None:
                s = m.store
                watched = {"compute": s.flat_compute}
                if fp8:
                    f = step.fp8
                    watched.update({"scale": f.meta.scale, "gscale": f.gmeta.scale, "amax": f.meta.amax,
                                    "gamax": f.gmeta.amax})
                    for i, (_, w8, _, _) in enumerate(f.weights.items):
                        watched[f"w8.{i}"] = w8.view(torch.uint8)
                fixed = [k_ for k_ in watched if k_ != "compute"]
                before = {k_: t.clone() for k_, t in watched.items()}
                flat, avg = s.flat.clone(), opt.ema.avg.clone()
                raw_loss = _validate(m, bs[STEPS])
                with opt.ema.swapped():
                    assert torch.equal(_bits(s.flat), _bits(avg))
                    assert not torch.equal(s.flat_compute, before["compute"])  # the model runs on the average
                    for k_ in fixed:
                        assert torch.equal(watched[k_], before[k_]), k_
                    ema_loss = _validate(m, bs[STEPS])
                    with pytest.raises(RuntimeError, match="swapped"):
                        step(*bs[k])
                torch.cuda.synchronize()
                print(f"fp8={fp8}: validation loss raw {raw_loss:.5f} ema {ema_loss:.5f}")
                assert ema_loss == ema_loss and ema_loss != raw_loss
                assert torch.equal(_bits(s.flat), _bits(flat)) and torch.equal(_bits(opt.ema.avg), _bits(avg))
                for k_, t in watched.items():
                    assert torch.equal(t, before[k_]), k_
            step(*bs[k])
        torch.cuda.synchronize()
        res[name] = {"flat": m.store.flat.clone(), "m": opt.m.clone(), "v": opt.v.clone(),
                     "step": opt.step.clone(), "compute": m.store.flat_compute.clone()}
        if name == "on":
            assert opt.ema.updates == STEPS
    for k, t in res["off"].items():
        assert t.dtype == res["on"][k].dtype and torch.equal(t.view(torch.uint8), res["on"][k].view(torch.uint8)), k


# --------------------------------------------------------------------------- data parallel
CFG = dict(d_model=512, heads=8, d_ff=2048, src_vocab=1000, tgt_vocab=1000, dropout=0.0)
DP_STEPS = 3


def _port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _batch(rank, i):
    g = torch.Generator().manual_seed(100 * i + rank)
    src = torch.randint(4, 1000, (8, 64), generator=g)
    tgt = torch.randint(4, 1000, (8, 65), generator=g)
    src[:, 50 + rank:] = 0
    tgt[:, 40 + 3 * rank:] = 0
    return src, tgt


def _worker(rank, world, port, out):
    import sys

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank), TDG_DIST_BACKEND="gloo",
                      TDG_DP_GRAPH="seg", TDG_DP_COMM_THREAD="force", TDG_DP_SIGNAL="1")
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from tensorflow_distributed_on_gke_amd.train import step as step_mod
    step_mod.WAVE_TILES = 37  # small waves: problems cut across launches
    step_mod.DP_OVERLAP_OPT = "tail"
    from tensorflow_distributed_on_gke_amd.models.transformer import Transformer, model_config
    from tensorflow_distributed_on_gke_amd.ops import tuning
    from tensorflow_distributed_on_gke_amd.parallel import dist as tdist
    from tensorflow_distributed_on_gke_amd.parallel.ddp import DataParallel
    from tensorflow_distributed_on_gke_amd.train.optim import Adam
    from tensorflow_distributed_on_gke_amd.train.step import TrainStep

    tuning.AUTOTUNE = False
    info = tdist.init_distributed("cuda")
    m = Transformer(model_config("tiny", **CFG)).build(info.device, seed=1 + rank)
    opt = Adam(m.store, m.cfg.d_model, lr=0.05, eps=1.0, ema_decay=0.9, ema_warmup=True)
    ddp = DataParallel(m.store, bucket_mb=1.0)
    ddp.broadcast_params(0)
    step = TrainStep(m, opt, ddp, workers=world, seed=5)
    assert ddp.opt is opt and ddp.ema is opt.ema
    src, tgt = _batch(rank, 0)
    assert step.capture(src.to(info.device), tgt.to(info.device))
    assert step.segments is not None and step.segments.num_calls >= 2
    assert opt.iterations == 0 and opt.ema.updates == 0
    for i in range(DP_STEPS):
        before = opt.ema.avg.clone()
        src, tgt = _batch(rank, i)
        step(src.to(info.device), tgt.to(info.device))
        torch.cuda.synchronize()
        ddp.verify_replicas()  # (weights, average and count)
        assert opt.ema.updates == i + 1
        ref_ema.check_one_step(opt.ema.avg, m.store.flat, before, 0.9, True, i, f"rank {rank} step {i}")
    assert opt.iterations == DP_STEPS
    torch.save({"avg": opt.ema.avg.cpu(), "flat": m.store.flat.cpu(), "count": opt.ema.updates,
                "nb": len(ddp.last_buckets)}, f"{out}.{rank}")
    ddp.close()
    tdist.barrier()
    tdist.shutdown()


def test_gpu_dp_ema_segmented_graph(tmp_path):
    world = 2
    out = str(tmp_path / "res")
    mp.start_processes(_worker, args=(world, _port(), out), nprocs=world, join=True, start_method="spawn")
    r0, r1 = (torch.load(f"{out}.{r}", weights_only=True) for r in range(world))
    assert torch.equal(_bits(r0["avg"]), _bits(r1["avg"])) and torch.equal(r0["flat"], r1["flat"])
    assert r0["count"] == r1["count"] == DP_STEPS
    assert r0["nb"] > 2  # several spans, each with its own Adam range, one EMA update after them
    assert not torch.equal(r0["avg"], r0["flat"])
