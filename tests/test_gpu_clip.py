"""Global-norm gradient clipping and non-finite step skip on the GPU: the
norm kernels (grad_sumsq + grad_norm_finalize), the Adam kernels reading the
decision from device memory, the whole training step (eager and captured,
bf16 and fp8) and two data-parallel ranks on one GPU."""
import math
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

import ref_tail as R

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _close(a, b, tol, what):  # as tests/test_gpu_kernels.py
    a = a.float().cpu()
    b = b.float().cpu()
    err = (a - b).abs().max().item()
    ref = b.abs().max().item() + 1e-6
    assert err <= tol * ref, f"{what}: max err {err:.3e} vs max |ref| {ref:.3e}"


def _plain_rows(a, b):
    return [(c0, min(4096, b - c0), -1, 0) for c0 in range(a, b, 4096)]


# --------------------------------------------------------------------------- norm kernels
@pytest.mark.parametrize("n", [4, 4092, 4096, 4100, 3 * 4096 + 8, 2 ** 20 + 4])
@pytest.mark.parametrize("off", [12, 4096 + 2052])
def test_grad_sumsq_ranges(n, off):
    """Plain (ptr, n) ranges and the same ranges as a chunk table, starting at
    a multiple of 4 that is not a multiple of 4096, with NaN just outside."""
    from tensorflow_distributed_on_gke_amd.ops import kernels as kk

    g = torch.Generator().manual_seed(n + off)
    buf = torch.full((off + n + 4096,), float("nan"), device=DEV)
    vals = torch.randn(n, generator=g)
    buf[off:off + n] = vals.to(DEV)
    want = float(vals.double().pow(2).sum())
    nch = (n + 4095) // 4096
    tab = torch.tensor(_plain_rows(off, off + n), dtype=torch.int64, device=DEV)
    assert tab.shape[0] == nch
    outs = []
    for form in ("plain", "plain", "table", "table"):
        partials = torch.full((nch + 3,), 7.0, device=DEV)
        st = torch.zeros(4, device=DEV)
        cn = torch.zeros(4, dtype=torch.int32, device=DEV)
        if form == "plain":
            k = kk.grad_sumsq(buf[off:off + n], partials, 1)
        else:
            k = kk.grad_sumsq(buf, partials, 1, chunks=tab)
        assert k == nch
        kk.grad_norm_finalize(partials[1:], k, st, cn)
        torch.cuda.synchronize()
        assert partials[0].item() == 7.0 and bool((partials[1 + nch:] == 7.0).all())  # no stray partial
        sumsq, norm, factor, skip = st.tolist()
        print(f"n={n} off={off} {form}: sumsq {sumsq!r} want {want!r} rel {abs(sumsq - want) / want:.2e}")
        assert abs(sumsq - want) <= 1e-5 * want
        assert abs(norm - math.sqrt(want)) <= 1e-5 * math.sqrt(want)
        assert factor == 1.0 and skip == 0.0  # clipping and skipping off
        assert cn.tolist()[:2] == [0, 0]
        assert cn[2:3].view(torch.float32).item() == norm
        outs.append((partials.clone(), st.clone()))
    for p, s in outs[1:]:  # bitwise reproducible, and one chunking for both forms
        assert torch.equal(p, outs[0][0]) and torch.equal(s, outs[0][1])


def test_grad_norm_finalize_decisions():
    from tensorflow_distributed_on_gke_amd.ops import kernels as kk

    n = 4096 + 8
    g = torch.full((n,), 0.5, device=DEV)  # norm = 0.5 * sqrt(n) ~ 32.03
    norm = 0.5 * math.sqrt(n)
    partials = torch.zeros(4, device=DEV)
    st = torch.zeros(4, device=DEV)
    cn = torch.zeros(4, dtype=torch.int32, device=DEV)

    def run(grad, **kw):
        k = kk.grad_sumsq(grad, partials)
        kk.grad_norm_finalize(partials, k, st, cn, **kw)
        return st.tolist(), cn.tolist()

    s, c = run(g, clip=100.0)
    assert s[2] == 1.0 and s[3] == 0.0 and c[:2] == [0, 0]  # norm <= clip: exactly 1.0f
    s, c = run(g, clip=2.0, skip_nonfinite=True)
    assert abs(s[1] - norm) <= 1e-6 * norm and abs(s[2] - 2.0 / norm) <= 1e-6 and c[:2] == [1, 0]
    s, c = run(g, clip=2.0, grad_scale=0.01)  # norm after grad_scale ~ 0.32 < clip
    assert abs(s[1] - 0.01 * norm) <= 1e-6 * norm and s[2] == 1.0 and c[:2] == [1, 0]
    for bad in (float("inf"), float("nan")):
        gb = g.clone()
        gb[4100] = bad
        s, c0 = run(gb, clip=2.0, skip_nonfinite=True)
        assert not math.isfinite(s[1]) and s[2] == 1.0 and s[3] == 1.0
        s, c1 = run(gb, skip_nonfinite=True)  # skipping without clipping: factor stays 1
        assert s[2] == 1.0 and s[3] == 1.0 and c1[1] == c0[1] + 1
        s, c2 = run(gb, clip=2.0)  # not skipped: NaN, as tf.clip_by_global_norm signals it
        assert math.isnan(s[2]) and s[3] == 0.0 and c2[1] == c1[1]
    # the maximum is over the finite norms only
    assert abs(cn[2:3].view(torch.float32).item() - norm) <= 1e-6 * norm


# --------------------------------------------------------------------------- Adam kernels
ARGS = (0.9, 0.98, 1e-9, 0.0, 128.0, 4000.0)
W8 = (8, 2048)  # (offset, numel) of the weight with an e4m3 copy in the fp8 table


class _AdamCase:
    def __init__(self, n, form, seed=0):
        from tensorflow_distributed_on_gke_amd.ops import fp8 as F

        gen = torch.Generator().manual_seed(seed + n)
        self.n, self.form = n, form
        self.p = torch.randn(n, generator=gen)
        self.g = torch.randn(n, generator=gen)
        self.meta = F.Fp8Meta(DEV)
        self.slot = self.meta.slot("w:a")
        self.meta.scale[self.slot] = 64.0
        self.y8 = torch.zeros(W8[1], dtype=F.FP8, device=DEV)
        if form == "chunks8":
            off, k = W8
            rows = _plain_rows(0, off) + [(off, k, self.slot, self.y8.data_ptr())] + _plain_rows(off + k, n)
            F.validate_chunk_table(rows, n, self.meta.scale.numel(), [(self.y8.data_ptr(), k)])
        else:
            rows = _plain_rows(0, n)
        self.tab = torch.tensor(rows, dtype=torch.int64, device=DEV)

    def state(self, g, gs=1.0, **kw):
        from tensorflow_distributed_on_gke_amd.ops import kernels as kk

        partials = torch.zeros(8, device=DEV)
        st = torch.zeros(4, device=DEV)
        cn = torch.zeros(4, dtype=torch.int32, device=DEV)
        kk.grad_norm_finalize(partials, kk.grad_sumsq(g, partials), st, cn, grad_scale=gs, **kw)
        return st

    def run(self, g=None, state="none", gs=1.0, zero_grad=True, **kw):
        """One Adam call from m = v = 0 at step 10. Returns every buffer the
        kernel may write."""
        from tensorflow_distributed_on_gke_amd.ops import kernels as kk

        n = self.n
        pd = self.p.clone().to(DEV)
        gd = (self.g if g is None else g).clone().to(DEV)
        md, vd = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        sh = torch.full((n,), 3.0, dtype=torch.bfloat16, device=DEV)
        step = torch.tensor([10], dtype=torch.int64, device=DEV)
        self.meta.amax.zero_()
        self.y8.view(torch.uint8).fill_(0x55)
        st = self.state(gd, gs, **kw) if state == "norm" else None
        if self.form == "adam":
            kk.adam(pd, gd, md, vd, sh, step, *ARGS, gs, 0.0, 1, zero_grad, True, norm_state=st)
        else:
            kk.adam_chunks(pd, gd, md, vd, sh, self.tab, step, *ARGS, gs, 0.0, 1, zero_grad, True,
                           self.meta.scale, self.meta.amax, norm_state=st)
        torch.cuda.synchronize()
        return dict(p=pd, g=gd, m=md, v=vd, shadow=sh, step=step, y8=self.y8.view(torch.uint8).clone(),
                    amax=self.meta.amax.clone(), state=st)


@pytest.mark.parametrize("n", [4096, 4096 + 8])
@pytest.mark.parametrize("form", ["adam", "chunks", "chunks8"])
def test_adam_kernels_apply_clip_factor(n, form):
    from tensorflow_distributed_on_gke_amd.ops import fp8 as F

    c = _AdamCase(n, form)
    norm = float(c.g.double().norm())  # ~ 64
    for gs, clip in ((1.0, 1.0), (0.5, 4.0)):
        assert clip < gs * norm / 4
        out = c.run(state="norm", gs=gs, clip=clip)
        factor = clip / (gs * norm)
        assert abs(out["state"][2].item() - factor) <= 1e-6 * factor
        ge = c.g * gs * factor
        lr = 128 ** -0.5 * min(10 * 4000 ** -1.5, 10 ** -0.5)
        lr_t = lr * math.sqrt(1 - 0.98 ** 11) / (1 - 0.9 ** 11)
        m_ = ge * 0.1
        ref = c.p - lr_t * m_ / ((ge * ge * 0.02).sqrt() + 1e-9)
        _close(out["p"], ref, 1e-5, "adam p")
        _close(out["m"], m_, 1e-6, "adam m")
        _close(out["shadow"], ref, 1e-2, "adam shadow")
        assert out["step"].item() == 11
        assert out["g"].abs().max().item() == 0.0
        # v = (g * gs * factor)^2 * (1 - beta2) is the buffer that shows the factor (Adam's
        # first step from zero moments does not depend on the gradient's scale, so p cannot);
        # p through its update, m and v elementwise against the float64 reference, whose
        # grad_scale is the f32 product the kernels form from the device's factor
        gsf = float(torch.tensor(gs, dtype=torch.float32) * out["state"][2].cpu())
        zero = torch.zeros(n)
        R.check_adam((out["p"].cpu(), out["m"].cpu(), out["v"].cpu()), c.p, c.g, zero, zero, 10,
                     R.AdamCfg(grad_scale=gsf), f"{form} gs={gs} clip={clip}")
        # ... and against the host's factor, which the device's matches to 1e-6 (above):
        # 2e-6 for its square, on top of the table's f32 tolerance
        want = (c.g.double() * gs * factor) ** 2 * (1 - R._f32r(0.98))
        assert bool(((out["v"].cpu().double() - want).abs() <= (2e-6 + R.tol("adam_v")) * want).all())
        if form == "chunks8":
            off, k = W8
            want = F.quantize(out["shadow"][off:off + k], c.meta, c.slot, record=False)
            assert torch.equal(out["y8"], want.view(torch.uint8))
    # norm <= clip: factor exactly 1.0f, bitwise the call with a null state
    for gs in (1.0, 0.5):
        a = c.run(state="norm", gs=gs, clip=2 * norm)
        b = c.run(state="none", gs=gs)
        assert a["state"][2].item() == 1.0
        for k in ("p", "g", "m", "v", "shadow", "step", "y8", "amax"):
            assert torch.equal(a[k], b[k]), k
    if form == "chunks8":
        assert not bool((b["y8"] == 0x55).all()) and bool(b["amax"].any())  # the fp8 chunks ran


@pytest.mark.parametrize("n", [4096, 4096 + 8])
@pytest.mark.parametrize("form", ["adam", "chunks", "chunks8"])
def test_adam_kernels_skip_nonfinite(n, form):
    c = _AdamCase(n, form)
    for bad in (float("inf"), float("nan")):
        g = c.g.clone()
        g[n - 3] = bad
        for zero_grad in (True, False):
            out = c.run(g=g, state="norm", zero_grad=zero_grad, clip=1.0, skip_nonfinite=True)
            assert out["state"][3].item() == 1.0
            assert torch.equal(out["p"].cpu(), c.p)
            assert not out["m"].any() and not out["v"].any()
            assert bool((out["shadow"] == 3.0).all())
            assert bool((out["y8"] == 0x55).all()) and not out["amax"].any()
            assert out["step"].item() == 10
            if zero_grad:
                assert not out["g"].any()  # still consumed
            else:
                assert torch.equal(out["g"].cpu().view(torch.int32), g.view(torch.int32))


# --------------------------------------------------------------------------- training step
STEPS = 3
CLIP = 0.01  # far below the tiny model's first gradient norm (asserted)


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


def _run(fp8, graph, steps=STEPS + 1, **opt_kw):
    m, opt, step = _make(fp8, **opt_kw)
    bs = _batches(DEV)
    if graph:
        assert step.capture(*bs[0], warmup=2)
        assert step.graph is not None
        assert opt.iterations == 0 and int(step.rt.ctr.item()) == 0
        if opt.clip_on:  # capture() trains nothing and counts nothing
            assert opt.clip_counters() == {"clipped_steps": 0, "skipped_steps": 0, "grad_norm_max": 0.0}
    norms = []
    for i in range(steps):
        step(*bs[i])
        if opt.clip_on:
            norms.append(opt.last_grad_norm())
    torch.cuda.synchronize()
    assert opt.iterations == steps
    return m, opt, norms


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_step_clip_graph_replay_matches_eager(fp8):
    me, oe, ne = _run(fp8, graph=False, global_clipnorm=CLIP)
    mg, og, ng = _run(fp8, graph=True, global_clipnorm=CLIP)
    assert torch.isfinite(mg.store.flat).all()
    assert torch.equal(me.store.flat, mg.store.flat)
    assert ne == ng
    assert og.clip_counters() == oe.clip_counters()
    assert og.clip_counters()["clipped_steps"] == STEPS + 1
    # the reported norm: the float64 norm of a twin's first gradient (same
    # kernels; on the GPU the step leaves the consumed gradient in place)
    mt, ot, _ = _run(fp8, graph=False, steps=1)
    want = float(mt.store.flat_grad.double().norm())
    print(f"fp8={fp8}: grad_norm {ne[0]!r} twin float64 norm {want!r}")
    assert want > 20 * CLIP
    assert abs(ne[0] - want) <= 1e-4 * want
    mc, _, _ = _run(fp8, graph=False, steps=1, global_clipnorm=CLIP)
    assert not torch.equal(mc.store.flat, mt.store.flat)  # clipping changed the update


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_step_skip_nonfinite_leaves_model_unchanged(fp8):
    m, opt, step = _make(fp8, global_clipnorm=CLIP, skip_nonfinite=True)
    bs = _batches(DEV)
    step(*bs[0])
    step.model.loss_and_backward(*bs[1], step.rt, 1.0)
    torch.cuda.synchronize()
    s = m.store
    watched = {"flat": s.flat, "m": opt.m, "v": opt.v, "compute": s.flat_compute, "step": opt.step}
    if fp8:
        names = step.fp8.meta.names
        wslots = [i for i, n in enumerate(names) if n.startswith(("w:", "wt:"))]
        assert wslots and step.fp8.weights.adam_chunks(s) is not None  # the fused fp8 Adam path
        for i, (_, w8, _, _) in enumerate(step.fp8.weights.items):
            watched[f"w8.{i}"] = w8.view(torch.uint8)
    before = {k: t.clone() for k, t in watched.items()}
    wscale = step.fp8.meta.scale[wslots].clone() if fp8 else None
    s.flat_grad[s.total // 2] = float("inf")
    step.optimize()
    torch.cuda.synchronize()
    for k, t in watched.items():
        assert torch.equal(t, before[k]), k
    if fp8:  # the untouched e4m3 copies keep the scales they were written with
        assert torch.equal(step.fp8.meta.scale[wslots], wscale)
    assert opt.iterations == 1
    assert opt.clip_counters()["skipped_steps"] == 1 and not math.isfinite(opt.last_grad_norm())
    step(*bs[2])  # and training goes on
    torch.cuda.synchronize()
    assert opt.iterations == 2 and torch.isfinite(s.flat).all()
    assert not torch.equal(s.flat, before["flat"])


# --------------------------------------------------------------------------- data parallel
CFG = dict(d_model=512, heads=8, d_ff=2048, src_vocab=1000, tgt_vocab=1000, dropout=0.0)
# eps = 1 keeps the update ~linear in the gradient (tests/test_gpu_dp.py); the
# learning rate makes up for the clip factor (~1e-2), so the update stays well
# above the f32 weights' own rounding, as the unclipped one of that file does
DP_ADAM = dict(lr=1.0, eps=1.0)
DP_CLIP = 0.02


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


def _worker(rank, world, port, out, graph, comm_thread):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank), TDG_DIST_BACKEND="gloo",
                      TDG_DP_GRAPH=graph or "0", TDG_DP_COMM_THREAD=comm_thread, TDG_DP_SIGNAL="1")
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
    opt = Adam(m.store, m.cfg.d_model, global_clipnorm=DP_CLIP, **DP_ADAM)
    ddp = DataParallel(m.store, bucket_mb=1.0)
    ddp.broadcast_params(0)
    step = TrainStep(m, opt, ddp, workers=world, seed=5)
    assert ddp.opt is opt
    if graph:
        src, tgt = _batch(rank, 0)
        assert step.capture(src.to(info.device), tgt.to(info.device))
        assert step.segments is not None and step.segments.num_calls >= 2
        assert opt.iterations == 0 and opt.clip_counters()["clipped_steps"] == 0
    norms = []
    for i in range(DP_STEPS):
        src, tgt = _batch(rank, i)
        step(src.to(info.device), tgt.to(info.device))
        ddp.verify_replicas()
        norms.append(opt.last_grad_norm())
    torch.cuda.synchronize()
    assert opt.iterations == DP_STEPS
    torch.save({"flat": m.store.flat.cpu(), "norms": torch.tensor(norms, dtype=torch.float64),
                "nb": len(ddp.last_buckets), "counters": opt.clip_counters()}, f"{out}.{rank}")
    ddp.close()
    tdist.barrier()
    tdist.shutdown()


DP_STEPS = 3


@pytest.mark.parametrize("graph,comm_thread", [("", "0"), ("seg", "force")], ids=["eager", "seg"])
def test_gpu_dp_clip_matches_single_process(tmp_path, graph, comm_thread, monkeypatch):
    from tensorflow_distributed_on_gke_amd.models.layers import RunCtx
    from tensorflow_distributed_on_gke_amd.models.transformer import Transformer, model_config
    from tensorflow_distributed_on_gke_amd.ops import tuning
    from tensorflow_distributed_on_gke_amd.train.optim import Adam

    world = 2
    out = str(tmp_path / "res")
    mp.start_processes(_worker, args=(world, _port(), out, graph, comm_thread), nprocs=world, join=True,
                       start_method="spawn")
    r0, r1 = (torch.load(f"{out}.{r}", weights_only=True) for r in range(world))
    assert torch.equal(r0["flat"], r1["flat"])  # replicas bitwise identical
    assert torch.equal(r0["norms"], r1["norms"])  # one norm, of the summed gradient
    assert r0["nb"] > 2  # several spans launched from inside backward
    assert r0["counters"]["clipped_steps"] == DP_STEPS and r0["counters"]["skipped_steps"] == 0
    # single process: both ranks' batches accumulated, clipped once
    monkeypatch.setattr(tuning, "AUTOTUNE", False)
    m = Transformer(model_config("tiny", **CFG)).build("cuda", seed=1)
    init = m.store.flat.clone()
    opt = Adam(m.store, m.cfg.d_model, global_clipnorm=DP_CLIP, **DP_ADAM)
    norms = []
    for i in range(DP_STEPS):
        for r in range(world):
            rt = RunCtx(training=True, dropout=0.0, seed=5, store=m.store,
                        ctr=torch.zeros(1, dtype=torch.int64, device="cuda"), accumulate=r > 0)
            src, tgt = _batch(r, i)
            m.loss_and_backward(src.cuda(), tgt.cuda(), rt, float(world))
        opt.apply()
        norms.append(opt.last_grad_norm())
    print(f"graph={graph!r}: norms dp {r0['norms'].tolist()} single {norms}")
    assert min(norms) > 20 * DP_CLIP
    assert torch.allclose(r0["norms"], torch.tensor(norms, dtype=torch.float64), rtol=1e-3)
    ref = m.store.flat.cpu()
    moved = (ref - init.cpu()).norm()
    assert moved > 0
    rel = (r0["flat"] - ref).norm() / moved
    print(f"graph={graph!r}: rel {rel:.3e}")
    assert rel < 1e-3, f"DP update differs from the single-process update: rel {rel:.3e}"
