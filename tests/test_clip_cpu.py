"""Adam's opt-in global-norm gradient clipping (Keras `global_clipnorm`,
tf.clip_by_global_norm) and non-finite step skip, on the CPU path: the update
against the formula written out in float64, the skip rules, the settings, and
two gloo ranks whose replicas must stay bitwise equal while clipping by the
norm of the all-reduced gradient."""
import math
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

from tensorflow_distributed_on_gke_amd.config import load_settings
from tensorflow_distributed_on_gke_amd.data.synthetic import SyntheticPairs
from tensorflow_distributed_on_gke_amd.models.layers import RunCtx
from tensorflow_distributed_on_gke_amd.models.transformer import Transformer, model_config
from tensorflow_distributed_on_gke_amd.train.optim import Adam

CFG = dict(src_vocab=60, tgt_vocab=50, dropout=0.0)
B1, B2, EPS, LR = 0.9, 0.98, 1e-9, 0.01


def _model(seed=1):
    return Transformer(model_config("tiny", **CFG)).build("cpu", seed=seed)


def _grads(n, steps, scale):
    g = torch.Generator().manual_seed(11)
    return [torch.randn(n, generator=g) * scale for _ in range(steps)]


def _formula64(p0, grads, clip, grad_scale):
    """tf.clip_by_global_norm + Keras Adam, in float64. Returns p, m, v and
    the per-step norms."""
    p = p0.double().clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    norms = []
    for t, g in enumerate(grads, 1):
        g = g.double() * grad_scale
        norm = g.pow(2).sum().sqrt()
        norms.append(float(norm))
        if clip > 0:
            g = g * (clip / max(float(norm), clip))
        m += (g - m) * (1 - B1)
        v += (g * g - v) * (1 - B2)
        lr_t = LR * math.sqrt(1 - B2 ** t) / (1 - B1 ** t)
        p -= lr_t * m / (v.sqrt() + EPS)
    return p, m, v, norms


# gradient of norm ~ sqrt(n) * 0.1 (n ~ 1e5: ~ 30): clip 1e4 never clips,
# clip 0.5 always does
@pytest.mark.parametrize("clip,grad_scale", [(1e4, 1.0), (0.5, 1.0), (0.5, 0.25)],
                         ids=["below", "above", "grad_scale"])
def test_cpu_adam_global_clipnorm_matches_float64_formula(clip, grad_scale):
    steps = 3
    mc, mu = _model(), _model()
    n = mc.store.total
    grads = _grads(n, steps, 0.1)
    oc = Adam(mc.store, mc.cfg.d_model, beta1=B1, beta2=B2, eps=EPS, lr=LR, global_clipnorm=clip)
    ou = Adam(mu.store, mu.cfg.d_model, beta1=B1, beta2=B2, eps=EPS, lr=LR)
    assert oc.clip_on and not ou.clip_on
    p0 = mc.store.flat.clone()
    norms32 = []
    for g in grads:
        mc.store.flat_grad.copy_(g)
        mu.store.flat_grad.copy_(g)
        assert oc.apply(grad_scale)
        ou.apply(grad_scale)
        norms32.append(oc.last_grad_norm())
        assert not mc.store.flat_grad.any()  # consumed gradient zeroed
    p, m, v, norms = _formula64(p0, grads, clip, grad_scale)
    assert oc.iterations == steps
    for got, want in zip(norms32, norms):
        assert abs(got - want) <= 1e-6 * want
    if clip > max(norms):
        # factor exactly 1.0f: bitwise the unclipped update
        assert torch.equal(mc.store.flat, mu.store.flat)
        assert torch.equal(oc.m, ou.m) and torch.equal(oc.v, ou.v)
        assert oc.clip_counters()["clipped_steps"] == 0
    else:
        assert clip < min(norms)
        assert not torch.equal(mc.store.flat, mu.store.flat)
        assert oc.clip_counters()["clipped_steps"] == steps
    # f32 update against float64. The moments are sums that cancel, so their
    # error is absolute: each of the `steps` updates rounds a few times at the
    # size of the largest (clipped) gradient element, 2^-24 relative each
    gmax = max(float(g.abs().max()) for g in grads) * grad_scale * min(1.0, clip / min(norms))
    ulp = 2.0 ** -24
    assert torch.allclose(oc.m.double(), m, rtol=1e-5, atol=4 * steps * ulp * gmax)
    assert torch.allclose(oc.v.double(), v, rtol=1e-5, atol=4 * steps * ulp * gmax * gmax)
    # weights ~ 1e-1 and below, each step's update <= lr_t ~ LR: rounding at
    # the weight's own size plus the update's relative error
    assert torch.allclose(mc.store.flat.double(), p, rtol=1e-6, atol=1e-5 * LR * steps)
    c = oc.clip_counters()
    assert c["skipped_steps"] == 0
    assert abs(c["grad_norm_max"] - max(norms)) <= 1e-6 * max(norms)
    oc.reset_norm_max()
    assert oc.clip_counters()["grad_norm_max"] == 0.0
    assert oc.clip_counters()["clipped_steps"] == c["clipped_steps"]  # counts are kept


def test_cpu_adam_rejects_bad_clipnorm():
    m = _model()
    for bad in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            Adam(m.store, m.cfg.d_model, global_clipnorm=bad)


@pytest.mark.parametrize("bad", [float("inf"), float("nan")], ids=["inf", "nan"])
@pytest.mark.parametrize("clip", [0.0, 0.5], ids=["skip_only", "skip_and_clip"])
def test_cpu_adam_skip_nonfinite(bad, clip):
    ms, mr = _model(), _model()
    n = ms.store.total
    g1, g2, g3 = _grads(n, 3, 0.1)
    kw = dict(beta1=B1, beta2=B2, eps=EPS, lr=LR, global_clipnorm=clip)
    osk = Adam(ms.store, ms.cfg.d_model, skip_nonfinite=True, **kw)
    oref = Adam(mr.store, mr.cfg.d_model, skip_nonfinite=True, **kw)  # never sees the bad step
    for o, mod in ((osk, ms), (oref, mr)):
        mod.store.flat_grad.copy_(g1)
        o.apply()
    before = [t.clone() for t in (ms.store.flat, osk.m, osk.v)]
    g2[n // 3] = bad
    ms.store.flat_grad.copy_(g2)
    assert osk.apply()
    assert torch.equal(ms.store.flat, before[0])
    assert torch.equal(osk.m, before[1]) and torch.equal(osk.v, before[2])
    assert osk.iterations == 1
    assert not ms.store.flat_grad.any()  # the bad gradient is still consumed
    c = osk.clip_counters()
    assert c["skipped_steps"] == 1
    assert not math.isfinite(osk.last_grad_norm())
    assert math.isfinite(c["grad_norm_max"])  # the maximum is over finite norms
    for o, mod in ((osk, ms), (oref, mr)):
        mod.store.flat_grad.copy_(g3)
        o.apply()
    assert osk.iterations == 2 and oref.iterations == 2
    assert torch.equal(ms.store.flat, mr.store.flat)
    assert torch.equal(osk.m, oref.m) and torch.equal(osk.v, oref.v)
    assert osk.clip_counters()["skipped_steps"] == 1 and oref.clip_counters()["skipped_steps"] == 0


def test_cpu_adam_skip_in_ranges_does_not_advance_step():
    """The data-parallel form: per-range norm sums, one finalize, per-range
    updates, advance_step() -- a skipped step advances nothing."""
    m = _model()
    n = m.store.total
    cut = (n // 2) // 64 * 64
    o = Adam(m.store, m.cfg.d_model, lr=LR, skip_nonfinite=True)
    p0 = m.store.flat.clone()
    for bad, want_iter in ((True, 0), (False, 1)):
        g = _grads(n, 1, 0.1)[0]
        if bad:
            g[5] = float("inf")
        m.store.flat_grad.copy_(g)
        for a, b in ((0, cut), (cut, n)):
            o.accumulate_norm(a, b)
        o.finalize_norm()
        for a, b in ((0, cut), (cut, n)):
            o.apply_range(a, b, inc_step=False)
        o.advance_step()
        assert o.iterations == want_iter
        assert torch.equal(m.store.flat, p0) == bad
        assert not m.store.flat_grad.any()


def test_settings_parse_clip_keys():
    s = load_settings()
    assert s.global_clipnorm == 0.0 and s.skip_nonfinite is False  # both off by default
    s = load_settings(overrides=["global_clipnorm=0.5", "skip_nonfinite=true"])
    assert s.global_clipnorm == 0.5 and s.skip_nonfinite is True


# ---------------------------------------------------------------- two gloo ranks
STEPS = 3
# (eps = 1: the update stays ~linear in the gradient, tests/test_parallel_cpu.py)
DP_ADAM = dict(lr=0.05, eps=1.0)
DP_CLIP = 1e-3  # far below the tiny model's gradient norm (~1e-1 and above)


def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _data(rank, world):
    return SyntheticPairs(4, 10, 11, 60, 50, seed=3, rank=rank, world=world, min_len=3)


def _worker(rank, world, port, out, overlap_opt):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from tensorflow_distributed_on_gke_amd.train import step as step_mod
    step_mod.DP_OVERLAP_OPT = overlap_opt
    torch.set_num_threads(2)
    from tensorflow_distributed_on_gke_amd.parallel import dist as tdist
    from tensorflow_distributed_on_gke_amd.parallel.ddp import DataParallel
    from tensorflow_distributed_on_gke_amd.train.step import TrainStep

    tdist.init_distributed("cpu")
    m = Transformer(model_config("tiny", **CFG)).build("cpu", seed=1 + rank)
    opt = Adam(m.store, m.cfg.d_model, global_clipnorm=DP_CLIP, **DP_ADAM)
    ddp = DataParallel(m.store, bucket_mb=0.05)
    ddp.broadcast_params(0)
    step = TrainStep(m, opt, ddp, workers=world, seed=5)
    assert ddp.opt is opt and ddp._upd_stream is None
    early = []  # no span may be updated before the whole norm is known
    data = _data(rank, world)
    norms = []
    for i in range(STEPS):
        apply_range, seen = opt.apply_range, []

        def spy(a, b, *args, _f=apply_range, _seen=seen, **kw):
            _seen.append(opt._nparts if m.store.flat.is_cuda else float(opt._sumsq))
            return _f(a, b, *args, **kw)

        opt.apply_range = spy
        step(*data.batch(i))
        opt.apply_range = apply_range
        early.append(any(s != 0 for s in seen))  # every Adam ran after finalize_norm()
        ddp.verify_replicas()
        norms.append(opt.last_grad_norm())
    torch.save({"flat": m.store.flat.clone(), "norms": torch.tensor(norms, dtype=torch.float64),
                "nb": len(ddp.last_buckets), "iters": opt.iterations, "early": early,
                "counters": opt.clip_counters()}, f"{out}.{rank}")
    ddp.close()
    tdist.barrier()
    tdist.shutdown()


def _single_process(world, clip):
    m = _model()
    opt = Adam(m.store, m.cfg.d_model, global_clipnorm=clip, **DP_ADAM)
    datas = [_data(r, world) for r in range(world)]
    norms = []
    for i in range(STEPS):
        for r in range(world):
            rt = RunCtx(training=True, dropout=0.0, seed=5, ctr=torch.zeros(1, dtype=torch.int64),
                        accumulate=r > 0)
            m.loss_and_backward(*datas[r].batch(i), rt, float(world))
        norms.append(float(m.store.flat_grad.double().norm()))
        opt.apply()
    return m.store.flat, norms


@pytest.mark.parametrize("overlap_opt", ["tail", "1"])
def test_dp2_clip_replicas_identical(tmp_path, overlap_opt):
    """Two ranks: the factor comes from the norm of the summed gradient, so
    both compute the same one and the replicas stay bitwise equal; the
    mid-backward optimizer mode ("1") behaves as "tail"."""
    world = 2
    out = str(tmp_path / "res")
    mp.start_processes(_worker, args=(world, _free_port(), out, overlap_opt), nprocs=world, join=True,
                       start_method="spawn")
    r0 = torch.load(out + ".0", weights_only=True)
    r1 = torch.load(out + ".1", weights_only=True)
    assert r0["nb"] > 3  # several spans, launched from inside backward
    assert torch.equal(r0["flat"], r1["flat"])
    assert torch.equal(r0["norms"], r1["norms"])  # the same grad_norm on both ranks
    assert r0["iters"] == STEPS and r0["early"] == [False] * STEPS
    assert r0["counters"]["clipped_steps"] == STEPS and r0["counters"]["skipped_steps"] == 0
    ref_flat, ref_norms = _single_process(world, DP_CLIP)
    assert min(ref_norms) > 50 * DP_CLIP
    assert torch.allclose(r0["norms"], torch.tensor(ref_norms, dtype=torch.float64), rtol=1e-5)
    assert torch.allclose(r0["flat"], ref_flat, atol=1e-6, rtol=1e-5)
    # (the clipped update is small: also relative to how far the weights moved)
    moved = (ref_flat - _model().store.flat).double().norm()
    assert moved > 0
    assert (r0["flat"] - ref_flat).double().norm() <= 1e-4 * moved
    unclipped, _ = _single_process(world, 0.0)
    assert not torch.allclose(r0["flat"], unclipped, atol=1e-6, rtol=1e-5)


def _train_cli(tmp, *sets):
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mf = os.path.join(tmp, "metrics.jsonl")
    cmd = [sys.executable, "-m", "tensorflow_distributed_on_gke_amd", "train", "--config",
           os.path.join(root, "configuration", "settings.yaml"), "--device", "cpu"]
    for kv in ["preset=tiny", "steps_per_epoch=2", "log_every=1", "local_batch_size=2", "src_len=8",
               "tgt_len=8", "src_vocab=100", "tgt_vocab=100", "snapshot_every_epochs=0",
               "validation_steps=1", "epochs=1", "resume=false", f"metrics_file={mf}", *sets]:
        cmd += ["--set", kv]
    r = subprocess.run(cmd, cwd=tmp, env=dict(os.environ, PYTHONPATH=root), capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(mf) as f:
        return r.stdout, [json.loads(line) for line in f]


def test_train_records_gain_clip_fields_only_when_on(tmp_path):
    """The JSONL `train` / `epoch` records carry grad_norm, grad_norm_max,
    clipped_steps, skipped_steps with either setting on and are as before
    with both off; the reference log lines are the same either way."""
    extra = {"grad_norm", "grad_norm_max", "clipped_steps", "skipped_steps"}
    (tmp_path / "off").mkdir()
    (tmp_path / "on").mkdir()
    out_off, off = _train_cli(str(tmp_path / "off"))
    out_on, on = _train_cli(str(tmp_path / "on"), "global_clipnorm=0.001", "skip_nonfinite=true")
    assert [r["kind"] for r in on] == [r["kind"] for r in off] == ["train", "train", "epoch"]
    for a, b in zip(off, on):
        assert not extra & set(a)
        assert set(b) == set(a) | extra
        assert b["grad_norm"] > 0.001 and b["skipped_steps"] == 0
    assert [r["clipped_steps"] for r in on] == [1, 2, 2]
    # the maximum is since the previous record: each train record's is its one
    # step's own norm, and no step ran between the last of them and the epoch's
    assert [r["grad_norm_max"] for r in on] == [on[0]["grad_norm"], on[1]["grad_norm"], 0.0]
    assert on[2]["grad_norm"] == on[1]["grad_norm"]
    logline = [ln.split(" Loss ")[0] for ln in out_off.splitlines() if ln.startswith("Epoch 1")]
    assert logline == [ln.split(" Loss ")[0] for ln in out_on.splitlines() if ln.startswith("Epoch 1")]
