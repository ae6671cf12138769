"""What the weight EMA costs per training step on one GPU.

Builds two TrainSteps directly (Transformer-base, batch 64, sequence 128 by
default): one with Adam's defaults, one with ema_decay on, captures each into
its HIP graph and times replays of the two, interleaved round by round in one
process, with a device synchronise around every timed window. Also times the
EMA kernel alone (whole-buffer updates; a HIP graph of repeated updates
between device events) against its floor, 12 B x parameters (8 read, 4
written) at the HBM rate.

  python scripts/ema_cost.py [--rounds 7] [--steps 40] [--out FILE]

Needs a GPU; there is no CPU fallback.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tensorflow_distributed_on_gke_amd.data.synthetic import SyntheticPairs  # noqa: E402
from tensorflow_distributed_on_gke_amd.models.transformer import Transformer, model_config  # noqa: E402
from tensorflow_distributed_on_gke_amd.train.optim import Adam  # noqa: E402
from tensorflow_distributed_on_gke_amd.train.step import TrainStep  # noqa: E402

HBM_TBS = 6.3  # achievable HBM3E rate of one MI355X (8.0 peak), TB/s


def build(args, **opt_kw):
    cfg = model_config(args.preset, max_src_len=max(1000, args.seq_len), max_tgt_len=max(1000, args.seq_len))
    model = Transformer(cfg).build("cuda", seed=args.seed)
    opt = Adam(model.store, cfg.d_model, **opt_kw)
    fp8_state = None
    if args.dtype == "fp8":
        from tensorflow_distributed_on_gke_amd.ops.fp8 import Fp8State
        fp8_state = Fp8State(model)
    step = TrainStep(model, opt, None, workers=1, seed=args.seed + 17, fp8_state=fp8_state)
    return cfg, model, opt, step


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="base")
    ap.add_argument("--local-batch", type=int, default=64)
    ap.add_argument("--seq-len", type=int, default=128)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp8"])
    ap.add_argument("--decay", type=float, default=0.999)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=40, help="timed replays per arm and round")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the report here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ema_cost.py needs a GPU")

    arms = {}
    for name, kw in (("off", {}), ("on", dict(ema_decay=args.decay, ema_warmup=True))):
        cfg, model, opt, step = build(args, **kw)
        arms[name] = (model, opt, step)
    S = T = args.seq_len
    data = SyntheticPairs(batch=args.local_batch, src_len=S, tgt_len=T + 1, src_vocab=cfg.src_vocab,
                          tgt_vocab=cfg.tgt_vocab, seed=args.seed, pin=True)
    batches = [tuple(t.cuda() for t in data.batch(i)) for i in range(4)]
    for name, (_, _, step) in arms.items():
        assert step.capture(*batches[0]), name
        for i in range(args.warmup):
            step(*batches[i % len(batches)])
    torch.cuda.synchronize()

    ms = {k: [] for k in arms}
    for _ in range(args.rounds):
        for name, (_, _, step) in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.steps):
                step(*batches[i % len(batches)])
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / args.steps * 1e3)

    # the kernel alone: REP whole-buffer updates per graph replay between device events
    model, opt, _ = arms["on"]
    ema = opt.ema
    updates = ema.updates
    REP, REPLAYS = 20, 10
    saved = (ema.avg.clone(), ema.count.clone())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(REP):
            ema.update()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ema_us = []
    for _ in range(REPLAYS):
        e0.record()
        g.replay()
        e1.record()
        e1.synchronize()
        ema_us.append(e0.elapsed_time(e1) / REP * 1e3)
    ema.avg.copy_(saved[0])
    ema.count.copy_(saved[1])
    torch.cuda.synchronize()

    total = model.store.total
    floor_us = total * 12 / (HBM_TBS * 1e12) * 1e6
    med = {k: statistics.median(v) for k, v in ms.items()}
    kern = statistics.median(ema_us)
    lines = [
        f"ema_cost: transformer-{args.preset} {args.dtype}, batch {args.local_batch}, seq {S}, "
        f"{total} f32 parameters ({total * 4 / 1e6:.1f} MB), {torch.cuda.get_device_name(0)}",
        f"captured step, {args.rounds} interleaved rounds x {args.steps} replays per arm "
        "(host clock around a device synchronise):",
    ]
    for k in arms:
        lines.append(f"  EMA {k:3s}: median {med[k]:.4f} ms/step  (min {min(ms[k]):.4f}, max {max(ms[k]):.4f};"
                     f" rounds: {' '.join(f'{x:.4f}' for x in ms[k])})")
    spread = max(max(v) - min(v) for v in ms.values())
    lines += [
        f"  on - off: {(med['on'] - med['off']) * 1e3:+.1f} us/step = "
        f"{(med['on'] - med['off']) / med['off'] * 100:+.2f} % of the step (largest within-arm spread "
        f"{spread * 1e3:.1f} us)",
        f"EMA kernel alone (ema_kernel + count advance, plain stores, {REP} updates per graph replay, device "
        f"events, {REPLAYS} replays): median {kern:.1f} us  (min {min(ema_us):.1f}, max {max(ema_us):.1f})",
        f"  floor: 12 B x {total} at {HBM_TBS} TB/s = {floor_us:.1f} us; measured / floor = {kern / floor_us:.2f}; "
        f"{total * 12 / (kern * 1e-6) / 1e12:.2f} TB/s",
        "  (back-to-back updates re-read two buffers, part of which the 256 MB Infinity Cache may hold; in",
        "   the step the weights were just written by Adam and the average was last touched a step ago)",
        f"EMA arm: {updates} updates before the kernel timing, decay {args.decay} with warm-up",
    ]
    report = "\n".join(lines)
    print(report, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
