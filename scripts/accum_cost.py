"""What a micro-batch of gradient accumulation costs on one GPU.

Builds one TrainStep per accum_steps = N in (1, 2, 4, 8) directly
(Transformer-base, micro-batch 64, sequence 128 by default), captures each
update's micro-batches into HIP graphs and times whole updates, the arms
interleaved round by round in one process, with a device synchronise around
every timed window. Reports ms per update and per micro-batch next to
N x (the N = 1 step): the expectation is that every micro-batch beyond the
first costs one step minus the optimizer pass (Adam's 30 B per parameter).

  python scripts/accum_cost.py [--rounds 7] [--updates 24] [--loss-mode replica_mean] [--out FILE]

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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="base")
    ap.add_argument("--local-batch", type=int, default=64, help="sentences per micro-batch")
    ap.add_argument("--seq-len", type=int, default=128)
    ap.add_argument("--accum", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--loss-mode", default="replica_mean", choices=["replica_mean", "global_mean"])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--updates", type=int, default=24, help="micro-batches per arm and round (a multiple of every N)")
    ap.add_argument("--warmup", type=int, default=8, help="warm-up micro-batches per arm")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the report here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("accum_cost.py needs a GPU")
    if 1 not in args.accum or any(args.updates % n for n in args.accum):
        sys.exit("--accum must hold 1 and --updates must be a multiple of every N")

    cfg = model_config(args.preset, max_src_len=max(1000, args.seq_len), max_tgt_len=max(1000, args.seq_len))
    S = T = args.seq_len
    data = SyntheticPairs(batch=args.local_batch, src_len=S, tgt_len=T + 1, src_vocab=cfg.src_vocab,
                          tgt_vocab=cfg.tgt_vocab, seed=args.seed, pin=True)
    batches = [tuple(t.cuda() for t in data.batch(i)) for i in range(8)]
    arms = {}
    for n in args.accum:
        model = Transformer(cfg).build("cuda", seed=args.seed)
        opt = Adam(model.store, cfg.d_model)
        step = TrainStep(model, opt, None, workers=1, seed=args.seed + 17, loss_mode=args.loss_mode,
                         accum_steps=n)
        assert step.capture(*batches[0]), n
        arms[n] = (model, opt, step)

    def run(n: int, micro: int) -> None:
        step = arms[n][2]
        for u in range(micro // n):
            step.update([batches[(u * n + k) % len(batches)] for k in range(n)])

    for n in arms:
        run(n, max(n, args.warmup // n * n))
    torch.cuda.synchronize()
    ms = {n: [] for n in arms}  # per update
    for _ in range(args.rounds):
        for n in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(n, args.updates)
            torch.cuda.synchronize()
            ms[n].append((time.perf_counter() - t0) / (args.updates // n) * 1e3)

    total = arms[1][0].store.total
    med = {n: statistics.median(v) for n, v in ms.items()}
    base = med[1]
    lines = [
        f"accum_cost: transformer-{args.preset} bf16, micro-batch {args.local_batch}, seq {S}, "
        f"loss_mode {args.loss_mode}, {total} f32 parameters, {torch.cuda.get_device_name(0)}",
        f"captured updates (one HIP graph per micro-batch), {args.rounds} interleaved rounds x "
        f"{args.updates} micro-batches per arm (host clock around a device synchronise):",
        "   N  ms/update  ms/micro-batch  N x (N=1 step)  saved/update  per extra micro-batch  (min .. max per update)",
    ]
    for n in arms:
        extra = (med[n] - base) / (n - 1) if n > 1 else float("nan")
        lines.append(f"  {n:2d}  {med[n]:9.4f}  {med[n] / n:14.4f}  {n * base:14.4f}  "
                     f"{(n * base - med[n]) * 1e3:9.1f} us  "
                     + (f"{extra:9.4f} ms = step {(extra - base) * 1e3:+7.1f} us" if n > 1 else " " * 32)
                     + f"  ({min(ms[n]):.4f} .. {max(ms[n]):.4f})")
    adam_floor = total * 30 / (HBM_TBS * 1e12) * 1e6
    spread = max(max(v) - min(v) for v in ms.values())
    lines += [
        f"largest within-arm spread {spread * 1e3:.1f} us per update",
        f"the optimizer pass an extra micro-batch does not run: Adam, 30 B x {total} at {HBM_TBS} TB/s "
        f"= {adam_floor:.1f} us at the floor",
        f"tokens per update at N = {max(arms)}: {max(arms) * args.local_batch * (S + T)}",
    ]
    report = "\n".join(lines)
    print(report, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
