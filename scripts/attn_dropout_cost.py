"""What attention dropout costs on one GPU.

(a) The attention kernels alone, p = 0 against p = 0.1 (the DROP variants,
    csrc/kernels/attn_impl.h), hd 64, self-attention without padding:
    forward and fused backward at B 64, H 8, L 128; forward and backward at
    B 16, H 16, L 512, where p = 0 runs the LDS-DMA pipelined kernels and
    p = 0.1 the register-staged forward and the split dQ / dK,dV pair (the
    pipelined kernels have no DROP variant). One call per graph replay
    between device events; the arm each call took is printed.
(b) The training step (Transformer-base by default, bf16, one HIP graph) with
    attention_dropout 0 and 0.1 on the same batches, interleaved round by
    round in one process: the mask and the lost projection + attention fusion
    together.

  python scripts/attn_dropout_cost.py [--rounds 5] [--out FILE]

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
from tensorflow_distributed_on_gke_amd.ops import kernels as K  # noqa: E402
from tensorflow_distributed_on_gke_amd.ops._ext import C  # noqa: E402
from tensorflow_distributed_on_gke_amd.train.optim import Adam  # noqa: E402
from tensorflow_distributed_on_gke_amd.train.step import TrainStep  # noqa: E402

P = 0.1
FAMILY = {0: "fwd64", 1: "fwd128", 2: "fwd128w8", 3: "fwd_pipe", 5: "bwd_fused", 6: "bwd_fdo", 7: "bwd_split",
          8: "bwd_pipe"}


def capture(fn):
    """`fn` as a one-call graph, replayed 20 times (clocks up, code loaded)."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    for _ in range(20):
        g.replay()
    torch.cuda.synchronize()
    return g


def replay_us(g, replays):
    """us of each of `replays` replays of g, between device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    us = []
    for _ in range(replays):
        e0.record()
        g.replay()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    return us


def kernel_part(args, lines) -> None:
    lines.append(f"(a) attention kernels alone, hd 64, no padding, causal off, p = 0 against p = {P}; one call per "
                 f"graph replay, device events, {args.rounds} interleaved rounds of {args.replays} replays after 20 "
                 "untimed ones; us median (min, max) [arm]:")
    ctr = torch.tensor([1], dtype=torch.int64, device="cuda")
    for B, H, L in ((64, 8, 128), (16, 16, 512)):
        g = torch.Generator().manual_seed(args.seed)
        q, k, v, do = (torch.randn(B, L, H, 64, generator=g).to(torch.bfloat16).cuda() for _ in range(4))
        dq, dk, dv = (torch.empty_like(q) for _ in range(3))
        scale = 0.125
        for name in ("forward", "backward"):
            row, graphs = {}, {}
            for p in (0.0, P):
                drop = (p, 7, ctr, 2049) if p else None
                o, lse = K.attn_fwd(q, k, v, None, scale, False, drop=drop)
                if name == "forward":
                    fn = lambda: K.attn_fwd(q, k, v, None, scale, False, drop=drop)  # noqa: E731
                else:
                    fn = lambda: K.attn_bwd(q, k, v, o, do, lse, dq, dk, dv, None, scale, False, drop=drop)  # noqa: E731
                graphs[p] = (capture(fn), FAMILY.get(int(C().attn_last_plan()[0]), "?"), [])
            for _ in range(args.rounds):
                for p, (gr, _, us) in graphs.items():
                    us += replay_us(gr, args.replays)
            for p, (_, arm, us) in graphs.items():
                row[p] = ((statistics.median(us), min(us), max(us)), arm)
            (t0, a0), (t1, a1) = row[0.0], row[P]
            lines.append(f"  B {B} H {H} L {L} {name}: p = 0 {t0[0]:.1f} ({t0[1]:.1f}, {t0[2]:.1f}) [{a0}]   p = {P} "
                         f"{t1[0]:.1f} ({t1[1]:.1f}, {t1[2]:.1f}) [{a1}]   {t1[0] / t0[0]:.2f} x, + {t1[0] - t0[0]:.1f} us")


def step_part(args, lines) -> None:
    arms = {}
    for p in (0.0, P):
        cfg = model_config(args.preset, attention_dropout=p)
        data = SyntheticPairs(batch=args.batch, src_len=args.seq, tgt_len=args.seq + 1, src_vocab=cfg.src_vocab,
                              tgt_vocab=cfg.tgt_vocab, min_len=args.seq // 2, seed=args.seed)
        batches = [tuple(t.cuda() for t in data.batch(i)) for i in range(4)]
        m = Transformer(cfg).build("cuda", seed=args.seed)
        step = TrainStep(m, Adam(m.store, cfg.d_model), None, workers=1.0)
        assert step.capture(*batches[0])
        arms[p] = step
    ms = {n: [] for n in arms}
    for _ in range(args.rounds):
        for n, step in arms.items():
            for b in batches[:2]:
                step(*b)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.steps):
                step(*batches[i % len(batches)])
            torch.cuda.synchronize()
            ms[n].append((time.perf_counter() - t0) / args.steps * 1e3)
    med = {n: statistics.median(v) for n, v in ms.items()}
    lines.append(f"(b) training step, transformer-{args.preset} (random init), batch {args.batch} x seq {args.seq}, "
                 f"bf16, dropout {cfg.dropout}, one HIP graph, {args.steps} steps per timing, {args.rounds} "
                 "interleaved rounds (host clock around a device synchronise):")
    for n in arms:
        lines.append(f"  attention_dropout {n:g}: median {med[n]:.3f} ms/step  (min {min(ms[n]):.3f}, max "
                     f"{max(ms[n]):.3f}; {med[n] / med[0.0]:.3f} x the plain step, + {med[n] - med[0.0]:.3f} ms)")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="base")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seq", type=int, default=128)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--replays", type=int, default=30)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--skip-step", action="store_true", help="only the kernels-alone part")
    ap.add_argument("--out", default=None, help="also write the report here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("attn_dropout_cost.py needs a GPU")
    lines = [f"attn_dropout_cost: {torch.cuda.get_device_name(0)}"]
    kernel_part(args, lines)
    if not args.skip_step:
        step_part(args, lines)
    report = "\n".join(lines)
    print(report, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
