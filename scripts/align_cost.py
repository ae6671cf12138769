"""What word alignment from cross-attention costs on one GPU.

(a) The kernel alone (attn_align, csrc/kernels/attn_align.hip; hard + conf,
    no soft output) at B 64 x H 8 x hd 64 with Lq = Lk in {32, 128, 512} and
    at B 16 x H 16 x hd 64 x 1000, ragged kv_len, against the torch
    composition it replaces: attn_probs (the [B, H, Lq, Lk] f32 tensor),
    mean(1), a masked max. One call per graph replay between device events,
    the arms interleaved round by round; plus the largest |soft - float64
    reference| at the shapes of <= 128 tokens.
(b) align_pairs on Transformer-base (random init), 64 pairs of 128 + 128
    tokens, against score_pairs on the same batch, interleaved, host clock
    around a device synchronise.

  python scripts/align_cost.py [--rounds 5] [--out FILE]

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

from tensorflow_distributed_on_gke_amd.infer.align import align_pairs  # noqa: E402
from tensorflow_distributed_on_gke_amd.infer.score import score_pairs  # noqa: E402
from tensorflow_distributed_on_gke_amd.models.transformer import Transformer, model_config  # noqa: E402
from tensorflow_distributed_on_gke_amd.ops.kernels import attention as KA  # noqa: E402

SHAPES = [(64, 8, 32), (64, 8, 128), (64, 8, 512), (16, 16, 1000)]  # (B, H, L), hd 64


def composition(q, k, kv_len, scale):
    a = KA.attn_probs(q, k, kv_len, scale, False).mean(1)
    keys = torch.arange(k.shape[1], device=q.device).view(1, 1, -1)
    rng = (keys >= 1) & (keys < (kv_len - 1).view(-1, 1, 1))
    return a.masked_fill(~rng, -1.0).max(-1)


def graph(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def replay_us(g, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        g.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def fmt(v):
    return f"median {statistics.median(v):.1f} us  (min {min(v):.1f}, max {max(v):.1f})"


def kernel_part(args, lines) -> None:
    lines.append(f"(a) kernel alone, hd 64, bf16, kv_len uniform in [L / 2, L], k_lo = k_trim = 1; graph replays "
                 f"between device events, {args.replays} replays per timing, {args.rounds} interleaved rounds:")
    for B, H, L in SHAPES:
        g = torch.Generator().manual_seed(args.seed)
        q = torch.randn(B, L, H, 64, generator=g).to(torch.bfloat16).cuda()
        k = torch.randn(B, L, H, 64, generator=g).to(torch.bfloat16).cuda()
        kv_len = torch.randint(L // 2, L + 1, (B,), generator=g, dtype=torch.int32).cuda()
        arms = {"attn_align": graph(lambda: KA.attn_align(q, k, kv_len, 0.125, None, 1, 1)),
                "attn_align + soft": graph(lambda: KA.attn_align(q, k, kv_len, 0.125, None, 1, 1, want_soft=True)),
                "attn_probs, mean, masked max": graph(lambda: composition(q, k, kv_len, 0.125))}
        us = {n: [] for n in arms}
        for _ in range(args.rounds):
            for n, gr in arms.items():
                us[n].append(replay_us(gr, args.replays))
        hard, conf, soft = KA.attn_align(q, k, kv_len, 0.125, None, 1, 1, want_soft=True)
        cv, ci = composition(q, k, kv_len, 0.125)
        same = float((hard == ci).float().mean())
        lines.append(f"  B {B} x H {H} x Lq = Lk = {L}: hard equals the composition's arg-max in {same:.4%} of rows, "
                     f"largest |conf - composition| {float((conf - cv).abs().max()):.2e}")
        for n in arms:
            lines.append(f"    {n}: {fmt(us[n])}" + ("" if n == "attn_align" else
                         f" = {statistics.median(us[n]) / statistics.median(us['attn_align']):.2f} x attn_align"))
        if L <= 128:
            p = torch.softmax((torch.einsum("bqhd,bkhd->bhqk", q.double().cpu(), k.double().cpu()) * 0.125)
                              .masked_fill(torch.arange(L).view(1, 1, 1, L) >= kv_len.cpu().view(B, 1, 1, 1),
                                           -float("inf")), -1).mean(1)
            lines.append(f"    largest |soft - float64 reference| {float((soft.cpu()[..., :L].double() - p).abs().max()):.2e}")


def model_part(args, lines) -> None:
    cfg = model_config(args.preset)
    m = Transformer(cfg).build("cuda", seed=args.seed)
    g = torch.Generator().manual_seed(args.seed)
    B, L = args.batch, args.seq
    src = torch.randint(4, cfg.src_vocab, (B, L), generator=g)
    tgt = torch.randint(4, cfg.tgt_vocab, (B, L + 1), generator=g)
    src[:, 0], src[:, -1], tgt[:, 0], tgt[:, -1] = 2, 3, 2, 3
    src, tgt = src.cuda(), tgt.cuda()
    arms = {"score_pairs": lambda: score_pairs(m, src, tgt), "align_pairs": lambda: align_pairs(m, src, tgt)}
    ms = {n: [] for n in arms}
    for fn in arms.values():
        fn()
    for _ in range(args.rounds):
        for n, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                fn()
            torch.cuda.synchronize()
            ms[n].append((time.perf_counter() - t0) / args.steps * 1e3)
    lines.append(f"(b) transformer-{args.preset} (random init), {B} pairs of {L} + {L} tokens, one teacher-forced "
                 f"forward per call, eager, {args.steps} calls per timing, {args.rounds} interleaved rounds (host "
                 "clock around a device synchronise; align_pairs includes its copy of hard / conf to the host and "
                 "the Python list of links, score_pairs the vocabulary projection and score_tokens):")
    for n in arms:
        lines.append(f"  {n}: median {statistics.median(ms[n]):.3f} ms  (min {min(ms[n]):.3f}, max {max(ms[n]):.3f})")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="base")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seq", type=int, default=128)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the report here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("align_cost.py needs a GPU")
    lines = [f"align_cost: {torch.cuda.get_device_name(0)}"]
    kernel_part(args, lines)
    model_part(args, lines)
    report = "\n".join(lines)
    print(report, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
