"""What the n-gram match kernel and MBR selection cost on one GPU.

Times the kernel alone (ngram_matches, a HIP graph of repeated launches between
device events) on the pairs of an MBR selection, 32 groups x 64 candidates =
64 512 unordered pairs, of 32, 64 and 128 random tokens from a 1000-word
vocabulary, in both variants: the ranks of x computed inside the pair kernel,
and read from a per-row pre-pass (its launch included); the two variants again
on the pairs of a corpus BLEU, where every row is in one pair. Against them,
on the same tensors in the same run: the torch composition the kernel replaces
(`ngram_matches_torch`: a broadcast equality tensor per pair, shifted ANDs for
n = 2..4, rank / count sums, chunked to fit memory; it synchronises with the
host, so it is timed eagerly between device events, not in a graph), and the
CPU `Counter` reference on a subsample of the pairs, extrapolated to all. Then
times `Tester.decode(sample=16, mbr=True)` against `sample=16` alone on a
random-init model (Transformer-base by default), 32 sentences, 32 steps,
interleaved round by round, a host clock around a device synchronise.

  python scripts/mbr_cost.py [--rounds 5] [--out FILE]

Needs a GPU; there is no CPU fallback.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tensorflow_distributed_on_gke_amd.infer.greedy import Tester  # noqa: E402
from tensorflow_distributed_on_gke_amd.infer.tokenizer import ByteTokenizer  # noqa: E402
from tensorflow_distributed_on_gke_amd.models.transformer import Transformer, model_config  # noqa: E402
from tensorflow_distributed_on_gke_amd.ops._ext import C  # noqa: E402
from tensorflow_distributed_on_gke_amd.ops.kernels.overlap import ngram_matches_torch  # noqa: E402

LENGTHS = (32, 64, 128)


def counter_matches(x, y):
    out = []
    for n in range(1, 5):
        cx = Counter(tuple(x[i:i + n]) for i in range(len(x) - n + 1))
        cy = Counter(tuple(y[i:i + n]) for i in range(len(y) - n + 1))
        out.append(sum((cx & cy).values()))
    return out


def graph_us(fn, rep, replays):
    """Median, min, max us per call of `fn`, `rep` calls per graph replay."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(rep):
            fn()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    us = []
    for _ in range(replays):
        e0.record()
        g.replay()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) / rep * 1e3)
    return statistics.median(us), min(us), max(us)


def eager_us(fn, calls):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    us = []
    for _ in range(calls):
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(us), min(us), max(us)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="base")
    ap.add_argument("--groups", type=int, default=32)
    ap.add_argument("--cands", type=int, default=64)
    ap.add_argument("--vocab", type=int, default=1000)
    ap.add_argument("--rep", type=int, default=10, help="launches per graph replay")
    ap.add_argument("--cpu-pairs", type=int, default=500, help="pairs of the Counter timing")
    ap.add_argument("--bleu-lines", type=int, default=32768, help="line pairs of the corpus BLEU shape")
    ap.add_argument("--sentences", type=int, default=32)
    ap.add_argument("--sample", type=int, default=16)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the report here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mbr_cost.py needs a GPU")

    B, n = args.groups, args.cands
    gen = torch.Generator().manual_seed(args.seed)
    iu = torch.triu_indices(n, n, 1)
    base = (torch.arange(B) * n).view(B, 1)
    pa = (base + iu[0]).reshape(-1).to(torch.int32).cuda()
    pb = (base + iu[1]).reshape(-1).to(torch.int32).cuda()
    P = pa.numel()
    lines = [
        f"mbr_cost: {torch.cuda.get_device_name(0)}",
        f"n-gram match kernel alone, {B} groups x {n} candidates = {P} pairs of L random tokens from a "
        f"{args.vocab}-word vocabulary; kernel: {args.rep} launches per graph replay, device events, 10 replays; "
        "torch composition: eager, device events, 3 calls; Counter: host clock, extrapolated from "
        f"{args.cpu_pairs} pairs",
    ]
    for L in LENGTHS:
        tok = torch.randint(0, args.vocab, (B * n, L), generator=gen, dtype=torch.int32)
        length = torch.full((B * n,), L, dtype=torch.int32)
        t0 = time.perf_counter()
        sub = [counter_matches(tok[a].tolist(), tok[b].tolist())
               for a, b in zip(pa[:args.cpu_pairs].tolist(), pb[:args.cpu_pairs].tolist())]
        cpu_s = (time.perf_counter() - t0) / args.cpu_pairs * P
        tok, length = tok.cuda(), length.cuda()
        out = torch.empty(P, 4, dtype=torch.int32, device="cuda")
        out_pre = torch.empty(P, 4, dtype=torch.int32, device="cuda")
        ranks = torch.empty(B * n, L, 4, dtype=torch.int16, device="cuda")
        inside = graph_us(lambda: C().ngram_matches(tok, length, pa, pb, out, None), args.rep, 10)
        pre = graph_us(lambda: C().ngram_matches(tok, length, pa, pb, out_pre, ranks), args.rep, 10)
        comp = eager_us(lambda: ngram_matches_torch(tok, length, pa, pb), 3)
        ref = ngram_matches_torch(tok, length, pa, pb)
        same = (torch.equal(out, ref) and torch.equal(out_pre, ref)
                and out[:args.cpu_pairs].tolist() == sub)
        lines.append(
            f"  L {L:3d}: ranks in the pair kernel median {inside[0]:.1f} us (min {inside[1]:.1f}, max "
            f"{inside[2]:.1f}); ranks from the pre-pass median {pre[0]:.1f} us (min {pre[1]:.1f}, max "
            f"{pre[2]:.1f}); torch composition median {comp[0] / 1e3:.1f} ms (min {comp[1] / 1e3:.1f}, max "
            f"{comp[2] / 1e3:.1f}) = {comp[0] / inside[0]:.0f} x the kernel; Counter on the host about "
            f"{cpu_s:.1f} s = {cpu_s * 1e6 / inside[0]:.0f} x; all four agree exactly: {same}")
    del tok, out, out_pre, ranks

    # the shape of corpus BLEU: every row in one pair only, (k, N + k)
    N = args.bleu_lines
    tok = torch.randint(0, args.vocab, (2 * N, 32), generator=gen, dtype=torch.int32).cuda()
    length = torch.full((2 * N,), 32, dtype=torch.int32, device="cuda")
    ka = torch.arange(N, dtype=torch.int32, device="cuda")
    kb = ka + N
    out = torch.empty(N, 4, dtype=torch.int32, device="cuda")
    ranks = torch.empty(2 * N, 32, 4, dtype=torch.int16, device="cuda")
    inside = graph_us(lambda: C().ngram_matches(tok, length, ka, kb, out, None), args.rep, 10)
    pre = graph_us(lambda: C().ngram_matches(tok, length, ka, kb, out, ranks), args.rep, 10)
    lines.append(f"corpus BLEU's pairs, {N} (hypothesis, reference) lines of 32 tokens, each row in one pair: ranks "
                 f"in the pair kernel median {inside[0]:.1f} us (min {inside[1]:.1f}, max {inside[2]:.1f}); ranks "
                 f"from the pre-pass median {pre[0]:.1f} us (min {pre[1]:.1f}, max {pre[2]:.1f})")
    del tok, out, ranks

    cfg = model_config(args.preset)
    model = Transformer(cfg).build("cuda", seed=args.seed)
    tester = Tester(ByteTokenizer(min(cfg.src_vocab, cfg.tgt_vocab)), model)
    src = torch.randint(4, cfg.src_vocab, (args.sentences, 24), generator=gen)
    mode = dict(max_length=args.steps, sample=args.sample, seed=args.seed)
    arms = {"sample alone": lambda: tester.decode(src, **mode),
            "sample + mbr": lambda: tester.decode(src, mbr=True, **mode)}
    for f in arms.values():  # warm-up: every shape of the timed window
        f()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(args.rounds):
        for k, f in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    lines.append(f"Tester.decode, transformer-{args.preset} (random init), {args.sentences} sentences x "
                 f"{args.sample} samples, {args.steps} steps, whole call (copy to the host included), "
                 f"{args.rounds} interleaved rounds (host clock around a device synchronise):")
    for k in arms:
        lines.append(f"  {k}: median {statistics.median(ms[k]):.2f} ms (min {min(ms[k]):.2f}, max "
                     f"{max(ms[k]):.2f})")
    a, b = statistics.median(ms["sample alone"]), statistics.median(ms["sample + mbr"])
    lines.append(f"  mbr adds {b - a:+.2f} ms = {100.0 * (b - a) / b:.1f} % of the call")
    report = "\n".join(lines)
    print(report, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
