"""What the character n-gram kernels and chrF-utility MBR cost on one GPU.

1. The pairs of an MBR selection, 32 groups x 64 candidates = 64 512 unordered
   pairs, of 160 / 320 / 480 / 640 / 2048 characters: `char_ngram_matches`
   (row pre-pass plus pair kernel, six orders) against `ngram_matches` with its
   pre-pass on the same rows (four orders, the lengths it admits) and against
   the torch composition (`char_ngram_matches_torch` on the GPU tensors, timed
   on the first group's pairs and scaled to all: it takes seconds). A group's
   candidates are one random sentence over an English-like letter distribution
   with 15 % of the characters substituted per candidate, which is what samples
   of one source look like: long shared n-grams, the case that keeps the
   searches busy up to the top order.
2. The pairs of a corpus chrF: 32 768 (hypothesis, reference) lines of 160
   characters, every row in one pair, so the pre-pass is not amortised.
3. `Tester.decode(sample=16, mbr=True, mbr_utility="chrf")` against the BLEU
   utility and the samples alone on a random-init model, and the host
   detokenisation of the chrF path on its own.

The kernels are timed as HIP graphs of `--rep` launches between device events,
the arms of a shape interleaved replay by replay; medians with min and max.

  python scripts/chrf_cost.py [--rounds 5] [--out FILE]

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

from tensorflow_distributed_on_gke_amd.infer.chrf import char_units  # noqa: E402
from tensorflow_distributed_on_gke_amd.infer.greedy import Tester  # noqa: E402
from tensorflow_distributed_on_gke_amd.infer.tokenizer import ByteTokenizer  # noqa: E402
from tensorflow_distributed_on_gke_amd.models.transformer import Transformer, model_config  # noqa: E402
from tensorflow_distributed_on_gke_amd.ops._ext import C  # noqa: E402
from tensorflow_distributed_on_gke_amd.ops.kernels.chrf import char_ngram_matches_torch  # noqa: E402

LENGTHS = (160, 320, 480, 640, 2048)
# the relative letter frequencies of English text, in descending order (which letter gets which does not matter)
FREQ = (127, 91, 82, 75, 70, 67, 63, 61, 60, 43, 40, 28, 28, 24, 24, 22, 20, 20, 19, 15, 10, 8, 2, 2, 1, 1)


def similar_rows(groups, cands, L, gen, rate=0.15):
    """int32 [groups * cands, L]: per group one sentence, per candidate `rate` of it substituted."""
    w = torch.tensor(FREQ, dtype=torch.float32)
    draw = lambda n: torch.multinomial(w, n, replacement=True, generator=gen).view(-1, L)
    base = draw(groups * L).repeat_interleave(cands, dim=0)
    swap = torch.rand(groups * cands, L, generator=gen) < rate
    return (torch.where(swap, draw(groups * cands * L), base) + ord("a")).to(torch.int32)


def graphs_us(arms, rep, replays):
    """{name: (median, min, max) us per call}: one graph of `rep` calls per
    arm, the arms' replays interleaved."""
    graphs = {}
    for k, fn in arms.items():
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(rep):
                fn()
        g.replay()
        graphs[k] = g
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    us = {k: [] for k in arms}
    for _ in range(replays):
        for k, g in graphs.items():
            e0.record()
            g.replay()
            e1.record()
            e1.synchronize()
            us[k].append(e0.elapsed_time(e1) / rep * 1e3)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in us.items()}


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


def kernel_arms(chr_, length, pa, pb):
    """The timed calls on one set of rows and pairs, and their outputs."""
    N, L = chr_.shape
    P = pa.numel()
    out6 = torch.empty(P, 6, dtype=torch.int32, device="cuda")
    keys = torch.empty(N, L, 2, dtype=torch.int64, device="cuda")
    ranks8 = torch.empty(N, L, 8, dtype=torch.int16, device="cuda")
    arms = {"chrf": lambda: C().char_ngram_matches(chr_, length, pa, pb, out6, keys, ranks8)}
    out4 = None
    if L <= 512:
        out4 = torch.empty(P, 4, dtype=torch.int32, device="cuda")
        ranks4 = torch.empty(N, L, 4, dtype=torch.int16, device="cuda")
        arms["ngram"] = lambda: C().ngram_matches(chr_, length, pa, pb, out4, ranks4)
    return arms, out6, out4


def fmt(t, unit="us"):
    s = 1e3 if unit == "ms" else 1.0
    return f"median {t[0] / s:.1f} {unit} (min {t[1] / s:.1f}, max {t[2] / s:.1f})"


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="base")
    ap.add_argument("--groups", type=int, default=32)
    ap.add_argument("--cands", type=int, default=64)
    ap.add_argument("--rep", type=int, default=5, help="launches per graph replay")
    ap.add_argument("--replays", type=int, default=10)
    ap.add_argument("--corpus-lines", type=int, default=32768)
    ap.add_argument("--sentences", type=int, default=32)
    ap.add_argument("--sample", type=int, default=16)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the report here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("chrf_cost.py needs a GPU")

    B, n = args.groups, args.cands
    gen = torch.Generator().manual_seed(args.seed)
    iu = torch.triu_indices(n, n, 1)
    base = (torch.arange(B) * n).view(B, 1)
    pa = (base + iu[0]).reshape(-1).to(torch.int32).cuda()
    pb = (base + iu[1]).reshape(-1).to(torch.int32).cuda()
    P, P1 = pa.numel(), iu.shape[1]
    lines = [
        f"chrf_cost: {torch.cuda.get_device_name(0)}",
        f"1. MBR pairs: {B} groups x {n} candidates = {P} pairs of L characters (a group: one sentence of "
        "English-like letters, 15 % substituted per candidate). chrf: char_ngram_matches, pre-pass + pair "
        "kernel, six orders; ngram: ngram_matches with its pre-pass on the same rows, four orders; "
        f"{args.rep} launches per graph replay, device events, {args.replays} replays, the two interleaved. "
        f"torch composition: eager on the first group's {P1} pairs, 3 calls, scaled by {B}",
    ]
    for L in LENGTHS:
        chr_ = similar_rows(B, n, L, gen).cuda()
        length = torch.full((B * n,), L, dtype=torch.int32, device="cuda")
        arms, out6, out4 = kernel_arms(chr_, length, pa, pb)
        t = graphs_us(arms, args.rep, args.replays)
        comp = eager_us(lambda: char_ngram_matches_torch(chr_, length, pa[:P1], pb[:P1]), 3)
        same = torch.equal(out6[:P1], char_ngram_matches_torch(chr_, length, pa[:P1], pb[:P1]))
        line = f"  L {L:4d}: chrf {fmt(t['chrf'])}"
        if out4 is not None:
            same = same and torch.equal(out6[:, :4], out4)
            line += f"; ngram {fmt(t['ngram'])} = {t['ngram'][0] / t['chrf'][0]:.2f} x chrf"
        line += (f"; torch composition about {comp[0] * B / 1e3:.0f} ms = {comp[0] * B / t['chrf'][0]:.0f} x chrf; "
                 f"all agree exactly: {same}")
        lines.append(line)
        print(line, flush=True)
        del chr_, arms, out6, out4

    N = args.corpus_lines
    ref = similar_rows(N, 1, 160, gen)
    swap = torch.rand(N, 160, generator=gen) < 0.15
    hyp = torch.where(swap, similar_rows(N, 1, 160, gen), ref)
    chr_ = torch.cat([hyp, ref]).cuda()
    length = torch.full((2 * N,), 160, dtype=torch.int32, device="cuda")
    ka = torch.arange(N, dtype=torch.int32, device="cuda")
    kb = ka + N
    arms, out6, out4 = kernel_arms(chr_, length, ka, kb)
    t = graphs_us(arms, args.rep, args.replays)
    comp = eager_us(lambda: char_ngram_matches_torch(chr_, length, ka[:2048], kb[:2048]), 3)
    lines.append(f"2. corpus pairs: {N} (hypothesis, reference) lines of 160 characters, each row in one pair: chrf "
                 f"{fmt(t['chrf'])}; ngram {fmt(t['ngram'])} = {t['ngram'][0] / t['chrf'][0]:.2f} x chrf; torch "
                 f"composition (2048 pairs, scaled) about {comp[0] * N / 2048 / 1e3:.0f} ms; agree exactly: "
                 f"{torch.equal(out6[:, :4], out4)}")
    print(lines[-1], flush=True)
    del chr_, arms, out6, out4

    cfg = model_config(args.preset)
    model = Transformer(cfg).build("cuda", seed=args.seed)
    tester = Tester(ByteTokenizer(min(cfg.src_vocab, cfg.tgt_vocab)), model)
    src = torch.randint(4, cfg.src_vocab, (args.sentences, 24), generator=gen)
    mode = dict(max_length=args.steps, sample=args.sample, seed=args.seed)
    drawn = tester.decode(src, **mode)[0]
    arms = {"sample alone": lambda: tester.decode(src, **mode),
            "sample + mbr, bleu": lambda: tester.decode(src, mbr=True, **mode),
            "sample + mbr, chrf": lambda: tester.decode(src, mbr=True, mbr_utility="chrf", **mode),
            "host detokenisation of the chrf path": lambda: [char_units(tester._text(r)[0])
                                                             for c in drawn.tolist() for r in c]}
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
    lines.append(f"3. Tester.decode, transformer-{args.preset} (random init, byte tokenizer), {args.sentences} "
                 f"sentences x {args.sample} samples, {args.steps} steps, whole call (copy to the host included), "
                 f"{args.rounds} interleaved rounds (host clock around a device synchronise):")
    for k in arms:
        lines.append(f"  {k}: median {statistics.median(ms[k]):.2f} ms (min {min(ms[k]):.2f}, max "
                     f"{max(ms[k]):.2f})")
    report = "\n".join(lines)
    print(report, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
