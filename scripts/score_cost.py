"""What teacher-forced scoring costs on one GPU.

Times the scoring kernel alone (score_tokens, a HIP graph of repeated launches
between device events) at rows x V = 8192 x 7010 (row stride 7040) with 1, 2
and 4 members, with and without top_lp, against the torch composition it
replaces on the same tensors in the same run (a float32 log_softmax + log w per
member, a stack, a logsumexp, a gather, and a max for top_lp) and against its
byte floor, members x rows x stride x 2 B at the HBM rate. Then times
`score_pairs` on random-init models (Transformer-base by default), 64 pairs of
128 + 128 tokens, against `Tester.score` on the same batch, interleaved round
by round, a host clock around a device synchronise.

  python scripts/score_cost.py [--rounds 5] [--out FILE]

Needs a GPU; there is no CPU fallback.
"""
from __future__ import annotations

import argparse
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tensorflow_distributed_on_gke_amd.infer.ensemble import Ensemble  # noqa: E402
from tensorflow_distributed_on_gke_amd.infer.greedy import Tester  # noqa: E402
from tensorflow_distributed_on_gke_amd.infer.score import score_pairs  # noqa: E402
from tensorflow_distributed_on_gke_amd.infer.tokenizer import END, START, ByteTokenizer  # noqa: E402
from tensorflow_distributed_on_gke_amd.models.transformer import Transformer, model_config  # noqa: E402
from tensorflow_distributed_on_gke_amd.ops.kernels.decode import score_tokens  # noqa: E402

HBM_TBS = 5.5  # the achievable HBM3E rate the README's floors use, TB/s
SIZES = (1, 2, 4)


def torch_score(logits, V, logw, labels, want_top):
    parts = [torch.log_softmax(x[:, :V].float(), dim=-1) + lw for x, lw in zip(logits, logw)]
    mix = torch.logsumexp(torch.stack(parts), dim=0)
    tok = mix.gather(1, labels.view(-1, 1)).view(-1)
    return tok, (mix.max(dim=1).values if want_top else None)


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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="base")
    ap.add_argument("--pairs", type=int, default=64, help="pairs of the score_pairs timing")
    ap.add_argument("--src-len", type=int, default=128)
    ap.add_argument("--tgt-len", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rows", type=int, default=8192, help="rows of the kernel-alone timing")
    ap.add_argument("--vocab", type=int, default=7010, help="V of the kernel-alone timing")
    ap.add_argument("--stride", type=int, default=7040, help="row stride of the kernel-alone timing")
    ap.add_argument("--rep", type=int, default=20, help="launches per graph replay")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the report here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("score_cost.py needs a GPU")

    R, V, ld = args.rows, args.vocab, args.stride
    g = torch.Generator().manual_seed(args.seed)
    logits = [(torch.randn(R, ld, generator=g) * 4.0).to(torch.bfloat16).cuda() for _ in range(max(SIZES))]
    labels = torch.randint(1, V, (R,), generator=g).cuda()
    lines = [
        f"score_cost: {torch.cuda.get_device_name(0)}",
        f"scoring kernel alone at rows x V = {R} x {V} (row stride {ld}, no pad_id row), {args.rep} launches per "
        "graph replay, device events, 10 replays; the torch composition on the same tensors in the same run",
    ]
    for M in SIZES:
        mem, logw = logits[:M], [math.log(1.0 / M)] * M
        floor_us = M * R * ld * 2 / (HBM_TBS * 1e12) * 1e6
        for want_top in (False, True):
            tok, top = score_tokens(mem, V, labels, want_top=want_top)
            rtok, rtop = torch_score(mem, V, logw, labels, want_top)
            diff = (tok - rtok).abs().max().item()
            if want_top:
                diff = max(diff, (top - rtop).abs().max().item())
            kern = graph_us(lambda: score_tokens(mem, V, labels, want_top=want_top), args.rep, 10)
            comp = graph_us(lambda: torch_score(mem, V, logw, labels, want_top), max(1, args.rep // 4), 10)
            lines.append(
                f"  {M} member{'s' if M > 1 else ' '}, top_lp {'yes' if want_top else 'no '}: score_tokens median "
                f"{kern[0]:.1f} us (min {kern[1]:.1f}, max {kern[2]:.1f}); composition median {comp[0]:.1f} us "
                f"(min {comp[1]:.1f}, max {comp[2]:.1f}); composition / kernel = {comp[0] / kern[0]:.1f}; floor "
                f"{M} x {R} x {ld} x 2 B at {HBM_TBS} TB/s = {floor_us:.1f} us, kernel / floor = "
                f"{kern[0] / floor_us:.2f}; largest |kernel - composition| {diff:.2e}")
    del logits

    cfg = model_config(args.preset)
    models = [Transformer(cfg).build("cuda", seed=args.seed + i) for i in range(2)]
    B, S, T = args.pairs, args.src_len, args.tgt_len
    src = torch.randint(4, cfg.src_vocab, (B, S), generator=g)
    tgt = torch.randint(4, cfg.tgt_vocab, (B, T + 1), generator=g)
    tgt[:, 0], tgt[:, -1] = START, END
    src, tgt = src.cuda(), tgt.cuda()
    tok = ByteTokenizer(min(cfg.src_vocab, cfg.tgt_vocab))
    arms = {}
    for name, model in (("1 model", models[0]), ("2 models", Ensemble(models))):
        tester = Tester(tok, model)
        arms[name + ", score_pairs"] = lambda model=model: score_pairs(model, src, tgt).sent_lp
        arms[name + ", score_pairs with top_lp"] = lambda model=model: score_pairs(model, src, tgt,
                                                                                     want_top=True).sent_lp
        arms[name + ", Tester.score"] = lambda tester=tester: tester.score(src, tgt)
    outs = {n: f().double().cpu() for n, f in arms.items()}  # warm-up: every shape of the timed window
    torch.cuda.synchronize()
    ms = {n: [] for n in arms}
    for _ in range(args.rounds):
        for n, f in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ms[n].append((time.perf_counter() - t0) * 1e3)
    lines.append(f"score_pairs, transformer-{args.preset} (random init), V {cfg.tgt_vocab}, {B} pairs of {S} + {T} "
                 f"tokens, whole call (forward included), {args.rounds} interleaved rounds (host clock around a "
                 "device synchronise; Tester.score ends in a copy to the host):")
    for n in arms:
        ref = outs[n.split(",")[0] + ", Tester.score"]
        lines.append(f"  {n}: median {statistics.median(ms[n]):.2f} ms/batch (min {min(ms[n]):.2f}, max "
                     f"{max(ms[n]):.2f}); largest |sentence log-prob - Tester.score| "
                     f"{(outs[n] - ref).abs().max().item():.2e} of about {ref.abs().mean().item():.0f}")
    report = "\n".join(lines)
    print(report, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
