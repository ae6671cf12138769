"""What ensemble decoding costs on one GPU.

Builds random-init models (Transformer-base by default) and times beam search
(beam 4) over the same batch of random sentences with 1, 2 and 4 of them as
one ensemble, interleaved round by round in one process, a host clock around a
device synchronise; reported per decoding step and per generated token of a
sentence. Also times the combine kernel alone (ensemble_logprobs, a HIP graph
of repeated launches between device events) at (rows, V, members) =
(128, 7010, 4) against the torch composition it replaces (a float32
log_softmax per member, a stack, a logsumexp, a cast) and against its floor,
(members + 1) x rows x V x 2 B at the HBM rate.

  python scripts/ensemble_cost.py [--rounds 5] [--out FILE]

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

from tensorflow_distributed_on_gke_amd.infer.beam import beam_search  # noqa: E402
from tensorflow_distributed_on_gke_amd.infer.ensemble import Ensemble  # noqa: E402
from tensorflow_distributed_on_gke_amd.infer.tokenizer import END, START  # noqa: E402
from tensorflow_distributed_on_gke_amd.models.transformer import Transformer, model_config  # noqa: E402
from tensorflow_distributed_on_gke_amd.ops import kernels as K  # noqa: E402

HBM_TBS = 6.3  # achievable HBM3E rate of one MI355X (8.0 peak), TB/s
SIZES = (1, 2, 4)


def torch_combine(logits, V, logw):
    parts = [torch.log_softmax(x[:, :V].float(), dim=-1) + lw for x, lw in zip(logits, logw)]
    return torch.logsumexp(torch.stack(parts), dim=0).to(torch.bfloat16)


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
    ap.add_argument("--batch", type=int, default=32, help="sentences decoded together")
    ap.add_argument("--src-len", type=int, default=32)
    ap.add_argument("--max-length", type=int, default=32)
    ap.add_argument("--beam", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rows", type=int, default=128, help="rows of the kernel-alone timing")
    ap.add_argument("--vocab", type=int, default=7010, help="V of the kernel-alone timing")
    ap.add_argument("--members", type=int, default=4, help="members of the kernel-alone timing")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the report here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ensemble_cost.py needs a GPU")

    cfg = model_config(args.preset)
    models = [Transformer(cfg).build("cuda", seed=args.seed + i) for i in range(max(SIZES))]
    g = torch.Generator().manual_seed(args.seed)
    src = torch.randint(4, cfg.src_vocab, (args.batch, args.src_len), generator=g)
    arms = {n: (models[0] if n == 1 else Ensemble(models[:n])) for n in SIZES}

    def decode(n):
        return beam_search(arms[n], src, START, END, beam=args.beam, max_length=args.max_length)

    steps = {}
    for n in SIZES:  # warm-up: every shape of the timed window
        steps[n] = decode(n)[2].shape[2] - 1
    torch.cuda.synchronize()
    ms = {n: [] for n in SIZES}
    for _ in range(args.rounds):
        for n in SIZES:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = decode(n)
            torch.cuda.synchronize()
            assert out[2].shape[2] - 1 == steps[n]
            ms[n].append((time.perf_counter() - t0) * 1e3)

    R, V, M = args.rows, args.vocab, args.members
    ld = (V + 7) // 8 * 8
    logits = [(torch.randn(R, ld, generator=g) * 4.0).to(torch.bfloat16).cuda() for _ in range(M)]
    out = torch.empty(R, ld, dtype=torch.bfloat16, device="cuda")
    logw = [math.log(1.0 / M)] * M
    diff = (K.ensemble_logprobs(logits, V, out=out)[:, :V].float() - torch_combine(logits, V, logw).float()).abs()
    kern = graph_us(lambda: K.ensemble_logprobs(logits, V, out=out), 50, 10)
    comp = graph_us(lambda: torch_combine(logits, V, logw), 50, 10)
    floor_us = (M + 1) * R * V * 2 / (HBM_TBS * 1e12) * 1e6

    lines = [
        f"ensemble_cost: transformer-{args.preset} (random init), V {cfg.tgt_vocab}, {args.batch} sentences of "
        f"{args.src_len} tokens, beam {args.beam}, max_length {args.max_length}, {torch.cuda.get_device_name(0)}",
        f"beam search, whole call (encoder included), {args.rounds} interleaved rounds "
        "(host clock around a device synchronise):",
    ]
    med = {n: statistics.median(v) for n, v in ms.items()}
    for n in SIZES:
        lines.append(f"  {n} member{'s' if n > 1 else ' '}: median {med[n]:.2f} ms/call over {steps[n]} steps = "
                     f"{med[n] / steps[n]:.3f} ms/step = {med[n] / steps[n] / args.batch * 1e3:.1f} us per generated "
                     f"token of a sentence  (min {min(ms[n]):.2f}, max {max(ms[n]):.2f} ms/call;"
                     f" {med[n] / med[1]:.2f} x one model)")
    lines += [
        f"combine kernel alone at (rows, V, members) = ({R}, {V}, {M}), 50 launches per graph replay, device events, "
        "10 replays:",
        f"  ensemble_logprobs: median {kern[0]:.2f} us  (min {kern[1]:.2f}, max {kern[2]:.2f})",
        f"  torch composition ({M} f32 log_softmax, stack, logsumexp, cast): median {comp[0]:.2f} us  "
        f"(min {comp[1]:.2f}, max {comp[2]:.2f}); composition / kernel = {comp[0] / kern[0]:.1f}",
        f"  floor: ({M} + 1) x {R} x {V} x 2 B at {HBM_TBS} TB/s = {floor_us:.2f} us; measured / floor = "
        f"{kern[0] / floor_us:.1f}  (the operands, {(M + 1) * R * V * 2 / 1e6:.1f} MB, stay in cache between "
        "back-to-back launches)",
        f"  largest |kernel - composition| on these inputs: {diff.max().item():.3e} (both rounded to bf16)",
    ]
    report = "\n".join(lines)
    print(report, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
