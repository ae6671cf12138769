"""What word-level distillation costs on one GPU.

(a) The loss kernel alone (xent_distill, csrc/kernels/distill.hip) at rows x
    V = 8192 x 7010 (row stride 7040) with 1, 2 and 4 teachers, against the
    plain cross entropy (xent) on the same rows, against the torch
    composition it replaces (a float32 log_softmax of the student, a softmax
    per teacher, the mixed target, loss and gradient, a cast) and against its
    byte floor, (2 + T) x rows x stride x 2 B at the HBM rate. One launch per
    graph replay between device events; the student buffer is rewritten by
    every launch (it then holds gradients: values differ, the traffic does
    not), so the inputs are restored before the correctness comparison only.
(b) The training step (Transformer-base by default, bf16, one HIP graph) with
    0, 1 and 2 teachers of the student's configuration, interleaved round by
    round in one process.

  python scripts/distill_cost.py [--rounds 5] [--out FILE]

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
from tensorflow_distributed_on_gke_amd.train.distill import Teacher  # noqa: E402
from tensorflow_distributed_on_gke_amd.train.optim import Adam  # noqa: E402
from tensorflow_distributed_on_gke_amd.train.step import TrainStep  # noqa: E402

HBM_TBS = 5.5  # the rate the Adam kernel reaches on one MI355X (docs/KERNELS.md), TB/s
TEACHERS = (1, 2, 4)


def torch_distill(x, teachers, V, lab, ntok, workers, s, alpha, w):
    """The composition the kernel replaces; returns (row_loss, dlogits bf16)."""
    logp = torch.log_softmax(x[:, :V].float(), dim=-1)
    q = sum(wm * torch.softmax(t[:, :V].float(), dim=-1) for t, wm in zip(teachers, w))
    hard = torch.nn.functional.one_hot(lab, V).float() * (1.0 - s) + s / V
    target = (1.0 - alpha) * hard + alpha * q
    valid = (lab != 0).float()
    loss = -(target * logp).sum(-1) * valid
    d = (torch.exp(logp) - target) * (valid / (ntok.clamp_min(1.0) * workers)).view(-1, 1)
    out = torch.zeros_like(x)
    out[:, :V] = d.to(torch.bfloat16)
    return loss, out


def graph_us(fn, replays):
    """Median, min, max us of `fn`, one call per graph replay."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
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
        us.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(us), min(us), max(us)


def kernel_part(args, lines) -> None:
    M, V = args.rows, args.vocab
    ld = (V + 63) // 64 * 64
    g = torch.Generator().manual_seed(args.seed)
    x0 = (torch.randn(M, ld, generator=g) * 3.0).to(torch.bfloat16).cuda()
    teachers = [(torch.randn(M, ld, generator=g) * 3.0).to(torch.bfloat16).cuda() for _ in range(max(TEACHERS))]
    lab = torch.randint(0, V, (M,), generator=g).cuda()
    ntok = torch.zeros(1, device="cuda")
    K.count_tokens(lab, ntok)
    rl, rc, rb = (torch.empty(M, device="cuda") for _ in range(3))
    x = x0.clone()
    lines.append(f"(a) loss kernel alone at rows x V = {M} x {V} (row stride {ld}), labels with PAD rows, "
                 f"smoothing 0.1, alpha 0.5; one launch per graph replay, device events, {args.replays} replays:")
    xe = graph_us(lambda: K.xent(x, V, lab, ntok, 1.0, 0.1, rl, rc), args.replays)
    lines.append(f"  xent (no teacher): median {xe[0]:.1f} us  (min {xe[1]:.1f}, max {xe[2]:.1f}); floor 2 x rows x "
                 f"stride x 2 B at {HBM_TBS} TB/s = {2 * M * ld * 2 / (HBM_TBS * 1e12) * 1e6:.1f} us")
    for T in TEACHERS:
        te, w = teachers[:T], [1.0 / T] * T
        kern = graph_us(lambda: K.xent_distill(x, te, V, lab, ntok, 1.0, 0.1, 0.5, None, rl, rc, rb), args.replays)
        comp = graph_us(lambda: torch_distill(x, te, V, lab, ntok, 1.0, 0.1, 0.5, w), max(3, args.replays // 4))
        x.copy_(x0)
        K.xent_distill(x, te, V, lab, ntok, 1.0, 0.1, 0.5, None, rl, rc, rb)
        ref_loss, ref_d = torch_distill(x0, te, V, lab, ntok, 1.0, 0.1, 0.5, w)
        dl = (rl - ref_loss).abs().max().item()
        dd = (x.float() - ref_d.float()).abs().max().item() / max(ref_d.float().abs().max().item(), 1e-30)
        floor_us = (2 + T) * M * ld * 2 / (HBM_TBS * 1e12) * 1e6
        lines.append(f"  {T} teacher{'s' if T > 1 else ' '}: xent_distill median {kern[0]:.1f} us  (min {kern[1]:.1f}, max "
                     f"{kern[2]:.1f}) = {kern[0] / xe[0]:.2f} x xent; torch composition median {comp[0]:.1f} us = "
                     f"{comp[0] / kern[0]:.1f} x the kernel; floor (2 + {T}) x rows x stride x 2 B = {floor_us:.1f} us, "
                     f"measured / floor = {kern[0] / floor_us:.2f}; largest |row_loss - composition| {dl:.2e}, "
                     f"largest |dlogits - composition| / max |dlogits| {dd:.2e}")


def step_part(args, lines) -> None:
    cfg = model_config(args.preset)
    data = SyntheticPairs(batch=args.batch, src_len=args.seq, tgt_len=args.seq + 1, src_vocab=cfg.src_vocab,
                          tgt_vocab=cfg.tgt_vocab, min_len=args.seq // 2, seed=args.seed)
    batches = [tuple(t.cuda() for t in data.batch(i)) for i in range(4)]
    pool = [Transformer(cfg).build("cuda", seed=args.seed + 100 + i) for i in range(2)]
    arms = {}
    for n in (0, 1, 2):
        m = Transformer(cfg).build("cuda", seed=args.seed)
        step = TrainStep(m, Adam(m.store, cfg.d_model), None, workers=1.0,
                         teacher=Teacher(pool[:n]) if n else None, distill_alpha=0.5 if n else 0.0)
        assert step.capture(*batches[0])
        arms[n] = step
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
                 f"bf16, one HIP graph, {args.steps} steps per timing, {args.rounds} interleaved rounds (host clock "
                 "around a device synchronise), teachers of the student's configuration:")
    for n in arms:
        lines.append(f"  {n} teacher{'s' if n != 1 else ' '}: median {med[n]:.3f} ms/step  (min {min(ms[n]):.3f}, max "
                     f"{max(ms[n]):.3f}; {med[n] / med[0]:.2f} x the plain step, + {med[n] - med[0]:.3f} ms)")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="base")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seq", type=int, default=128)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--vocab", type=int, default=7010)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--skip-step", action="store_true", help="only the kernel-alone part")
    ap.add_argument("--out", default=None, help="also write the report here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("distill_cost.py needs a GPU")
    lines = [f"distill_cost: {torch.cuda.get_device_name(0)}"]
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
