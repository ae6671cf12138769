"""What R-Drop consistency training costs on one GPU.

(a) The loss kernel alone (xent_rdrop, csrc/kernels/rdrop.hip) at 8192 pairs x
    V = 7010 (row stride 7040): against the plain cross entropy (xent) on the
    same 16384 rows, against the torch composition it replaces (two float32
    log_softmax, the two KL sums, the label term and autograd through them, a
    cast) and against its byte floor, (2 read + 2 written) x rows x stride x
    2 B at the HBM rate. One launch per graph replay between device events;
    the logits are rewritten by every launch (they then hold gradients: values
    differ, the traffic does not), so the inputs are restored before the
    correctness comparison only.
(b) The training step (Transformer-base by default, bf16, one HIP graph) with
    rdrop_alpha 0 and 5 on the same batches, interleaved round by round in one
    process. With rdrop_alpha = 5 the step runs twice the rows.

  python scripts/rdrop_cost.py [--rounds 5] [--out FILE]

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
from tensorflow_distributed_on_gke_amd.ops.kernels.loss import xent_rdrop  # noqa: E402
from tensorflow_distributed_on_gke_amd.train.optim import Adam  # noqa: E402
from tensorflow_distributed_on_gke_amd.train.step import TrainStep  # noqa: E402

HBM_TBS = 5.5  # the rate the Adam kernel reaches on one MI355X (docs/KERNELS.md), TB/s
ALPHA, SMOOTHING = 5.0, 0.1


def torch_rdrop(x2, V, lab, ntok, workers):
    """The composition the kernel replaces; returns (row_loss [2 M], dlogits bf16)."""
    M = x2.shape[0] // 2
    z = x2[:, :V].float().requires_grad_(True)
    la, lb = torch.log_softmax(z[:M], -1), torch.log_softmax(z[M:], -1)
    valid = (lab[:M] != 0).float()
    hard = torch.nn.functional.one_hot(lab[:M], V).float() * (1.0 - SMOOTHING) + SMOOTHING / V
    kab = torch.nn.functional.kl_div(lb, la, reduction="none", log_target=True).sum(-1)  # KL(p || r)
    kba = torch.nn.functional.kl_div(la, lb, reduction="none", log_target=True).sum(-1)
    rows = torch.cat([(-(hard * la).sum(-1) + 0.5 * ALPHA * kab) * valid,
                      (-(hard * lb).sum(-1) + 0.5 * ALPHA * kba) * valid])
    (rows.sum() / (ntok.clamp_min(1.0)[0] * workers)).backward()
    out = torch.zeros_like(x2)
    out[:, :V] = z.grad.to(torch.bfloat16)
    return rows.detach(), out


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


def eager_us(fn, reps):
    """Median us of `fn` run eagerly (autograd does not capture into a graph here)."""
    fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        us.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(us)


def kernel_part(args, lines) -> None:
    M, V = args.pairs, args.vocab
    ld = (V + 63) // 64 * 64
    g = torch.Generator().manual_seed(args.seed)
    a = torch.randn(M, ld, generator=g) * 3.0
    x0 = torch.cat([a, a + torch.randn(M, ld, generator=g) * 0.3]).to(torch.bfloat16).cuda()
    lab = torch.randint(0, V, (M,), generator=g).repeat(2).cuda()
    ntok = torch.zeros(1, device="cuda")
    K.count_tokens(lab, ntok)
    rl, rc, rb = (torch.empty(2 * M, device="cuda") for _ in range(3))
    x = x0.clone()
    floor_us = 4 * M * ld * 2 / (HBM_TBS * 1e12) * 1e6
    lines.append(f"(a) loss kernel alone at {M} pairs x V = {V} (row stride {ld}, {2 * M} rows), copy 2 = copy 1 + "
                 f"N(0, 0.3^2), labels with PAD pairs, smoothing {SMOOTHING}, alpha {ALPHA}; one launch per graph "
                 f"replay, device events, {args.replays} replays:")
    xe = graph_us(lambda: K.xent(x, V, lab, ntok, 1.0, SMOOTHING, rl, rc), args.replays)
    kern = graph_us(lambda: xent_rdrop(x, V, lab, ntok, 1.0, SMOOTHING, ALPHA, rl, rc, rb), args.replays)
    comp = eager_us(lambda: torch_rdrop(x, V, lab, ntok, 1.0), max(3, args.replays // 4))
    x.copy_(x0)
    xent_rdrop(x, V, lab, ntok, 1.0, SMOOTHING, ALPHA, rl, rc, rb)
    ref_loss, ref_d = torch_rdrop(x0, V, lab, ntok, 1.0)
    dl = (rl - ref_loss).abs().max().item()
    dd = (x.float() - ref_d.float()).abs().max().item() / max(ref_d.float().abs().max().item(), 1e-30)
    lines.append(f"  xent on the same {2 * M} rows: median {xe[0]:.1f} us  (min {xe[1]:.1f}, max {xe[2]:.1f})")
    lines.append(f"  xent_rdrop: median {kern[0]:.1f} us  (min {kern[1]:.1f}, max {kern[2]:.1f}) = {kern[0] / xe[0]:.2f} x "
                 f"xent; floor (2 + 2) x pairs x stride x 2 B at {HBM_TBS} TB/s = {floor_us:.1f} us, measured / floor "
                 f"= {kern[0] / floor_us:.2f}")
    lines.append(f"  torch composition (eager, host clock around a synchronise): median {comp:.1f} us = "
                 f"{comp / kern[0]:.1f} x the kernel; largest |row_loss - composition| {dl:.2e}, largest |dlogits - "
                 f"composition| / max |dlogits| {dd:.2e}")


def step_part(args, lines) -> None:
    cfg = model_config(args.preset)
    data = SyntheticPairs(batch=args.batch, src_len=args.seq, tgt_len=args.seq + 1, src_vocab=cfg.src_vocab,
                          tgt_vocab=cfg.tgt_vocab, min_len=args.seq // 2, seed=args.seed)
    batches = [tuple(t.cuda() for t in data.batch(i)) for i in range(4)]
    arms = {}
    for alpha in (0.0, ALPHA):
        m = Transformer(cfg).build("cuda", seed=args.seed)
        step = TrainStep(m, Adam(m.store, cfg.d_model), None, workers=1.0, rdrop_alpha=alpha)
        assert step.capture(*batches[0])
        arms[alpha] = step
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
                 "around a device synchronise); rdrop_alpha > 0 runs 2 x the rows:")
    for n in arms:
        lines.append(f"  rdrop_alpha {n:g}: median {med[n]:.3f} ms/step  (min {min(ms[n]):.3f}, max {max(ms[n]):.3f}; "
                     f"{med[n] / med[0.0]:.2f} x the plain step, + {med[n] - med[0.0]:.3f} ms)")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="base")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seq", type=int, default=128)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=8192)
    ap.add_argument("--vocab", type=int, default=7010)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--skip-step", action="store_true", help="only the kernel-alone part")
    ap.add_argument("--out", default=None, help="also write the report here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("rdrop_cost.py needs a GPU")
    lines = [f"rdrop_cost: {torch.cuda.get_device_name(0)}"]
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
