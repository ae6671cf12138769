"""Data parallel: how a TrainStep runs on this node, chosen once at start-up by
timing its options (TrainStep.choose_dp_mode delegates here).

The switches (DP_AUTOSELECT, ddp.COMM_THREAD) are read from their modules when
the function runs: tests and child processes set them there.
"""
from __future__ import annotations

import time
from typing import Dict

import torch
import torch.distributed as dist

from tensorflow_distributed_on_gke_amd.parallel import ddp as _ddp_mod
from tensorflow_distributed_on_gke_amd.train import step as _step_mod


def choose_dp_mode(step, src: torch.Tensor, tgt: torch.Tensor, steps: int = 8,
                   rounds: int = 3, margin: float = 0.03) -> Dict[str, object]:
    """Data parallel: pick how the step runs on THIS node, by measurement.

    Arms: the segmented graph (collectives issued between graph segments)
    and the eager step; and, where a comm thread exists
    (ddp.COMM_THREAD "auto"), both once more with the collectives issued
    by the host comm thread instead of the process group's own stream
    handoff. With accum_steps > 1 every arm runs whole updates (the batch
    repeated as each micro-batch). Each arm is timed in interleaved rounds
    (median per arm, MAX over ranks, so every rank takes the same
    decision) and, after its timed steps, the replicas must be bitwise
    equal (DataParallel.verify_replicas raises otherwise: an issue path
    that breaks synchronous DP is an error, not a slower option). The
    segmented graph wins when the host is the bottleneck (eight ranks
    sharing a node's CPUs); the eager step when the host keeps ahead. The
    training state is restored afterwards, so this trains nothing.
    Without a measurement (the step is not captured, DP_AUTOSELECT off)
    an available comm thread is used. Returns {"mode": "seg" | "0",
    "comm_thread": bool, "reason": "measured" | "unmeasured",
    "<arm>_ms": .., "select_s": seconds this selection took}."""
    ddp, cache = step.ddp, step.cache
    t_start = time.perf_counter()
    auto_thread = (ddp is not None and ddp.active and ddp.can_thread
                   and _ddp_mod.COMM_THREAD == "auto")
    if auto_thread:
        ddp.use_thread(False)

    def unmeasured(mode: str) -> Dict[str, object]:
        # no start-up measurement: with a comm thread available ("auto")
        # the thread issues the collectives -- it won the one-rank RCCL A/B
        # on MI355X for the eager and the segmented step alike (5.11 vs
        # 5.34 ms, profiles/r4/ab_dp_comm_thread.txt)
        if auto_thread:
            ddp.use_thread(True)
        th = ddp is not None and ddp._thread is not None
        return {"mode": mode, "comm_thread": th, "reason": "unmeasured",
                "select_s": round(time.perf_counter() - t_start, 3)}

    if not step.capture(src, tgt):
        return unmeasured(step.capture_mode())
    if not (ddp is not None and ddp.active and step.segments is not None) or not _step_mod.DP_AUTOSELECT:
        return unmeasured("seg" if step.segments is not None else step.capture_mode())
    # an arm: name -> (the captured micro-batches of one update as cache
    # entries, or None for the eager step; whether the comm thread issues the
    # collectives). Timed in this order within a round.
    arms = {"seg": (dict(cache.entries), ddp._thread is not None)}
    if auto_thread:
        cache.install(None)
        ddp.use_thread(True)
        if step.capture(src, tgt):
            arms["seg_thread"] = (dict(cache.entries), True)
        ddp.use_thread(False)
    # eager arms: the process group's handoff, and (auto) the comm thread
    arms["eager"] = (None, False)
    if auto_thread:
        arms["eager_thread"] = (None, True)

    def install(name: str) -> None:
        entries, thread = arms[name]
        cache.install(entries)
        ddp.use_thread(thread)  # (a captured graph keeps its own path)

    saved = step.snapshot()
    micro = [(src, tgt)] * step.accum_steps

    def run():
        step.update(micro)

    def timed() -> float:
        for _ in range(2):
            run()
        torch.cuda.synchronize()
        ddp.check_quiescent("choose_dp_mode")
        dist.barrier(group=ddp.group)
        t0 = time.perf_counter()
        for _ in range(steps):
            run()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / steps
        ddp.verify_replicas()  # the arm kept synchronous DP exact
        return dt

    names = list(arms)
    runs = {k: [] for k in names}
    for _ in range(rounds):
        for k in names:
            install(k)
            runs[k].append(timed())
    # median per arm: one noisy round (box clock, host contention) does
    # not decide the mode for the whole run
    med = {k: sorted(v)[len(v) // 2] for k, v in runs.items()}
    t = torch.tensor([med[k] for k in names], dtype=torch.float64, device=step.model.device)
    ddp.check_quiescent("choose_dp_mode")
    dist.all_reduce(t, op=dist.ReduceOp.MAX, group=ddp.group)
    ms = {k: float(v) for k, v in zip(names, t.tolist())}
    step.restore(saved)
    best_seg = min((k for k in names if arms[k][0] is not None), key=lambda k: ms[k])
    best_eager = min((k for k in names if arms[k][0] is None), key=lambda k: ms[k])
    best = best_eager if ms[best_eager] < ms[best_seg] * (1.0 - margin) else best_seg
    install(best)
    mode, th = ("0" if arms[best][0] is None else "seg"), arms[best][1]
    arms.clear()  # the other captures' graphs are released
    torch.cuda.synchronize()
    out = {"mode": mode, "comm_thread": th, "reason": "measured"}
    out.update({f"{k}_ms": round(v * 1e3, 3) for k, v in ms.items()})
    out["select_s"] = round(time.perf_counter() - t_start, 3)
    return out
