"""The timed tile search and the tuned-table files shared by the bf16
(`ops/kernels/gemm.py`) and fp8 (`ops/fp8.py`) GEMM wrappers."""
from __future__ import annotations

import json
import os
from typing import Callable, Dict, Iterable, Sequence, Tuple

import torch

# Timed tile search for shapes missing from the tuned table: a tool
# (TDG_GEMM_AUTOTUNE=1, scripts/tune_in_model.py), never on in training runs,
# where results must not depend on the timing noise of the box
AUTOTUNE = os.environ.get("TDG_GEMM_AUTOTUNE", "0") == "1"


def time_candidates(cands: Sequence, trial: Callable, reps: int):
    """Time trial(c) for each candidate once for this problem (a warm-up call,
    then `reps` calls between HIP events on the current stream; two
    interleaved rounds, min per candidate: robust to clock noise) and return
    the fastest, the first of equal minima. A candidate whose trial raises
    RuntimeError (an unsupported config) is dropped; when none is left, what
    trial(cands[0]) raises surfaces the binding's error for this problem."""
    times: Dict[object, float] = {}
    for rnd in range(2):
        for c in cands:
            if rnd and c not in times:
                continue
            try:
                trial(c)  # warm-up (also surfaces unsupported configs)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    trial(c)
                e1.record()
                e1.synchronize()
                t = e0.elapsed_time(e1)
            except RuntimeError:
                continue
            times[c] = min(t, times.get(c, float("inf")))
    if not times:
        trial(cands[0])
    return min(times, key=times.get)


def table_file(env: str, name: str) -> str:
    """Path of a tuned table: the environment variable `env`, else `name` in
    this directory (ops/)."""
    return os.environ.get(env) or os.path.join(os.path.dirname(os.path.abspath(__file__)), name)


def save_table(path: str, items: Iterable[Tuple[str, object]]) -> None:
    """Write (key string, value) pairs, in the order given, as a JSON object."""
    with open(path, "w") as f:
        json.dump(dict(items), f, indent=0)


def load_table(path: str, parse_key: Callable, parse_val: Callable) -> dict:
    """{parse_key(key string): parse_val(value)} of a table file; empty when
    the file does not exist."""
    if not os.path.exists(path):
        return {}
    with open(path) as f:
        data = json.load(f)
    return {parse_key(ks): parse_val(v) for ks, v in data.items()}
