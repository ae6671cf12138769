"""The grow-only per-device, per-stream scratch workspace of the launch
wrappers, so a captured HIP graph sees stable addresses."""
from __future__ import annotations

from typing import Dict, List, Tuple

import torch

NUM_CU = 256

_WS: Dict[Tuple[int, int, str], torch.Tensor] = {}
_WS_RETIRED: List[torch.Tensor] = []


def workspace(name: str, numel: int, device, dtype=torch.float32, zero: bool = False) -> torch.Tensor:
    """Named scratch buffer, one per (device, stream): a buffer is only ever
    used by kernels of one stream, so growing it (which frees the old one to
    the caching allocator, in that stream's pool) cannot race a kernel of
    another stream."""
    dev = torch.device(device)
    sid = torch.cuda.current_stream(dev).stream_id if dev.type == "cuda" else 0
    key = (dev.index or 0, sid, name)
    t = _WS.get(key)
    if t is None or t.numel() < numel or t.dtype != dtype:
        if t is not None:
            # a captured HIP graph may still address the smaller buffer (the
            # step cache keeps one graph per batch shape, train/step.py):
            # never hand its memory to another tensor
            _WS_RETIRED.append(t)
        t = (torch.zeros if zero else torch.empty)(max(numel, 1), dtype=dtype, device=dev)
        _WS[key] = t
    return t


def reset_workspace() -> None:
    _WS.clear()
    _WS_RETIRED.clear()
