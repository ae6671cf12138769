"""Exponential moving average of the weights (Keras Adam `use_ema`), kept
next to the flat master buffer for evaluation and decoding.

After every completed optimizer step
    avg += (flat - avg) * (1 - d_eff)
with d_eff = decay, or with warm-up min(decay, (1 + count) / (10 + count))
(the ramp of tf.train.ExponentialMovingAverage's num_updates), where `count`
is the number of updates applied so far. The first update copies the weights.
A step the optimizer skipped (skip_nonfinite) is no update. GPU: one streaming
kernel (csrc/kernels/ema.hip) reading the count and the skip flag on device,
so the update needs no host sync and is captured with the step. CPU: the same
f32 arithmetic in PyTorch.

`swapped()` puts the average in the weights' place (and the weights in the
average's) for a validation or decoding pass, in place: captured graphs hold
the buffers' addresses.
"""
from __future__ import annotations

from contextlib import contextmanager
from typing import Optional

import torch

from tensorflow_distributed_on_gke_amd.models.params import ParamStore
from tensorflow_distributed_on_gke_amd.ops import kernels as K


def check_decay(decay: float) -> float:
    decay = float(decay)
    if not (0.0 <= decay < 1.0):
        raise ValueError(f"ema_decay must lie in [0, 1) (0: off), got {decay!r}")
    return decay


class WeightEma:
    def __init__(self, store: ParamStore, decay: float, warmup: bool = False):
        self.store = store
        self.decay = check_decay(decay)
        self.warmup = bool(warmup)
        # (contents are irrelevant until the first update, which copies)
        self.avg = torch.zeros_like(store.flat)
        # updates applied so far: device-resident, like Adam's `iterations`
        self.count = torch.zeros(1, dtype=torch.int64, device=store.flat.device)
        self.in_swap = False

    @property
    def updates(self) -> int:
        return int(self.count.item())

    def d_eff(self, count: int) -> torch.Tensor:
        """The decay of the update that follows `count` earlier ones (f32)."""
        d = torch.tensor(self.decay, dtype=torch.float32)
        if self.warmup:
            c = torch.tensor(float(count), dtype=torch.float32)
            d = torch.minimum(d, (1.0 + c) / (10.0 + c))
        return d

    def check_not_swapped(self, what: str) -> None:
        if self.in_swap:
            raise RuntimeError(f"{what} inside WeightEma.swapped(): the weights and their average "
                               "are exchanged")

    def update(self, norm_state: Optional[torch.Tensor] = None, start: int = 0,
               end: Optional[int] = None, inc_count: bool = True) -> None:
        """One update of avg[start:end] (the whole buffer by default). Every
        range of a step reads the same count; exactly one call per step (the
        last) passes inc_count. norm_state: the optimizer's gradient-norm
        state, whose skip flag makes this a no-op."""
        self.check_not_swapped("EMA update")
        s = self.store
        end = s.total if end is None else end
        sl = slice(start, end)
        if s.flat.is_cuda:
            K.ema_update(s.flat[sl], self.avg[sl], self.count, self.decay, self.warmup, inc_count,
                         norm_state=norm_state)
            return
        if norm_state is not None and bool(norm_state[K.NORM_SKIP] != 0):
            return
        cnt = self.updates
        p, e = s.flat[sl], self.avg[sl]
        if cnt == 0:
            e.copy_(p)
        else:
            e.add_((p - e) * (1.0 - self.d_eff(cnt)))
        if inc_count:
            self.count += 1

    @contextmanager
    def swapped(self):
        """Exchange the contents of store.flat and avg in place and re-derive
        the compute copies, so the model runs on the averaged weights; on exit
        exchange them back (bitwise). The fp8 state (scales, amax tables, e4m3
        copies) is not touched: run bf16 inside (RunCtx(fp8=None)). No EMA
        update and no optimizer step may run inside."""
        self.check_not_swapped("swapped()")
        if self.updates == 0:
            raise RuntimeError("WeightEma.swapped(): no update applied yet, the average holds no weights")
        self._exchange()
        self.in_swap = True
        try:
            yield self
        finally:
            self.in_swap = False
            self._exchange()

    def _exchange(self) -> None:
        s = self.store
        with torch.no_grad():
            tmp = s.flat.clone()
            s.flat.copy_(self.avg)
            self.avg.copy_(tmp)
        s.refresh_compute()

    def state_dict(self) -> dict:
        return {"avg": self.avg.detach().cpu(), "updates": torch.tensor(self.updates)}

    def load_state_dict(self, sd: dict) -> None:
        self.avg.copy_(sd["avg"])
        self.count.fill_(int(sd["updates"]))
