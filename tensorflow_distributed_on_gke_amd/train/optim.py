"""Keras-semantics Adam over the flat master buffer.

GPU: one multi-tensor kernel (csrc/kernels/adam.hip) for the whole model,
reading the step counter and evaluating the Noam schedule on device, fused with
the bf16 shadow refresh and gradient zeroing. CPU: the same update in PyTorch.

Opt-in extensions (off by default; the reference sets neither): Keras'
`global_clipnorm` (tf.clip_by_global_norm: every gradient times
clip / max(norm, clip), norm = sqrt(sum g^2) over the whole flat gradient after
grad_scale) and `skip_nonfinite` (a step whose norm is inf or NaN changes
nothing but the gradient zeroing and does not advance `iterations`). The norm,
the factor and the skip flag live in device memory (grad_sumsq /
grad_norm_finalize in adam.hip) and the Adam kernels read them there, so the
step still needs no host sync.

`ema_decay` (off by default; Keras Adam's `use_ema` / `ema_momentum`) keeps an
exponential moving average of the weights (train/ema.py WeightEma, `opt.ema`),
updated once per completed step after the last Adam range.

Reference: distributed_training_transformer/__main__.py:72-73
(Adam(learning_rate=NoamSchedule(d_model), beta_1=0.9, beta_2=0.98, epsilon=1e-9)).
"""
from __future__ import annotations

import math
from typing import Optional

import torch

from tensorflow_distributed_on_gke_amd.models.params import ParamStore
from tensorflow_distributed_on_gke_amd.ops import kernels as K
from tensorflow_distributed_on_gke_amd.train.ema import WeightEma, check_decay
from tensorflow_distributed_on_gke_amd.train.schedule import noam_lr


# whole-buffer steps through the contiguous-chunk kernel (adam_chunk_kernel:
# one 4096-parameter chunk per workgroup) instead of the grid-strided one
ADAM_CHUNKED = True


class Adam:
    def __init__(self, store: ParamStore, d_model: int, warmup: float = 4000.0, beta1: float = 0.9,
                 beta2: float = 0.98, eps: float = 1e-9, lr: Optional[float] = None,
                 weight_decay: float = 0.0, global_clipnorm: float = 0.0,
                 skip_nonfinite: bool = False, ema_decay: float = 0.0, ema_warmup: bool = False):
        ema_decay = check_decay(ema_decay)
        if not (0.0 <= float(global_clipnorm) < math.inf):
            raise ValueError(f"global_clipnorm must be finite and >= 0 (0: off), got {global_clipnorm!r}")
        self.store = store
        self.d_model = d_model
        self.warmup = warmup
        self.beta1, self.beta2, self.eps = beta1, beta2, eps
        self.lr_const = lr  # None -> Noam schedule
        self.weight_decay = weight_decay
        dev = store.flat.device
        self.m = torch.zeros_like(store.flat)
        self.v = torch.zeros_like(store.flat)
        # Keras `iterations`: device-resident so the step is graph-capturable
        self.step = torch.zeros(1, dtype=torch.int64, device=dev)
        # zero the consumed gradient (so the next backward may accumulate).
        # TrainStep turns it off on the GPU, where every gradient writer of a
        # non-accumulating backward overwrites (beta = 0): 4 B/param of HBM
        # writes less in the bandwidth-bound optimizer.
        self.zero_grad = True
        self.global_clipnorm = float(global_clipnorm)
        self.skip_nonfinite = bool(skip_nonfinite)
        # the gradient-norm pass's device state, f32 (squared sum, norm, clip
        # factor, skip flag), and counters, int32 (steps clipped, steps
        # skipped, bits of the largest finite norm since reset_norm_max());
        # None with both settings off: the kernels then get a null pointer
        self.norm_state: Optional[torch.Tensor] = None
        self.norm_counters: Optional[torch.Tensor] = None
        self._nparts = 0  # chunk sums accumulated since the last finalize_norm()
        if self.clip_on:
            self.norm_state = torch.tensor([0.0, 0.0, 1.0, 0.0], dtype=torch.float32, device=dev)
            self.norm_counters = torch.zeros(4, dtype=torch.int32, device=dev)
            if dev.type == "cuda":
                # one f32 per <= 4096-element chunk; a range that does not
                # start on a chunk boundary adds at most one
                self._partials = torch.zeros(store.total // 4096 + 1 + 1024, dtype=torch.float32,
                                             device=dev)
            else:
                self._sumsq = torch.zeros((), dtype=torch.float64)
        # the averaged weights (None with ema_decay 0: no launch is added)
        self.ema: Optional[WeightEma] = WeightEma(store, ema_decay, ema_warmup) if ema_decay > 0.0 else None

    def update_ema(self) -> None:
        """The EMA update of a completed step (after its last Adam range)."""
        if self.ema is not None:
            self.ema.update(self.norm_state)

    @property
    def clip_on(self) -> bool:
        """Clipping or skipping is on: every step needs the gradient norm."""
        return self.global_clipnorm > 0.0 or self.skip_nonfinite

    # ------------------------------------------------------------------ gradient norm
    def accumulate_norm(self, start: int, end: int) -> None:
        """Add flat_grad[start:end]'s squared sum to the pending norm (one
        data-parallel span, once its all-reduce is done). Every element of
        the buffer must be covered exactly once before finalize_norm()."""
        s = self.store
        if not s.flat.is_cuda:
            self._sumsq += s.flat_grad[start:end].double().pow(2).sum()
            return
        tab = self._chunk_table(start, end)
        if tab is not None:
            n = K.grad_sumsq(s.flat_grad, self._partials, self._nparts, chunks=tab)
        else:
            n = K.grad_sumsq(s.flat_grad[start:end], self._partials, self._nparts)
        self._nparts += n

    def finalize_norm(self, grad_scale: float = 1.0) -> None:
        """Norm, clip factor, skip flag and counters from what
        accumulate_norm() collected (on device; no host read on the GPU)."""
        st, cn = self.norm_state, self.norm_counters
        if st.is_cuda:
            K.grad_norm_finalize(self._partials, self._nparts, st, cn, self.global_clipnorm,
                                 self.skip_nonfinite, grad_scale)
            self._nparts = 0
            return
        sumsq = self._sumsq * (float(grad_scale) ** 2)
        self._sumsq = torch.zeros((), dtype=torch.float64)
        norm = sumsq.sqrt().to(torch.float32)
        finite = bool(torch.isfinite(norm))
        skip = self.skip_nonfinite and not finite
        clip = torch.tensor(self.global_clipnorm, dtype=torch.float32)
        factor = torch.ones((), dtype=torch.float32)
        if self.global_clipnorm > 0.0 and not skip:
            # (a non-finite norm that is not skipped: NaN, as TF signals it)
            factor = clip / torch.maximum(norm, clip) if finite else norm * float("nan")
        st[K.NORM_SUMSQ], st[K.NORM_NORM] = sumsq.to(torch.float32), norm
        st[K.NORM_FACTOR], st[K.NORM_SKIP] = factor, float(skip)
        if finite and self.global_clipnorm > 0.0 and bool(norm > clip):
            cn[K.NORM_CLIPPED] += 1
        if skip:
            cn[K.NORM_SKIPPED] += 1
        if finite:
            cn[K.NORM_MAX] = torch.maximum(cn[K.NORM_MAX], norm.view(torch.int32))

    def compute_norm(self, grad_scale: float = 1.0) -> None:
        """The norm state of the whole gradient buffer."""
        self.accumulate_norm(0, self.store.total)
        self.finalize_norm(grad_scale)

    def last_grad_norm(self) -> float:
        """Global norm of the last step's gradient (host read)."""
        return float(self.norm_state[K.NORM_NORM].item()) if self.clip_on else float("nan")

    def clip_counters(self) -> dict:
        """Steps clipped and skipped so far and the largest finite norm since
        reset_norm_max() (host read; not checkpointed)."""
        if not self.clip_on:
            return {"clipped_steps": 0, "skipped_steps": 0, "grad_norm_max": 0.0}
        c = self.norm_counters.cpu()
        return {"clipped_steps": int(c[K.NORM_CLIPPED]), "skipped_steps": int(c[K.NORM_SKIPPED]),
                "grad_norm_max": float(c[K.NORM_MAX:K.NORM_MAX + 1].view(torch.float32)[0])}

    def reset_norm_max(self) -> None:
        """Start a new interval for clip_counters()['grad_norm_max']."""
        if self.clip_on:
            self.norm_counters[K.NORM_MAX] = 0

    def _skipped(self) -> bool:
        return self.clip_on and bool(self.norm_state[K.NORM_SKIP] != 0)

    def _chunk_table(self, start: int, end: int) -> Optional[torch.Tensor]:
        """The <= 4096-element chunk table of flat[start:end] for the chunked
        kernels (built once per range, outside captures), or None where the
        grid-stride kernel / a plain range is used."""
        s = self.store
        if not (s.flat.is_cuda and ADAM_CHUNKED and s.flat_compute is not None and s.total < (1 << 28)
                and start % 4 == 0 and end % 4 == 0 and end > start):
            return None
        tabs = self.__dict__.setdefault("_range_chunks", {})
        if (start, end) not in tabs:
            if torch.cuda.is_current_stream_capturing():
                return None  # (tables are built by the eager warm-up steps, not in a capture)
            rows = [(c0, min(4096, end - c0), -1, 0) for c0 in range(start, end, 4096)]
            from tensorflow_distributed_on_gke_amd.ops.fp8 import validate_chunk_table
            validate_chunk_table(rows, s.total, 1)
            tabs[(start, end)] = torch.tensor(rows, dtype=torch.int64, device=s.flat.device)
        return tabs[(start, end)]

    @property
    def iterations(self) -> int:
        return int(self.step.item())

    def lr_at(self, step: int) -> float:
        if self.lr_const is not None:
            return self.lr_const
        return noam_lr(step, self.d_model, self.warmup)

    def apply(self, grad_scale: float = 1.0, fp8w=None) -> bool:
        """The whole step. fp8w (ops.fp8.Fp8Weights): also refresh its e4m3
        weight copies from the updated weights in the same pass (GPU; returns
        False -- nothing done -- when its chunk table is unavailable). With
        clipping or skipping on, the norm pass over the whole buffer first."""
        s = self.store
        if self.ema is not None:
            self.ema.check_not_swapped("optimizer step")
        if fp8w is not None:
            chunks = fp8w.adam_chunks(s) if s.flat.is_cuda and s.flat_compute is not None else None
            if chunks is None:
                return False
            if self.clip_on:
                self.compute_norm(grad_scale)
            K.adam_chunks(s.flat, s.flat_grad, self.m, self.v, s.flat_compute, chunks, self.step,
                          self.beta1, self.beta2, self.eps, self.lr_const or 0.0, float(self.d_model),
                          float(self.warmup), 1.0 * grad_scale, self.weight_decay,
                          0 if self.lr_const is not None else 1, self.zero_grad, True,
                          fp8w.meta.scale, fp8w.meta.amax, norm_state=self.norm_state)
            s.refresh_transposed(0, s.total)
            self.update_ema()
            return True
        if self.clip_on:
            self.compute_norm(grad_scale)
        self.apply_range(0, self.store.total, grad_scale, inc_step=True)
        self.update_ema()
        return True

    def apply_range(self, start: int, end: int, grad_scale: float = 1.0, inc_step: bool = True) -> None:
        """Update flat[start:end] only (one data-parallel bucket, as soon as its
        all-reduce is done). Every range of a step reads the same step
        counter; exactly one call per step (the last) passes inc_step. With
        clipping or skipping on it applies the norm state as it stands: the
        caller has run accumulate_norm() over every range of the step and
        finalize_norm() first (apply() and DataParallel.finish() do)."""
        s = self.store
        if self.ema is not None:
            self.ema.check_not_swapped("optimizer step")
        sl = slice(start, end)
        ns = self.norm_state
        tab = self._chunk_table(start, end)
        if tab is not None:
            if getattr(self, "_no8", None) is None:
                self._no8 = (torch.ones(1, device=s.flat.device),
                             torch.zeros(2048, dtype=torch.int32, device=s.flat.device))
            K.adam_chunks(s.flat, s.flat_grad, self.m, self.v, s.flat_compute, tab,
                          self.step, self.beta1, self.beta2, self.eps, self.lr_const or 0.0,
                          float(self.d_model), float(self.warmup), grad_scale, self.weight_decay,
                          0 if self.lr_const is not None else 1, self.zero_grad, inc_step, *self._no8,
                          norm_state=ns)
            s.refresh_transposed(start, end)
            return
        if s.flat.is_cuda:
            K.adam(s.flat[sl], s.flat_grad[sl], self.m[sl], self.v[sl],
                   s.flat_compute[sl] if s.flat_compute is not None else None, self.step,
                   self.beta1, self.beta2, self.eps, self.lr_const or 0.0, float(self.d_model),
                   float(self.warmup), grad_scale, self.weight_decay,
                   0 if self.lr_const is not None else 1, self.zero_grad, inc_step, norm_state=ns)
            s.refresh_transposed(start, end)  # transposed compute copies of updated weights
            return
        if ns is not None:
            if self._skipped():  # nothing but the gradient zeroing; the step does not advance
                s.flat_grad[sl].zero_()
                return
            # (f32 product, as the kernels fold the factor into grad_scale)
            grad_scale = float(torch.tensor(grad_scale, dtype=torch.float32) * ns[K.NORM_FACTOR])
        step = int(self.step.item())
        lr = self.lr_at(step)
        t = step + 1
        lr_t = lr * math.sqrt(1 - self.beta2 ** t) / (1 - self.beta1 ** t)
        p, g, m, v = s.flat[sl], s.flat_grad[sl], self.m[sl], self.v[sl]
        g = g * grad_scale
        m.add_((g - m) * (1 - self.beta1))
        v.add_((g * g - v) * (1 - self.beta2))
        p.sub_(lr_t * m / (v.sqrt() + self.eps) + lr * self.weight_decay * p)
        s.flat_grad[sl].zero_()
        if inc_step:
            self.step += 1

    def advance_step(self) -> None:
        """Keras `iterations += 1` after a step applied as several ranges
        (not after a skipped one; decided on device on the GPU)."""
        if self.norm_state is None:
            self.step += 1
        elif self.step.is_cuda:
            K.adam_step_inc(self.step, self.norm_state)
        elif not self._skipped():
            self.step += 1

    def state_dict(self) -> dict:
        return {"m": self.m.detach().cpu(), "v": self.v.detach().cpu(),
                "iterations": torch.tensor(self.iterations)}

    def load_state_dict(self, sd: dict) -> None:
        self.m.copy_(sd["m"])
        self.v.copy_(sd["v"])
        self.step.fill_(int(sd["iterations"]))
