"""Optimizer family (csrc/kernels/adam.hip, ema.hip): Adam, the gradient
norm and its clip state, the weight EMA."""
from __future__ import annotations

from tensorflow_distributed_on_gke_amd.ops._ext import C


def adam_chunks(p, g, m, v, shadow, chunks, step, beta1, beta2, eps, lr_const, d_model, warmup,
                grad_scale, weight_decay, sched, zero_grad, inc_step, scale8, amax8, norm_state=None):
    """Adam over a chunk table that also refreshes e4m3 weight copies
    (adam.hip adam_chunk_kernel; table: ops.fp8.Fp8Weights.adam_chunks).
    norm_state: see adam()."""
    C().adam_chunks(p, g, m, v, shadow, chunks, step, beta1, beta2, eps, lr_const, d_model, warmup,
                    grad_scale, weight_decay, sched, zero_grad, inc_step, scale8, amax8, norm_state)


def adam(p, g, m, v, shadow, step, beta1, beta2, eps, lr_const, d_model, warmup, grad_scale=1.0,
         weight_decay=0.0, sched=1, zero_grad=True, inc_step=True, norm_state=None):
    """norm_state (grad_norm_finalize's f32 device state, or None): the
    gradient is also multiplied by its clip factor, and when its skip flag is
    set nothing is written but the gradient zeroing, nor the step advanced."""
    C().adam(p, g, m, v, shadow, step, beta1, beta2, eps, lr_const, d_model, warmup, grad_scale,
             weight_decay, sched, zero_grad, inc_step, norm_state)


def adam_step_inc(step, norm_state=None):
    """step += 1 on device, unless norm_state's skip flag is set."""
    C().adam_step_inc(step, norm_state)


# words of the gradient-norm device state / counters (adam.hip GNS_* / GNC_*)
NORM_SUMSQ, NORM_NORM, NORM_FACTOR, NORM_SKIP = 0, 1, 2, 3
NORM_CLIPPED, NORM_SKIPPED, NORM_MAX = 0, 1, 2


def grad_sumsq(g, partials, base=0, chunks=None) -> int:
    """partials[base ..] = the f32 squared sum of each <= 4096-element chunk
    of g (adam.hip grad_sumsq_kernel): the chunks of an Adam chunk table
    (g is then the whole flat buffer), or the consecutive 4096-element pieces
    of g (numel % 4 == 0). Returns the number of partials written."""
    return C().grad_sumsq(g, chunks, partials, base)


def grad_norm_finalize(partials, nparts, state, counters, clip=0.0, skip_nonfinite=False,
                       grad_scale=1.0):
    """state[0:4] = (squared sum, norm, clip factor clip / max(norm, clip),
    skip flag) of the gradient whose chunk sums are partials[:nparts], scaled
    by grad_scale; counters (int32): steps clipped, steps skipped, bits of the
    largest finite norm (adam.hip grad_norm_finalize_kernel)."""
    C().grad_norm_finalize(partials, nparts, state, counters, clip, skip_nonfinite, grad_scale)


def ema_update(p, e, count, decay, warmup=False, inc_count=True, norm_state=None):
    """e += (p - e) * (1 - d_eff) over two f32 ranges of one size (ema.hip):
    d_eff = decay, or with warmup min(decay, (1 + count) / (10 + count));
    count (int64 [1], device) is the number of updates so far -- at 0 the
    update copies p into e -- and advances when inc_count is set (the last
    range of a step). norm_state: see adam(); a skipped step changes neither
    e nor count."""
    C().ema(p, e, count, decay, warmup, inc_count, norm_state)
