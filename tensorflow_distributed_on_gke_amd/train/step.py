"""One synchronous data-parallel training step, optionally captured into a HIP
graph.

step = dropout-stream advance -> teacher-forced forward -> fused CE/accuracy ->
backward (gradients into the flat buffer, bucketed RCCL all-reduce started
from inside backward) -> wait for the buckets -> [gradient-norm pass, with
Adam's global_clipnorm / skip_nonfinite] -> multi-tensor Adam.

Gradient accumulation (accum_steps = N > 1, TrainStep.update): an update takes
N micro-batches, each treated as one more replica -- loss divided by
world * N (or, global token mean, by the label count of all of them) -- the
first overwriting the flat gradient buffer, the rest adding to it (the
kernels' beta = 1 paths); everything after backward (all-reduce spans, norm
pass, Adam, EMA) runs once, in the last micro-batch.

Reference: distributed_training_transformer/__main__.py:105-132 (train_step
inside strategy.run, apply_gradients all-reduce, strategy.reduce(SUM) of the
per-replica losses). The per-step loss stays on device; it is summed over
replicas only when the host reads it (log points).
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.distributed as dist

from tensorflow_distributed_on_gke_amd.config import check_accum_steps
from tensorflow_distributed_on_gke_amd.models.layers import RunCtx, WgradQueue
from tensorflow_distributed_on_gke_amd.models.transformer import Transformer
from tensorflow_distributed_on_gke_amd.parallel.ddp import DataParallel
from tensorflow_distributed_on_gke_amd.ops import kernels as K
from tensorflow_distributed_on_gke_amd.train.graphs import SegmentedGraph, prepare_capture
from tensorflow_distributed_on_gke_amd.train.optim import Adam
from tensorflow_distributed_on_gke_amd.train.step_cache import Captured, StepCache


# data parallel: weight gradients flushed in wave-sized chunks at layer ends
CHUNKED_WGRAD = True
# tiles per wave of the chunked schedule (0: one whole-K 256x256 tile per CU);
# tests set small values to force problems to be cut across launches
WAVE_TILES = 0
# skip the optimizer's gradient zeroing (all GPU gradient writers overwrite;
# with gradient accumulation the first micro-batch of every update does)
ZERO_GRAD_FREE = True
# how a data-parallel step is captured (TrainStep.capture):
#   "seg"  -- chain of HIP graphs cut at the collectives, which stay eager
#             RCCL calls between the segments (train/graphs.py; default)
#   "0"    -- no capture: the data-parallel step runs eagerly
# (round 1 also had "full", the collectives captured inside one graph; it
# failed capture under PyTorch 2.10's process-group watchdog and was removed)
DP_GRAPH = os.environ.get("TDG_DP_GRAPH", "seg")
# data parallel: time the segmented graph against the eager step once and keep
# the faster (TrainStep.choose_dp_mode); False keeps the segmented graph
DP_AUTOSELECT = True
# data parallel: each bucket's Adam runs as soon as its all-reduce is done.
# "tail": at the end of the step, so the last bucket's all-reduce overlaps the
# Adam of the others. "1": also mid-backward (decoder side during the
# encoder's backward) -- on one MI355X with --force-dp that concurrent Adam
# contended with the encoder backward for more than it hid (6.45 vs 6.34 ms).
# "0": one Adam after finish.
DP_OVERLAP_OPT = "tail"
# fp8 (one optimizer pass over the whole buffer): the Adam kernel also
# refreshes the e4m3 weight copies (no separate re-quantisation pass)
FUSED_FP8_ADAM = True


def micro_positions(n: int) -> List[str]:
    """Where each of an update's n micro-batches stands: "only", or "first",
    "middle"..., "last". The position decides what a micro-batch launches (the
    first overwrites the gradients, the last reduces and optimizes), so it is
    part of a captured micro-batch's cache key."""
    return ["only"] if n == 1 else ["first"] + ["middle"] * (n - 2) + ["last"]


class TrainStep:
    def __init__(self, model: Transformer, opt: Adam, ddp: Optional[DataParallel], workers: float,
                 seed: int = 0, dropout: Optional[float] = None, fp8_state=None,
                 defer_wgrad: Optional[bool] = None, loss_mode: str = "replica_mean",
                 accum_steps: int = 1, teacher=None, distill_alpha: float = 0.0):
        """teacher, distill_alpha: word-level distillation (train/distill.py).
        With a Teacher and distill_alpha in (0, 1] every micro-batch runs the
        teacher's forward before the student's -- inside the captured step,
        whichever way it is captured -- and trains on the mixed target; `accum`
        and `last` then hold that objective and `label_accum` the label
        cross entropy alone."""
        self.accum_steps = check_accum_steps(accum_steps, "fp8" if fp8_state is not None else "bf16")
        if not 0.0 <= float(distill_alpha) <= 1.0:
            raise ValueError(f"distill_alpha must lie in [0, 1], got {distill_alpha!r}")
        self.teacher = teacher if teacher is not None and distill_alpha > 0.0 else None
        self.distill_alpha = float(distill_alpha) if self.teacher is not None else 0.0
        if self.teacher is not None:
            if fp8_state is not None:
                raise ValueError("distillation with dtype=fp8 is not supported (use dtype=bf16)")
            self.teacher.check_student(model)
        self.model = model
        self.opt = opt
        self.ddp = ddp
        if ddp is not None:
            ddp.ema = opt.ema  # (verify_replicas also compares the averaged weights)
        # every micro-batch counts as one more replica
        self.workers = float(workers) * self.accum_steps
        # global token mean: every replica's loss is normalised by the label
        # count of the whole global batch (one scalar all-reduce per step,
        # overlapped with the forward) and the gradients are SUM-reduced
        if loss_mode not in ("replica_mean", "global_mean"):
            raise ValueError(f"loss_mode must be replica_mean or global_mean, got {loss_mode!r}")
        multi = ddp is not None and ddp.world > 1
        self.global_mean = loss_mode == "global_mean" and (multi or self.accum_steps > 1)
        self._ntok_sum = None
        # accumulation under the global token mean: the label count of the
        # whole update (all ranks, all micro-batches), set by _begin_update()
        # before the first micro-batch and read by every cross entropy
        self._ntok_total: Optional[torch.Tensor] = None
        dev = model.device
        if self.global_mean:
            self.workers = 1.0
            if self.accum_steps == 1:
                self._ntok_sum = ddp.all_reduce_async
            elif dev.type == "cuda":
                self._ntok_total = K.label_total(dev)[0]
            else:
                self._ntok_total = torch.zeros(1, dtype=torch.float32)
        self._ntok_reduce = ddp.all_reduce_async if multi else None
        # the micro-batch now running is its update's last (or only) one
        self.last_micro = True
        self.rt = RunCtx(training=True, dropout=model.cfg.dropout if dropout is None else dropout,
                         seed=seed, ctr=torch.zeros(1, dtype=torch.int64, device=dev),
                         store=model.store, fp8=fp8_state)
        # weight gradients grouped per shape (layers.WgradQueue): at the end of
        # backward on one GPU; with data parallelism also at the decoder /
        # encoder boundary so the decoder-side buckets' all-reduce overlaps
        # the encoder backward
        if defer_wgrad is None:
            defer_wgrad = True
        if defer_wgrad and dev.type == "cuda":
            dp = ddp is not None and ddp.active
            self.rt.wgrad = WgradQueue(flush_at_boundary=dp,
                                       wave_tiles=(WAVE_TILES or K.NUM_CU) if dp and CHUNKED_WGRAD else 0)
            # every encoder and decoder layer's backward ends with a layer_end()
            self.rt.wgrad.layers_per_step = 2 * model.cfg.layers
            # fp8: the bf16 weight gradients left (the vocab projection) are
            # too few tiles for the ragged 256x256 launch
            self.rt.wgrad.small_per_shape = fp8_state is not None and not self.rt.wgrad._chunking()
        self.fp8 = fp8_state
        if dev.type == "cuda" and not self.rt.accumulate and ZERO_GRAD_FREE:
            # every GPU gradient writer overwrites (the first micro-batch of an
            # update; the others run with rt.accumulate set)
            opt.zero_grad = False
        mode = DP_OVERLAP_OPT
        # (fp8: the scale update and the e4m3 weight re-quantisation run after
        # ddp.finish(), when every bucket's Adam is done, so the per-bucket
        # Adam stays on; the mid-backward variant would update weights the
        # fp8 copies of which the encoder backward still reads)
        if ddp is not None and ddp.active and mode != "0" and not (fp8_state is not None and mode != "tail"):
            # (clipping / skipping: no span's Adam before the norm of the whole
            # reduced gradient is known, so mid-backward "1" behaves as "tail")
            ddp.attach_optimizer(opt, release=mode != "tail" and not opt.clip_on)
        # metric accumulators [sum loss, sum acc, n steps, n tokens] (device)
        self.accum = torch.zeros(4, dtype=torch.float32, device=dev)
        self.last = torch.zeros(2, dtype=torch.float32, device=dev)
        # distillation: the label cross entropy alone, same four slots as accum
        self.label_accum = (torch.zeros(4, dtype=torch.float32, device=dev)
                            if self.teacher is not None else None)
        # Variable-length batches (text data, the reference's padded-to-the-
        # batch-max shapes: english_portugese_dataset.py:44-46, __main__.py:127
        # experimental_relax_shapes): with `bucketed` set, a batch of a shape
        # not captured yet is captured on the spot (warm-up, restore, capture:
        # it still trains once) and kept in an LRU cache of at most
        # `graph_cache` captured steps keyed by (source, target) shape. All of
        # them allocate from ONE memory pool: each replay is a whole step, so
        # the intermediates of different shapes may share memory (workspaces,
        # which persist, are never reused: ops.kernels.workspace).
        self.cache = StepCache(capacity=64, bucketed=False)
        self._pool = None
        self._cap_stream: Optional[torch.cuda.Stream] = None
        self._warm_stream: Optional[torch.cuda.Stream] = None

    # the captured steps (train/step_cache.py) under the names callers read
    graph = property(lambda self: self.cache.entry.graph)
    segments = property(lambda self: self.cache.entry.segments)
    captured = property(lambda self: bool(self.cache.entries))
    cached_shapes = property(lambda self: len(self.cache.entries))
    _graphs = property(lambda self: self.cache.entries)  # (read-only: the name before the cache)
    graph_stats = property(lambda self: self.cache.stats)
    bucketed = property(lambda self: self.cache.bucketed,
                        lambda self, v: setattr(self.cache, "bucketed", v))
    graph_cache = property(lambda self: self.cache.capacity,
                           lambda self, v: setattr(self.cache, "capacity", v))

    def capture_mode(self) -> str:
        """"single" (one graph, no collectives), "seg" or "0" (the
        data-parallel step stays eager)."""
        if self.ddp is None or not self.ddp.active:
            return "single"
        if DP_GRAPH not in ("seg", "0"):
            raise ValueError(f"TDG_DP_GRAPH must be seg or 0, got {DP_GRAPH!r}")
        if self.ddp._upd_stream is not None:
            # mid-backward Adam on its own stream would leave unjoined work
            # at a cut
            return "0"
        return DP_GRAPH

    # ------------------------------------------------------------------ state
    def _state(self):
        """Every tensor a training step mutates that outlives the step."""
        ts = [self.model.store.flat, self.opt.m, self.opt.v, self.opt.step, self.rt.ctr,
              self.accum, self.last]
        if self.fp8 is not None:
            ts += [self.fp8.meta.scale, self.fp8.gmeta.scale]
        if self.opt.clip_on:
            ts += [self.opt.norm_state, self.opt.norm_counters]
        if self.opt.ema is not None:
            ts += [self.opt.ema.avg, self.opt.ema.count]
        if self.label_accum is not None:
            ts += [self.label_accum]  # (the teacher's weights never change: not state)
        if self.accum_steps > 1:
            # a capture between two micro-batches warms up on the partial sums
            ts += [self.model.store.flat_grad]
            if self._ntok_total is not None:
                ts += [self._ntok_total]
        return ts

    def snapshot(self):
        st = [t.clone() for t in self._state()]
        if self.fp8 is not None:
            st += [self.fp8.meta.amax.clone(), self.fp8.gmeta.amax.clone()]
        return st  # (restore() reads the two amax tables from the end)

    def restore(self, st) -> None:
        """Put back a snapshot(): weights (and their derived bf16 / transposed /
        fp8 copies), Adam moments and step, dropout counter, metric
        accumulators, fp8 scales."""
        for t, v in zip(self._state(), st):
            t.copy_(v)
        self.model.store.refresh_compute()
        if self.fp8 is not None:
            self.fp8.weights.refresh()  # e4m3 copies with the restored scales
            self.fp8.meta.amax.copy_(st[-2])
            self.fp8.gmeta.amax.copy_(st[-1])

    def eager(self, src: torch.Tensor, tgt: torch.Tensor, pos: str = "only") -> torch.Tensor:
        """One micro-batch, uncaptured: forward and backward, the gradients
        overwriting the flat buffer ("only" / "first") or adding to it; the
        update's last one ("only" / "last") also reduces and optimizes.
        With accum_steps > 1 under the global token mean, _begin_update() must
        have set the update's label count."""
        first, last = pos in ("only", "first"), pos in ("only", "last")
        self.rt.accumulate = not first
        self.last_micro = last
        if self.ddp is not None:
            self.ddp.hold = not last
        try:
            self.model.loss_and_backward(src, tgt, self.rt, self.workers, accum=self.accum,
                                         step_out=self.last, bump_ctr=True, ntok_sum=self._ntok_sum,
                                         ntok_total=self._ntok_total, teacher=self.teacher,
                                         alpha=self.distill_alpha, label_accum=self.label_accum)
        finally:
            self.rt.accumulate = False
            self.last_micro = True
            if self.ddp is not None:
                self.ddp.hold = False
        if last:
            if self.ddp is not None:
                self.ddp.finish()
            self.optimize()
        return self.last

    def _begin_update(self, micro_batches) -> None:
        """Accumulation under the global token mean: the label count of all
        the update's micro-batches (GPU: one launch, ops.kernels
        count_labels_multi) summed over the ranks -- one scalar all-reduce per
        update -- into the scalar every cross entropy of the update reads."""
        tot = self._ntok_total
        if tot is None:
            return
        tgts = [t for _, t in micro_batches]
        if tot.is_cuda:
            K.count_labels_multi(tgts, tot, K.label_total(tot.device)[1])
        else:
            tot.fill_(float(sum(int((t[:, 1:] != 0).sum()) for t in tgts)))
        if self._ntok_reduce is not None:
            self._ntok_reduce(tot).wait()

    def update(self, micro_batches: Sequence[Tuple[torch.Tensor, torch.Tensor]]) -> torch.Tensor:
        """One optimizer update from accum_steps micro-batches (src, tgt),
        which may differ in shape. Defined as the update of world *
        accum_steps replicas with one batch each. Returns the device tensor
        [loss share, accuracy] of the LAST micro-batch; the update's loss is
        the sum of the shares, which `accum` collects ([sum of loss shares,
        sum of accuracies, micro-batches, labels])."""
        if len(micro_batches) != self.accum_steps:
            raise ValueError(f"update() takes accum_steps={self.accum_steps} micro-batches, "
                             f"got {len(micro_batches)}")
        if self.accum_steps == 1:
            return self(*micro_batches[0])
        if self.opt.ema is not None:  # (a replayed graph runs no Python: checked here)
            self.opt.ema.check_not_swapped("training step")
        self._begin_update(micro_batches)
        for (src, tgt), pos in zip(micro_batches, micro_positions(self.accum_steps)):
            if self.captured:
                self._replay(src, tgt, pos)
            else:
                self.eager(src, tgt, pos)
        return self.last

    def optimize(self) -> None:
        """The step after backward and ddp.finish(): the optimizer (unless
        finish() already ran it per span) and the fp8 bookkeeping."""
        if self.ddp is None or self.ddp.opt is None:
            if self.fp8 is not None and FUSED_FP8_ADAM and \
                    self.fp8.weights.adam_chunks(self.model.store) is not None:
                # new scales, then [the norm pass and] Adam refreshing the
                # e4m3 weight copies -- which a skipped step leaves alone, so
                # the weight slots then keep the scales of those copies
                held = self.fp8.hold_weight_scales() if self.opt.skip_nonfinite else None
                self.fp8.before_fused_opt()
                self.opt.apply(fp8w=self.fp8.weights)
                if held is not None:
                    self.fp8.keep_weight_scales_if(held, self.opt.norm_state[K.NORM_SKIP:K.NORM_SKIP + 1])
                return
            self.opt.apply()  # [the norm pass and] Adam
        if self.fp8 is not None:
            self.fp8.after_step()  # new scales, then fp8 weight copies

    # ------------------------------------------------------------------ HIP graph
    def capture(self, src: torch.Tensor, tgt: torch.Tensor, warmup: int = 2) -> bool:
        """Capture the whole step (fwd+bwd+optimizer) on static input buffers:
        one HIP graph on a single GPU; under data parallelism a segmented
        graph whose collectives are eager calls between the segments. With
        accum_steps > 1 that is one captured micro-batch per position an
        update of this shape needs (first, middle, last: micro_positions).

        Warm-up steps run first (lazily-allocated workspaces, GEMM tunings,
        communication buffers); the training state is snapshotted before and
        restored after them, so capture() itself trains nothing: after it the
        model, optimizer and counters are exactly as they were. Returns False
        (and leaves the step eager) when the data-parallel step is configured
        not to be captured."""
        if self.capture_mode() == "0":
            return False
        if self._ntok_total is not None:
            saved = self._ntok_total.clone()
            self._begin_update([(src, tgt)] * self.accum_steps)  # what the warm-ups divide by
        for pos in dict.fromkeys(micro_positions(self.accum_steps)):
            self._capture_micro(src, tgt, pos, warmup)
        if self._ntok_total is not None:
            self._ntok_total.copy_(saved)
        return True

    def _capture_micro(self, src: torch.Tensor, tgt: torch.Tensor, pos: str, warmup: int) -> None:
        """Capture one micro-batch at position `pos` (capture_mode() is not
        "0") and make it the current cache entry."""
        mode = self.capture_mode()
        if self._pool is None:
            self._pool = torch.cuda.graph_pool_handle()
        self.cache.clear_current()  # (no current entry until this one is put)
        static = (src.clone(), tgt.clone())
        saved = self.snapshot()
        if self._cap_stream is None:
            # one warm-up and one capture stream for every captured shape: the
            # workspaces (keyed by stream) are shared by all of them
            self._warm_stream = torch.cuda.Stream()
            self._cap_stream = torch.cuda.Stream()
        s = self._warm_stream
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(warmup):
                self.eager(*static, pos)
        torch.cuda.current_stream().wait_stream(s)
        self.restore(saved)
        del saved
        if mode != "single":
            # no collective of the warm-up may still be pending in the process
            # group's watchdog when the capture starts
            torch.cuda.synchronize()
            self.ddp.check_quiescent("capture")
            dist.barrier(group=self.ddp.group)
            torch.cuda.synchronize()
        g = rec = None
        if mode == "seg":
            prepare_capture()
            cap = self._cap_stream
            cap.wait_stream(torch.cuda.current_stream())
            rec = SegmentedGraph(cap, pool=self._pool)
            self.ddp.recorder = rec
            try:
                with torch.cuda.stream(cap):
                    rec.begin()
                    self.eager(*static, pos)
                    rec.end()
            except BaseException:
                rec.abort()
                raise
            finally:
                self.ddp.recorder = None
            torch.cuda.current_stream().wait_stream(cap)
        else:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=self._pool, stream=self._cap_stream):
                self.eager(*static, pos)
        self.cache.put(self._cache_key(src.shape, tgt.shape, pos), Captured(g, rec, static))

    # ------------------------------------------------------------------ shape cache
    def _cache_key(self, src_shape, tgt_shape, pos: str) -> tuple:
        """What a captured micro-batch bakes in: the batch shape, its position
        in the update, the loss divisor (world * accum_steps, or 1 with the
        global token mean) and where the label count comes from."""
        return (tuple(src_shape), tuple(tgt_shape), pos, self.workers, self.global_mean)

    def _select(self, key: tuple, src: torch.Tensor, tgt: torch.Tensor) -> None:
        """Make the captured micro-batch of this batch shape and position
        current: a cache hit, or (bucketed) a capture on the spot, evicting
        the least recently used one when the cache is full. Every rank sees
        the same global-batch shapes in the same order, so every rank
        captures and evicts alike."""
        cache = self.cache
        if cache.get(key) is not None:
            return
        if not cache.bucketed:
            raise ValueError(f"captured step takes {' or '.join(f'{a} / {b}' for a, b in cache.shapes())} "
                             f"batches, got {tuple(src.shape)} / {tuple(tgt.shape)}")
        cache.make_room()
        if self.capture_mode() == "0":
            raise RuntimeError("bucketed step: capture of a new batch shape failed")
        self._capture_micro(src, tgt, key[2], warmup=1)

    def _replay(self, src: torch.Tensor, tgt: torch.Tensor, pos: str) -> None:
        key = self._cache_key(src.shape, tgt.shape, pos)
        if key != self.cache.current:
            self._select(key, src, tgt)
        graph, segments, static = self.cache.entry
        self.cache.stats["replays"] += 1
        static[0].copy_(src, non_blocking=True)
        static[1].copy_(tgt, non_blocking=True)
        if segments is not None:
            segments.replay()
        else:
            graph.replay()

    def choose_dp_mode(self, src: torch.Tensor, tgt: torch.Tensor, steps: int = 8,
                       rounds: int = 3, margin: float = 0.03) -> Dict[str, object]:
        """Data parallel: pick how the step runs on THIS node, by measurement
        (train/dp_select.py has the arms, the rule and the returned record)."""
        from tensorflow_distributed_on_gke_amd.train.dp_select import choose_dp_mode
        return choose_dp_mode(self, src, tgt, steps, rounds, margin)

    def __call__(self, src: torch.Tensor, tgt: torch.Tensor) -> torch.Tensor:
        if self.accum_steps != 1:
            raise ValueError(f"a TrainStep with accum_steps={self.accum_steps} takes whole updates: "
                             "update(micro_batches)")
        if self.opt.ema is not None:  # (a replayed graph runs no Python: checked here)
            self.opt.ema.check_not_swapped("training step")
        if not self.captured:
            return self.eager(src, tgt)
        self._replay(src, tgt, "only")
        return self.last

    step = __call__
