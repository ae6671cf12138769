"""The deferred weight-gradient queue (RunCtx.wgrad) and the helpers models/layers.py feeds it through."""
from __future__ import annotations

from collections import namedtuple
from typing import Optional

from tensorflow_distributed_on_gke_amd.models.params import Param
from tensorflow_distributed_on_gke_amd.ops import kernels as K
from tensorflow_distributed_on_gke_amd.ops import fp8


def _beta(rt) -> float:
    return 1.0 if rt.accumulate else 0.0


def _ready(rt, *params: Param) -> None:
    if rt.store is not None:
        for p in params:
            rt.store.grad_ready(p)


class Wgrad(namedtuple("Wgrad", "dy x N w b beta rt")):
    """w.grad[N, K] (=|+= beta) dy[M, N]^T @ x[M, K]; b.grad (b may be None): dy's column sums."""

    @property
    def tiles(self) -> int:
        return -(-self.N // 256) * -(-self.x.shape[1] // 256)

    @property
    def ragged_ok(self) -> bool:
        return self.x.shape[0] % 64 == 0 and self.dy.stride(0) % 8 == 0 and self.x.stride(0) % 8 == 0

    @property
    def params(self):
        return (self.w,) if self.b is None else (self.w, self.b)


# w.grad (=|+= beta) dequant(dy8^T @ x8): e5m2 gradient (scale sa) x e4m3
# activation (scale sb), token-major (ops.fp8.wgrad_fp8)
Wgrad8 = namedtuple("Wgrad8", "dy8 sa x8 sb w beta rt")
# deferred column folds, (partials, out, nparts, N, beta) each, and the
# parameters whose gradients are final once they ran
Fold = namedtuple("Fold", "entries params rt")


class WgradQueue:
    """Weight-gradient GEMMs deferred to the end of backward.

    Nothing in backward reads a weight gradient, so instead of one small
    long-K GEMM per layer (split-K slabs + a reduce kernel, 64x64 tiles to
    fill the chip) all of them run as ONE ragged launch of 256x256 whole-K
    tiles (ops.kernels.wgrad_ragged: 5 shapes, 62 problems, ~730 tiles for
    Transformer-base; bias gradients fused). A flush holding an operand the
    ragged kernel does not take (Wgrad.ragged_ok), and the small fp8 flush
    (small_per_shape), fall back to one grouped launch per shape
    (ops.kernels.wgrad_grouped) plus column sums.
    The data-parallel grad_ready notifications follow in backward order."""

    def __init__(self, flush_at_boundary: bool = False, wave_tiles: int = 0):
        self.items = []
        # data parallel: also flush when the decoder's backward is complete,
        # so the decoder-side buckets are all-reduced while the encoder's
        # backward runs (only without wave chunking)
        self.flush_at_boundary = flush_at_boundary
        # data parallel, ragged path: at every layer end launch as many whole
        # waves of `wave_tiles` tiles (one 256x256 whole-K tile per CU) as are
        # queued -- a launch of the queue's first n*wave_tiles tiles, cutting
        # the boundary problem by tile range -- so the all-reduce of those
        # gradients starts layers earlier while the launches together cost
        # exactly the waves of a single launch (chunks that each fill only
        # part of a wave cost a whole wave each: 4 chunks measured 1004 us vs
        # 745 us for one launch on Transformer-base)
        self.wave_tiles = wave_tiles
        # layer_end() calls per backward (set by the owner: encoder + decoder
        # layers). With wave chunking the LAST layer end flushes everything
        # queued, partial wave included: otherwise the remainder waits for the
        # end of backward and its gradients join the embedding gradients in
        # the final, fully exposed all-reduce span (71 MB at Transformer-base;
        # with the full flush the final span holds little more than the
        # source embedding)
        self.layers_per_step = 0
        self._layer_ends = 0
        self._cursor = 0  # tiles of items[0] already launched
        # deferred LayerNorm dgamma/dbeta/bias partial folds (one launch per flush)
        self._folds = []
        self.fp8_items = []
        self.small_per_shape = False

    def boundary(self) -> None:
        if self.flush_at_boundary and not self._chunking() and (self.items or self._folds or self.fp8_items):
            self.flush()

    def _chunking(self) -> bool:
        return bool(self.wave_tiles)

    def layer_end(self) -> None:
        """A decoder or encoder layer's backward is complete."""
        self._layer_ends += 1
        last = self.layers_per_step > 0 and self._layer_ends >= self.layers_per_step
        if self._chunking() and self.fp8_items:
            self._flush_fp8()  # (its gradients join the next all-reduce span)
        if not self._chunking() or not self.items:
            return
        if last or not all(it.ragged_ok for it in self.items):
            self.flush()
            return
        queued = sum(it.tiles for it in self.items) - self._cursor
        n = queued // self.wave_tiles * self.wave_tiles
        if n:
            self._finish_flush(self._launch_prefix(n))

    def add(self, dy2, x2, N, w: Param, b: Optional[Param], beta: float, rt):
        self.items.append(Wgrad(dy2, x2, N, w, b, beta, rt))

    def add_fp8(self, dy8, sa, x8, sb, w: Param, beta: float, rt):
        """An fp8 weight gradient (ops.fp8.wgrad_fp8), launched with the
        next flush / layer end as one ragged fp8 launch."""
        self.fp8_items.append(Wgrad8(dy8, sa, x8, sb, w, beta, rt))

    def defer_fold(self, entries, params, rt) -> None:
        """Column folds, (partials, out, nparts, N, beta) each, to run with the
        next flush (ops.kernels.reduce_partials_multi, one launch for all);
        `params`: the parameters to report ready once they ran."""
        self._folds.append(Fold(tuple(entries), tuple(params), rt))

    def _flush_fp8(self) -> None:
        if not self.fp8_items:
            return
        by_beta = {}
        for it in self.fp8_items:
            by_beta.setdefault(it.beta, []).append(it)
        for beta, its in by_beta.items():
            # equal shapes adjacent (one class each)
            its.sort(key=lambda it: (it.w.shape, it.dy8.stride(0), it.x8.stride(0)))
            fp8.wgrad_fp8([it.dy8 for it in its], [it.sa for it in its], [it.x8 for it in its],
                          [it.sb for it in its], [it.w.grad for it in its], beta)
        for it in self.fp8_items:
            _ready(it.rt, it.w)
        self.fp8_items = []

    def step_done(self) -> None:
        """End of a backward: the layer-end count restarts."""
        self._layer_ends = 0

    def flush(self) -> None:
        self._flush_fp8()
        done = []
        if self.items:
            # (small_per_shape: a flush of under half a wave of 256x256 tiles
            # -- the fp8 step's lone bf16 vocab projection -- runs per shape
            # on 128x128 tiles)
            if all(it.ragged_ok for it in self.items) and (
                    not self.small_per_shape or self._cursor
                    or sum(it.tiles for it in self.items) >= K.NUM_CU // 2):
                done = self._launch_prefix(sum(it.tiles for it in self.items) - self._cursor)
            else:  # (never partially launched: chunking needs the ragged path)
                self._flush_grouped()
                self._flush_bias()
                done, self.items = self.items, []
        self._finish_flush(done)

    def _finish_flush(self, done) -> None:
        """Run the deferred folds; report the launched items' and their parameters ready."""
        folds, self._folds = self._folds, []
        if folds:
            K.reduce_partials_multi([e for f in folds for e in f.entries])
        final = done + folds
        for it in final:
            _ready(it.rt, *it.params)
        if final and final[0].rt.store is not None:
            final[0].rt.store.grad_sync()

    def _launch_prefix(self, n: int) -> list:
        """Launch the first n not-yet-launched tiles of the queue (whole-K
        256x256 tiles, bias gradients fused) and return the items they
        complete; a cut item stays at the queue head with self._cursor set."""
        sel = []  # (item, t_first, t_count)
        done = []
        left = n
        while left > 0 and self.items:
            it = self.items[0]
            avail = it.tiles - self._cursor
            take = min(avail, left)
            sel.append((it, self._cursor, take))
            left -= take
            if take == avail:
                done.append(self.items.pop(0))
                self._cursor = 0
            else:
                self._cursor += take
        # one launch per (token count, beta); within it full problems of equal
        # shape adjacent (one class each), cut problems as classes of their own
        runs = {}
        for it, first, cnt in sel:
            full = first == 0 and cnt == it.tiles
            key = (it.N, it.x.shape[1], it.dy.stride(0), it.x.stride(0)) if full else ("cut", id(it), first)
            runs.setdefault((it.x.shape[0], it.beta), {}).setdefault(key, []).append((it, first, cnt))
        for (_, beta), by_shape in runs.items():
            groups = list(by_shape.values())
            for s0 in range(0, len(groups), K.RAGGED_MAX_SHAPES):
                chunk = [e for grp in groups[s0:s0 + K.RAGGED_MAX_SHAPES] for e in grp]
                for c0 in range(0, len(chunk), K.RAGGED_MAX_PROBLEMS):
                    part = chunk[c0:c0 + K.RAGGED_MAX_PROBLEMS]
                    K.wgrad_ragged([it.dy for it, _, _ in part], [it.x for it, _, _ in part],
                                   [it.w.grad for it, _, _ in part], beta,
                                   [it.b.grad if it.b is not None else None for it, _, _ in part],
                                   ranges=[(first, cnt) for _, first, cnt in part])
        return done

    @staticmethod
    def _per_shape(items, key):
        """items in chunks of up to 32 of equal key(item), keys in first-appearance order"""
        groups = {}
        for it in items:
            groups.setdefault(key(it) + (it.N, it.beta), []).append(it)
        return [g[c0:c0 + 32] for g in groups.values() for c0 in range(0, len(g), 32)]

    def _flush_grouped(self) -> None:
        for chunk in self._per_shape(self.items, lambda it: (
                tuple(it.dy.shape), it.dy.stride(0), tuple(it.x.shape), it.x.stride(0))):
            it = chunk[0]
            if len(chunk) == 1:
                K.linear_wgrad(it.dy, it.x, it.N, it.w.grad, it.beta)
            else:
                K.wgrad_grouped([i.dy for i in chunk], [i.x for i in chunk], [i.w.grad for i in chunk], it.beta)

    def _flush_bias(self) -> None:
        for chunk in self._per_shape([it for it in self.items if it.b is not None],
                                     lambda it: (tuple(it.dy.shape), it.dy.stride(0))):
            it = chunk[0]
            if len(chunk) == 1:
                K.colsum(it.dy, it.N, it.b.grad, it.beta)
            else:
                K.colsum_grouped([i.dy for i in chunk], [i.b.grad for i in chunk], it.beta)


def _wgrad(rt, dy2, x2, N: int, w: Param, b: Optional[Param] = None) -> None:
    """dW (+ bias grad) of a Linear on the GPU: deferred (rt.wgrad) or now."""
    bt = _beta(rt)
    if rt.wgrad is not None:
        rt.wgrad.add(dy2, x2, N, w, b, bt, rt)
        return
    K.linear_wgrad(dy2, x2, N, w.grad, bt)
    if b is not None:
        K.colsum(dy2, N, b.grad, bt)
    _ready(rt, w, *([b] if b is not None else []))


def _fold_bias_later(rt, part, nparts: int, N: int, b: Param) -> None:
    """b's gradient = column sums of the [nparts, N] partials, folded with the
    queue's other deferred column reductions at the next flush."""
    rt.wgrad.defer_fold([(part, b.grad, nparts, N, _beta(rt))], (b,), rt)


def _fp8_grad_bias(g, g_slot: int, b: Param, rt, key: str):
    """e5m2 copy of the bf16 gradient g [M, N] and, from the same pass, the
    bias gradient (column sums) -- folded with the queue's other deferred
    column reductions at the next flush (one launch)."""
    g8, part, nparts = fp8.quantize_colsum(g, rt.fp8.gmeta, g_slot, key)
    _fold_bias_later(rt, part, nparts, g.shape[1], b)
    return g8
