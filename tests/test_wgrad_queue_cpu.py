"""The deferred weight-gradient queue's launch plan, on the CPU.

What WgradQueue launches and when is pure host arithmetic: whole waves of
tiles at layer ends, a cut problem staying at the queue head, the last layer
end flushing the remainder, deferred column folds before their parameters are
reported. The kernels are replaced by recording stubs and the tensors are CPU
tensors used only for their shapes and strides, so the tests assert the plan's
invariants, not numbers."""
import pytest
import torch

from tensorflow_distributed_on_gke_amd.models import layers
from tensorflow_distributed_on_gke_amd.models.layers import RunCtx, WgradQueue
from tensorflow_distributed_on_gke_amd.ops import fp8
from tensorflow_distributed_on_gke_amd.ops import kernels as K

TOK, WAVE, LAYERS = 128, 3, 4
# per layer: (name, N, K, has bias) -> ceil(N / 256) * ceil(K / 256) tiles.
# Tiles queued at the four layer ends: 5, 2 + 6, 2 + 5, 1 + 3, so with waves
# of 3 the launches cut inside `b`, then across `b` and `c` (both cut), then
# across `c`, `d` and `e`, and the last layer end flushes a partial wave of 4.
PROBLEMS = [
    [("a", 256, 256, True), ("b", 512, 264, False)],
    [("c", 520, 512, True)],
    [("d", 320, 256, True), ("e", 256, 768, False)],
    [("f", 256, 256, True), ("g", 320, 256, True)],
]


def _tiles(N, Kd):
    return -(-N // 256) * -(-Kd // 256)


class _P:
    """Stand-in for models.params.Param: the queue reads .grad and .shape."""

    def __init__(self, name, *shape):
        self.name, self.shape = name, shape
        self.grad = torch.empty(shape)


class _Rec:
    """The log of everything the queue launched or reported, by name."""

    def __init__(self):
        self.log = []
        self.names = {}

    def param(self, name, *shape):
        p = _P(name, *shape)
        self.names[id(p.grad)] = name
        return p

    def n(self, t):
        return None if t is None else self.names[id(t)]

    # the store
    def grad_ready(self, p):
        self.log.append(("ready", p.name))

    def grad_sync(self):
        self.log.append(("sync",))

    def where(self, kind):
        return [(i, e) for i, e in enumerate(self.log) if e[0] == kind]


@pytest.fixture
def rec(monkeypatch):
    r = _Rec()

    def wgrad_ragged(dys, xs, dws, beta=0.0, biases=None, ranges=None):
        biases = biases if biases is not None else [None] * len(dws)
        r.log.append(("ragged", [(r.n(w), r.n(b), tuple(rg)) for w, b, rg in zip(dws, biases, ranges)]))

    def linear_wgrad(dy2, x2, N, dw, beta=0.0):
        r.log.append(("gemm", [r.n(dw)]))

    def wgrad_grouped(dys, xs, dws, beta=0.0):
        r.log.append(("gemm", [r.n(w) for w in dws]))

    def colsum(x2, N, out, beta=0.0):
        r.log.append(("colsum", [r.n(out)]))

    def colsum_grouped(xs, outs, beta=0.0):
        r.log.append(("colsum", [r.n(o) for o in outs]))

    def reduce_partials_multi(items):
        r.log.append(("reduce", [r.n(out) for part, out, nparts, N, beta in items]))

    def wgrad_fp8(dy8s, sas, x8s, sbs, dws, beta=0.0):
        r.log.append(("fp8", [r.n(w) for w in dws]))

    for mod, fn in ((K, wgrad_ragged), (K, linear_wgrad), (K, wgrad_grouped), (K, colsum),
                    (K, colsum_grouped), (K, reduce_partials_multi), (fp8, wgrad_fp8)):
        monkeypatch.setattr(mod, fn.__name__, fn)
    return r


def _fold(rt, part, nparts, N, p):
    """Register a deferred column fold whose completion makes p's gradient ready."""
    layers._fold_bias_later(rt, part, nparts, N, p)


def _add(rec, rt, name, N, Kd, bias, tok=TOK):
    w = rec.param(name, N, Kd)
    b = rec.param(name + ".b", N) if bias else None
    rt.wgrad.add(torch.empty(tok, N), torch.empty(tok, Kd), N, w, b, 0.0, rt)


def _backward(rec, q):
    """One backward of LAYERS layers: per layer its weight gradients, one
    deferred fold and one fp8 weight gradient, then the layer end."""
    rt = RunCtx(training=True, store=rec, wgrad=q)
    for li, probs in enumerate(PROBLEMS):
        for name, N, Kd, bias in probs:
            _add(rec, rt, name, N, Kd, bias)
        _fold(rt, torch.empty(2 * 256), 2, 256, rec.param(f"ln{li}", 256))
        q.add_fp8(torch.empty(TOK, 256), None, torch.empty(TOK, 256), None,
                  rec.param(f"w8_{li}", 256, 256), 0.0, rt)
        q.layer_end()
        rec.log.append(("layer_end", li))
    q.flush()
    q.step_done()


def _chunked():
    q = WgradQueue(flush_at_boundary=True, wave_tiles=WAVE)
    q.layers_per_step = LAYERS
    assert q._chunking()
    return q


def test_wave_chunked_plan(rec):
    q = _chunked()
    _backward(rec, q)
    assert not q.items and q._cursor == 0
    log = rec.log
    order = [p for probs in PROBLEMS for p in probs]
    tiles = {name: _tiles(N, Kd) for name, N, Kd, _ in order}

    # every tile of every problem exactly once: the ranges partition [0, tiles) in order
    ranges, last_launch, bias_of = {}, {}, {}
    for i, (_, probs) in rec.where("ragged"):
        for w, b, rg in probs:
            ranges.setdefault(w, []).append(rg)
            last_launch[w] = i
            bias_of[w] = b
    assert set(ranges) == set(tiles)
    for name, rgs in ranges.items():
        end = 0
        for first, cnt in rgs:
            assert first == end and cnt > 0, (name, rgs)
            end += cnt
        assert end == tiles[name], (name, rgs)
        assert bias_of[name] == (name + ".b" if dict((p[0], p[3]) for p in order)[name] else None)
    assert len(ranges["b"]) == 2 and len(ranges["c"]) == 2 and len(ranges["e"]) == 2  # the cuts

    # whole waves before the last layer end, the partial remainder at it
    ends = [i for i, _ in rec.where("layer_end")]
    per_end = [sum(rg[1] for j, (_, probs) in rec.where("ragged") if lo < j < hi for _, _, rg in probs)
               for lo, hi in zip([-1] + ends[:-1], ends)]
    assert per_end == [3, 6, 6, 4]
    assert all(n and n % WAVE == 0 for n in per_end[:-1])
    assert not [j for j, _ in rec.where("ragged") if j > ends[-1]], "nothing left for the final flush"

    # ready: once each, after the launch of the last tile, weight then its bias, in queue order
    ready = [e[1] for _, e in rec.where("ready")]
    assert len(ready) == len(set(ready))
    at = {e[1]: i for i, e in rec.where("ready")}
    for name, _, _, bias in order:
        assert at[name] > last_launch[name]
        # (a cut problem is not reported by the launch of its first part)
        assert not [j for j, _ in rec.where("ragged") if last_launch[name] < j < at[name]]
        if bias:
            assert at[name + ".b"] == at[name] + 1
    assert [n for n in ready if n in tiles] == [p[0] for p in order]

    # every fold and every fp8 gradient launched once, before its parameter is ready
    for kind, names in (("reduce", [f"ln{li}" for li in range(LAYERS)]),
                        ("fp8", [f"w8_{li}" for li in range(LAYERS)])):
        launched = [(i, n) for i, (_, ns) in rec.where(kind) for n in ns]
        assert sorted(n for _, n in launched) == names
        for i, n in launched:
            assert i < at[n]
    assert set(at) == set(tiles) | {n + ".b" for n, _, _, b in order if b} | {
        f"ln{li}" for li in range(LAYERS)} | {f"w8_{li}" for li in range(LAYERS)}
    # a collective boundary after every batch of gradients
    assert log[max(at.values()) + 1] == ("sync",)

    # step_done() restarted the layer-end count: a second backward plans the same
    first, rec.log = rec.log, []
    _backward(rec, q)
    assert rec.log == first
    assert not q.items and q._cursor == 0


def test_unchunked_queue_launches_at_flush(rec):
    """Without wave chunking the layer ends launch nothing; boundary() flushes
    only a flush_at_boundary queue; one flush launches every tile."""
    for at_boundary in (False, True):
        rec.log = []
        q = WgradQueue(flush_at_boundary=at_boundary)
        q.layers_per_step = LAYERS
        rt = RunCtx(training=True, store=rec, wgrad=q)
        for name, N, Kd, bias in PROBLEMS[0] + PROBLEMS[1]:
            _add(rec, rt, name, N, Kd, bias)
        _fold(rt, torch.empty(2 * 256), 2, 256, rec.param("ln", 256))
        q.layer_end()
        assert rec.log == []
        q.boundary()
        assert bool(rec.log) == at_boundary
        q.flush()
        q.step_done()
        assert not q.items and q._cursor == 0
        (_, probs), = [e for _, e in rec.where("ragged")]
        assert sorted(probs) == [("a", "a.b", (0, 1)), ("b", None, (0, 4)), ("c", "c.b", (0, 6))]
        assert [e[1] for _, e in rec.where("reduce")] == [["ln"]]
        assert [e[1] for _, e in rec.where("ready")] == ["a", "a.b", "b", "c", "c.b", "ln"]


def test_odd_token_count_takes_the_grouped_path(rec):
    """One operand the ragged kernel does not take (token count not a multiple
    of 64) sends the whole flush to the per-shape launches and column sums."""
    q = _chunked()
    rt = RunCtx(training=True, store=rec, wgrad=q)
    _add(rec, rt, "a", 256, 256, True)
    _add(rec, rt, "odd", 256, 256, True, tok=100)
    _add(rec, rt, "b", 256, 256, True)
    _add(rec, rt, "c", 512, 264, False)
    _fold(rt, torch.empty(2 * 256), 2, 256, rec.param("ln", 256))
    q.layer_end()
    launched = list(rec.log)
    q.flush()
    assert rec.log == launched, "the layer end flushed everything"
    assert not q.items and q._cursor == 0
    assert not rec.where("ragged")
    gemms = [e[1] for _, e in rec.where("gemm")]
    assert sorted(gemms) == [["a", "b"], ["c"], ["odd"]]  # same shapes in one launch
    assert sorted(n for _, e in rec.where("colsum") for n in e[1]) == ["a.b", "b.b", "odd.b"]
    assert [e[1] for _, e in rec.where("reduce")] == [["ln"]]
    first_ready = rec.where("ready")[0][0]
    assert all(i < first_ready for k in ("gemm", "colsum", "reduce") for i, _ in rec.where(k))
    assert [e[1] for _, e in rec.where("ready")] == ["a", "a.b", "odd", "odd.b", "b", "b.b", "c", "ln"]
    assert rec.log[-1] == ("sync",)
