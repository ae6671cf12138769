"""Float64 / exact references, comparators, case tables and mutants for the
bf16 attention family (csrc/kernels/attn_impl.h, attn_fwd.h, attn_bwd.h,
attn_qkv.h): attn_fwd_kernel in its three shapes, attn_fwd_pipe_kernel,
attn_probs_kernel, attn_bwd_fused_kernel (plain and FDO), the register-staged
and the pipelined dQ / dK/dV pairs, and qkv_attn_fwd_kernel (self and cross).
No GPU needed.

Semantics (attn_impl.h header, key_window), evaluated in float64 from exactly
what a kernel receives -- bf16 q / k / v / dO, and for the backward the GIVEN
bf16 o and f32 lse:

  forward   P = softmax over the attended keys (key < kv_len[b], and key <= q
            when causal); masked keys get probability exactly 0; O = P V;
            lse = log2 sum exp2(c S), c = scale log2(e).
  kv_len 0  the row is uniform over all Lk keys, padding included, causal off,
            lse = log2 Lk; dQ / dK keep the real scale. kv_len None: all keys.
  backward  P = exp2(c S - lse) masked, delta = rowsum(dO o), dS = P (dP -
            delta), dQ = scale dS K, dK = scale dS^T Q, dV = P^T dO.

Two input families come from one builder (`build`):

  exact ("selection")  q and k are +-1 sign codes, every query the code of
      one attended key, the scale a power of two large enough that the
      selected key beats every other attended key by >= 160 in the log2 domain:
      every other probability underflows to exactly 0 in v_exp_f32, P is
      one-hot, O IS the selected V row, dV the scatter-add of the
      small-integer dO rows onto their selected keys, dQ and dK exactly +-0
      (dP_sel == delta in exact arithmetic). Every V row is distinct. The
      selected key sits, by turns over the queries, at the last attended key,
      the causal diagonal, the first / last key of a 16-key group and of a
      64-key tile, in a tile earlier than the row's last and in the last tile
      (SEL_MODES). A batch row with kv_len == 0 is uniform, not one-hot: it is
      held to the toleranced comparison below like every other element.
  toleranced  "flat" (logit standard deviation about 1), "peaky" (about 4),
      "ramp_up" / "ramp_down" (logits rising along the key index, so every
      tile grows the row maximum, and falling, so the __ballot(mn > m) skip is
      taken on every later tile), compared elementwise as
          |got - ref| <= 2^-8 |ref| + (2^-8 + tol) scale
      -- the first 2^-8 the bf16 store, the second the one bf16 MFMA operand
      the design rounds (P for O and dV, dS for dQ and dK), tol = 8 E the f32
      remainder; `scale` the float64 magnitude the operand rounding acts on
      (O: sum_k P|V|, dV: sum_q P|dO|, dQ: scale sum_k |dS||K|, dK: scale
      sum_q |dS||Q|). lse, delta and probs go through ref_tail.close_f32.

Buffers: every input is a strided view into a flat buffer whose gaps are NaN
(row stride > H hd, a gap between batch elements; for part of each table the
fused [B, L, 3, H, hd] and [B, S, layers 2d] layouts of the model). Every
output (o, dq, dk, dv, probs, the projection, lse and delta as slices of larger
buffers) is a view into a buffer filled with a quiet NaN with a payload: after
a launch every byte outside the views must be unchanged and no sentinel may be
left inside. K / V rows inside the tensor but outside a batch element's key
window are finite TRAP rows: K such that its logit beats every valid key's
(every query in the toleranced families; the trap's own query -- and, where all
queries select one key, every query -- in the exact one and, its queries being
projected in the kernel, in the cross-attention arm), V = +-2^14 with a sign
pattern of its own per row -- a mask that lets one such key in is a gross
error, not a 1 / Lk one. Traps are finite: the kernels multiply P = 0 by what
lies there. Batch elements with kv_len 0 or None attend those rows and carry
no traps.

`attn_f32` is the plain float32 PyTorch evaluation of the same formulas with
the design's roundings (bf16 P / dS operand, bf16 store) on the built
buffers; with `mutant=...` it is wrong in one line.
tests/test_attn_refs_cpu.py shows that `check` accepts the former and rejects
every mutant on the cases tests/test_gpu_attn.py runs. `expected_arm` mirrors
the launchers (fwd_hd, probs_hd, bwd_hd, tdg_attn_bwd_fdo, tdg_qkv_attn_fwd);
it exists only so the GPU tests can assert, through attn_last_plan, that the
arm a case is named after is the arm that ran.
"""
from __future__ import annotations

import functools
import math
from collections import namedtuple
from dataclasses import dataclass

import torch

import ref_gemm as G
import ref_tail as R
from ref_tail import BF16, F32, F64, MARGIN, Mismatch, tol  # noqa: F401

# --------------------------------------------------------------------------- tolerances
# Same form and discipline as ref_tail.E32: E32 is the worst ratio of the plain
# float32 PyTorch evaluation (no bf16 rounding anywhere) against the float64
# reference over the case tables below, err / scale for the bf16 outputs and
# err / (|ref| + scale) for the f32 ones, measured on the CPU by
# test_attn_refs_cpu.py::test_e_table_is_measured. The tolerance is MARGIN = 8
# times it (hardware exp2 / log2, another summation order, the online
# rescale). `kernel` is the worst ratio of the HIP kernels on the MI355X in
# the same unit: for the bf16 outputs the part of the error beyond the two
# 2^-8 terms (0: the whole error lay within them), with the largest fraction
# of the whole bound that any element used in brackets (2^-8 is the bound of
# ONE round-to-nearest at 8 significand bits, so a fraction near 1 is the
# design's two roundings both at their worst, not slack used up).
#
#   entry           E32        kernel          what
E32 = {
    "attn_o":      2.1e-5,   # 0 (0.81)       O; scale sum_k P |V|
    "attn_lse":    1.0e-3,   # 1.0e-3         lse; scale max_k |c S| over the attended keys (a row that attends one
                             #                key has lse = c S: the rounding of the dot product against the dot product)
    "attn_dv":     1.6e-5,   # 0 (0.96)       dV; scale sum_q P |dO|
    "attn_dq":     3.2e-6,   # 5.1e-8 (0.82)  dQ; see grad_scales
    "attn_dk":     2.5e-6,   # 1.5e-8 (0.94)  dK; see grad_scales
    "attn_delta":  5.8e-8,   # 4.5e-8         delta; scale sum |dO o|
    "attn_probs":  8.7e-7,   # 8.7e-7         attn_probs; scale P max_k |scale S|
}
R.register(E32)
BF16_ULP = R.BF16_ULP  # 2^-8

LOG2E = float(torch.tensor(1.4426950408889634, dtype=F32))  # attn_impl.h LOG2E as the f32 it is
SENT_BF16, SENT_F32 = G.SENT_BF16, G.SENT_F32
TRAP_V = 2.0 ** 14
GAP_LOG2 = 160.0  # below 2^-149, the smallest f32 subnormal: v_exp_f32 gives exactly 0

Arm = namedtuple("Arm", "family hd wgs threads wgs2")
# tdg_attn_last_plan's family word (attn_impl.h AttnPlanFamily)
FAMILY_CODE = {0: "fwd64", 1: "fwd128", 2: "fwd128w8", 3: "fwd_pipe", 4: "probs", 5: "bwd_fused",
               6: "bwd_fdo", 7: "bwd_split", 8: "bwd_pipe", 9: "qkv_self", 10: "qkv_cross"}
HDS = (16, 32, 64, 128)
# family word -> head dims it exists for
ARM_HDS = {"fwd64": HDS, "fwd128": (16, 32, 64), "fwd128w8": (128,), "fwd_pipe": (64,), "probs": HDS,
           "bwd_fused": HDS, "bwd_fdo": (64,), "bwd_split": (16, 32, 128), "bwd_pipe": (64,),
           "qkv_self": (64,), "qkv_cross": (64,)}
ARM_OP = {"fwd64": "fwd", "fwd128": "fwd", "fwd128w8": "fwd", "fwd_pipe": "fwd", "probs": "probs",
          "bwd_fused": "bwd", "bwd_fdo": "fdo", "bwd_split": "bwd", "bwd_pipe": "bwd",
          "qkv_self": "qkv_self", "qkv_cross": "qkv_cross"}
FWD_OPS = ("fwd", "qkv_self", "qkv_cross")
BWD_OPS = ("bwd", "fdo")


def cdiv(a, b):
    return -(-a // b)


def expected_arm(op, hd, Lq, Lk, B=4, H=3):
    """The launch fwd_hd / probs_hd / bwd_hd / tdg_attn_bwd_fdo /
    tdg_qkv_attn_fwd make: family, head dim, workgroups, threads, workgroups
    of the second (dK/dV) launch."""
    bh = B * H
    if op == "fwd":
        if hd == 64 and Lq > 128:
            return Arm("fwd_pipe", hd, cdiv(Lq, 128) * bh, 512, 0)
        if Lq > 64:
            return Arm("fwd128" if hd <= 64 else "fwd128w8", hd, cdiv(Lq, 128) * bh, 256 if hd <= 64 else 512, 0)
        return Arm("fwd64", hd, cdiv(Lq, 64) * bh, 256, 0)
    if op == "probs":
        return Arm("probs", hd, cdiv(bh * Lq, 4), 256, 0)
    if op == "bwd":
        if Lq <= 128 and Lk <= 128:
            return Arm("bwd_fused", hd, bh, 512, 0)
        if hd == 64:
            return Arm("bwd_pipe", hd, cdiv(Lq, 128) * bh, 256, cdiv(Lk, 128) * bh)
        return Arm("bwd_split", hd, cdiv(Lq, 64) * bh, 256, cdiv(Lk, 64) * bh)
    assert hd == 64 and Lq <= 128 and Lk <= 128, (op, hd, Lq, Lk)
    return Arm({"fdo": "bwd_fdo", "qkv_self": "qkv_self", "qkv_cross": "qkv_cross"}[op], 64, bh, 512, 0)


def plan_arm(plan):
    """tdg_attn_last_plan's five words as an Arm."""
    return Arm(FAMILY_CODE.get(int(plan[0]), "?"), *(int(x) for x in plan[1:5]))


# --------------------------------------------------------------------------- case tables
FAMILIES = ("exact", "flat", "peaky", "ramp_up", "ramp_down")
MASKS = ("none", "pad", "causal", "pad+causal")
LAYOUTS = ("gap", "fused")
SEL_MODES = ("last", "diag", "g16_first", "g16_last", "t64_first", "t64_last", "early_tile", "last_tile")


@dataclass(frozen=True)
class Case:
    op: str          # fwd | probs | bwd | fdo | qkv_self | qkv_cross
    family: str      # FAMILIES
    hd: int
    Lq: int
    Lk: int
    mask: str        # MASKS
    kv: tuple        # kv_len per batch element, or None
    layout: str      # "gap": every tensor its own padded buffer; "fused": the model's fused layouts
    B: int = 4
    H: int = 3
    seed: int = 0

    @property
    def causal(self):
        return "causal" in self.mask

    @property
    def arm(self):
        return expected_arm(self.op, self.hd, self.Lq, self.Lk, self.B, self.H)

    def what(self):
        return (f"{self.op} {self.family} hd{self.hd} Lq={self.Lq} Lk={self.Lk} {self.mask} kv={self.kv} "
                f"{self.layout} B={self.B} H={self.H}")


def kv_of(Lk, mask, k, B=4):
    """kv_len of a padded case: Lk, 0, 1 and a tile edge (64, 65 or Lk - 1,
    whichever fit, by turns), rotated over the batch elements."""
    if "pad" not in mask:
        return None
    edges = [e for e in (64, 65, Lk - 1) if 1 <= e <= Lk] or [Lk]
    base = [Lk, 0, 1, edges[k % len(edges)]]
    r = k % 4
    return tuple((base[r:] + base[:r])[:B])


# (Lq, Lk) points of every arm; `sq`: the points that also run causal
FWD64_PTS = [(q, k) for q in (1, 16, 17, 63, 64) for k in (1, 63, 64, 65, 129)]
FWD128_LK = (1, 127, 128, 129, 257)
PIPE_PTS = [(q, k) for q in (129, 256, 257) for k in (1, 64, 65, 128, 129, 192, 193, 257)] + [(193, 193)]
FUSED_PTS = [(q, k) for q in (1, 16, 17, 33, 127, 128) for k in (1, 17, 64, 65, 128)]
FUSED_SQ = ((1, 1), (17, 17), (128, 128))
SPLIT_PTS = [(1, 129), (129, 1), (129, 129), (130, 200), (200, 65)]
BWD_PIPE_PTS = [(1, 129), (129, 1), (129, 64), (64, 129), (129, 129), (257, 193), (193, 257), (321, 321)]
PROBS_LK = (1, 63, 64, 65, 200)
QKV_SELF_L = (1, 17, 64, 65, 127, 128)
QKV_CROSS_PTS = [(1, 128), (128, 1), (65, 64), (64, 65), (37, 128), (128, 77)]


def _walk(op, hd, pts, sq, families=FAMILIES, dense=False, B=4, H=3, causal_any=False):
    """One case per point (`dense`: one unpadded and one padded), walking
    family x mask x layout at coprime strides so that every factor meets every
    other over a table; the points of `sq` also get a causal and a
    pad + causal case."""
    out, k, kc = [], 0, 0

    def add(Lq, Lk, mask):
        nonlocal k, kc
        fam = families[k % len(families)]
        if "causal" in mask:  # (a turn of their own: every table's first causal case is of the first family)
            fam = families[kc % len(families)]
            kc += 1
        out.append(Case(op, fam, hd, Lq, Lk, mask, kv_of(Lk, mask, k, B), LAYOUTS[(k // 2 + k // 3) % 2], B, H,
                        seed=k))
        k += 1

    for (Lq, Lk) in pts:
        if dense:
            add(Lq, Lk, "none")
            add(Lq, Lk, "pad")
        else:
            add(Lq, Lk, ("pad", "none", "pad", "pad")[k % 4])
        if (Lq, Lk) in sq or causal_any:
            add(Lq, Lk, "causal")
            add(Lq, Lk, "pad+causal")
    return tuple(out)


@functools.lru_cache(maxsize=None)
def cases(arm, hd=64, H=3):
    """The case table of a kernel family word at a head dim (the qkv arms: at
    H heads, d = 64 H)."""
    op = ARM_OP[arm]
    assert hd in ARM_HDS[arm], (arm, hd)
    if arm == "fwd64":
        return _walk(op, hd, FWD64_PTS, {(1, 1), (63, 63), (64, 64)})
    if arm in ("fwd128", "fwd128w8"):
        lqs = (65, 127, 128) if hd == 64 else (65, 128, 129, 257)
        sq = [(65, 65), (128, 128)] + ([(129, 129)] if hd != 64 else [])
        pts = [(q, k) for q in lqs for k in FWD128_LK] + [(65, 65)]
        return _walk(op, hd, pts, set(sq))
    if arm == "fwd_pipe":
        return _walk(op, hd, PIPE_PTS, {(129, 129), (193, 193), (257, 257)})
    if arm in ("bwd_fused", "bwd_fdo"):
        return _walk(op, hd, FUSED_PTS, set(FUSED_SQ))
    if arm == "bwd_split":
        return _walk(op, hd, SPLIT_PTS, {(129, 129)}, dense=True)
    if arm == "bwd_pipe":
        return _walk(op, hd, BWD_PIPE_PTS, {(129, 129), (321, 321)}, dense=True)
    if arm == "probs":
        # (the kernel's causal window, key <= q, is defined for any Lq, Lk; the launchers of the
        # model use it with Lq == Lk only)
        return _walk(op, hd, [(5, k) for k in PROBS_LK], set(), dense=True, causal_any=True)
    fams = ("flat", "peaky")  # (q / k / v come out of the projection: no sign codes, no ramps)
    if arm == "qkv_self":
        return _walk(op, 64, [(L, L) for L in QKV_SELF_L], set(), families=fams, dense=True, H=H, causal_any=True)
    assert arm == "qkv_cross"
    return _walk(op, 64, QKV_CROSS_PTS, set(), families=fams, dense=True, H=H)


def all_tables():
    """(arm, hd, H, table) of everything tests/test_gpu_attn.py runs."""
    for arm, hds in ARM_HDS.items():
        if arm.startswith("qkv"):
            for H in (1, 2, 3):
                yield arm, 64, H, cases(arm, 64, H)
        else:
            for hd in hds:
                yield arm, hd, 3, cases(arm, hd)


# --------------------------------------------------------------------------- buffers
def sentinel(n, f32):
    return G.sentinel(n, f32)


class Flat:
    """One flat buffer and the views cut from it. Inputs: NaN everywhere a
    view does not cover. Outputs: the sentinel."""

    def __init__(self, n, dtype, out):
        self.out = out
        self.t = sentinel(n, dtype == F32) if out else torch.full((n,), float("nan"), dtype=dtype)
        self.views = {}

    def cut(self, name, shape, strides, offset):
        assert offset % 8 == 0 or self.t.dtype == F32
        self.views[name] = (tuple(shape), tuple(strides), offset)
        return self.t.as_strided(shape, strides, offset)

    def inside(self):
        m = torch.zeros(self.t.numel(), dtype=torch.bool)
        for shape, strides, off in self.views.values():
            m.as_strided(shape, strides, off).fill_(True)
        return m


def _gap(name, B, L, H, hd, out):
    """[B, L, H, hd] with 8 elements after every row, 24 after every batch
    element and a row before and after."""
    rs = H * hd + 8
    bs = L * rs + 24
    f = Flat(rs + B * bs + rs, BF16, out)
    f.cut(name, (B, L, H, hd), (bs, rs, hd, 1), rs)
    return f


def _fused3(names, B, L, H, hd, out):
    """The model's [B, L, 3, H, hd] projection output, 8 elements between
    batch elements."""
    rs = 3 * H * hd
    bs = L * rs + 8
    f = Flat(8 + B * bs + rs, BF16, out)
    for i, n in enumerate(names):
        f.cut(n, (B, L, H, hd), (bs, rs, hd, 1), 8 + i * H * hd)
    return f


def _kvlayers(names, B, S, H, hd, out, layers=3, layer=1):
    """K | V of decoder layer `layer` in the batched [B, S, layers * 2d] buffer."""
    d = H * hd
    rs = layers * 2 * d
    bs = S * rs + 8
    f = Flat(8 + B * bs + rs, BF16, out)
    for i, n in enumerate(names):
        f.cut(n, (B, S, H, hd), (bs, rs, hd, 1), 8 + layer * 2 * d + i * d)
    return f


def _rows2d(name, M, N, out, dtype=BF16, pad=8):
    """[M, N] with `pad` elements after every row (0: contiguous) and guards."""
    ld = N + pad
    g = max(ld, 64)
    f = Flat(g + M * ld + g, dtype, out)
    f.cut(name, (M, N), (ld, 1), g)
    return f


def _vec(name, shape, out):
    """A contiguous f32 tensor as a slice of a larger buffer."""
    n = math.prod(shape)
    f = Flat(64 + n + 64, F32, out)
    strides = [1] * len(shape)
    for i in range(len(shape) - 2, -1, -1):
        strides[i] = strides[i + 1] * shape[i + 1]
    f.cut(name, shape, strides, 64)
    return f


@dataclass
class Built:
    case: Case
    scale: float                 # the f32 scale argument, as a Python float
    pools: dict                  # pool name -> Flat
    where: dict                  # tensor name -> pool name
    kv: torch.Tensor             # int32 [B] or None
    sel: torch.Tensor = None     # exact family: selected key [B, H, Lq]
    modes: dict = None           # exact family: SEL_MODES realised -> count
    exact_rows: torch.Tensor = None  # bool [B]: batch elements held bitwise
    untouched: tuple = ()        # output-side buffers the launch must leave alone entirely

    def view(self, name, pool_tensors=None):
        """The strided view `name` of this case's buffers (or of the same
        buffers after a launch: pool name -> flat tensor)."""
        p = self.where[name]
        t = self.pools[p].t if pool_tensors is None else pool_tensors[p]
        return t.as_strided(*self.pools[p].views[name])

    def val(self, name):
        return self.view(name).to(F64)

    def outputs(self):
        return [p for p, f in self.pools.items() if f.out]

    def dev(self, device):
        """(pool name -> flat device tensor, tensor name -> device view)."""
        flat = {p: f.t.to(device) for p, f in self.pools.items()}
        views = {n: flat[p].as_strided(*self.pools[p].views[n]) for n, p in self.where.items()}
        return flat, views

    def kv_dev(self, device):
        return None if self.kv is None else self.kv.to(device)


def _gen(idx, c):
    return torch.Generator().manual_seed((idx * 1000003 + c.Lq * 7919 + c.Lk * 104729 + c.hd * 1299709 +
                                          c.seed * 15485863 + len(c.op) * 31 + c.H) % (2 ** 31 - 1))


def window(c: Case, mutant=None):
    """Per batch element: key limit, causal flag, logit factor (0: the
    uniform row of kv_len == 0) -- key_window."""
    klim, causal, lf = [], [], []
    for b in range(c.B):
        n = c.Lk if c.kv is None else c.kv[b]
        if c.kv is not None and n == 0:
            if mutant == "kv0_nothing":
                klim.append(0)
            else:
                klim.append(c.Lk)
            causal.append(c.causal if mutant == "kv0_causal_prefix" else False)
            lf.append(1.0 if mutant == "kv0_keeps_scale" else 0.0)
        else:
            n = min(n, c.Lk)
            if c.kv is not None and mutant == "window_wide":
                n = min(n + 1, c.Lk)
            if c.kv is not None and mutant == "window_narrow":
                n = n - 1
            klim.append(n)
            causal.append(c.causal)
            lf.append(1.0)
    return klim, causal, lf


def attends(c: Case, mutant=None):
    """bool [B, Lq, Lk]: does query q of batch element b attend to key k."""
    klim, causal, _ = window(c, mutant)
    keys = torch.arange(c.Lk).view(1, c.Lk)
    qs = torch.arange(c.Lq).view(c.Lq, 1)
    out = torch.empty(c.B, c.Lq, c.Lk, dtype=torch.bool)
    for b in range(c.B):
        m = (keys < klim[b]).expand(c.Lq, c.Lk)
        if causal[b]:
            if mutant == "diag_excluded":
                m = m & (keys < qs)
            elif mutant == "diag_plus1":
                m = m & (keys <= qs + 1)
            else:
                m = m & (keys <= qs)
        out[b] = m
    return out


def _select(c: Case):
    """Exact family: the selected key of every (b, h, q), by turns over
    SEL_MODES (a mode that does not fit the row falls back to "last"), and
    how often each mode was realised."""
    klim, causal, _ = window(c)
    sel = torch.zeros(c.B, c.H, c.Lq, dtype=torch.int64)
    modes = {m: 0 for m in SEL_MODES}
    for b in range(c.B):
        for i in range(c.Lq):
            n = min(klim[b], i + 1) if causal[b] else klim[b]  # attended keys: [0, n)
            nt = cdiv(n, 64)
            for h in range(c.H):
                mode = SEL_MODES[(i + h + 3 * b) % len(SEL_MODES)]
                key = None
                if mode == "diag" and causal[b] and i < klim[b]:
                    key = i
                elif mode == "g16_first":
                    key = 16 * ((7 * i + h) % cdiv(n, 16))
                elif mode == "g16_last" and n >= 16:
                    key = 16 * ((5 * i + h) % (n // 16)) + 15
                elif mode == "t64_first":
                    key = 64 * ((i + h) % nt)
                elif mode == "t64_last" and n >= 64:
                    key = 64 * ((i + h) % (n // 64)) + 63
                elif mode == "early_tile" and nt >= 2:
                    key = 64 * ((i + h) % (nt - 1)) + (11 * i) % 64
                elif mode == "last_tile" and nt >= 2:
                    key = 64 * (nt - 1) + (13 * i) % (n - 64 * (nt - 1))
                if key is None:
                    mode, key = "last", n - 1
                assert 0 <= key < n
                modes[mode] += 1
                sel[b, h, i] = key
    return sel, modes


def _codes(g, B, L, H, hd):
    """+-1 codes [B, L, H, hd], distinct within every (b, h)."""
    nb = min(hd, 20)
    w = 2 ** torch.arange(nb)
    out = (torch.randint(0, 2, (B, L, H, hd), generator=g) * 2 - 1).to(F64)
    for b in range(B):
        for h in range(H):
            ids = torch.randperm(2 ** nb, generator=g)[:L] if nb < 20 else \
                torch.unique(torch.randint(0, 2 ** nb, (4 * L + 64,), generator=g))[:L]
            ids = ids[torch.randperm(L, generator=g)]
            out[b, :, h, :nb] = ((ids.view(L, 1) // w) % 2 * 2 - 1).to(F64)
    return out


def _inputs(c: Case):
    """(q, k, v, dO, scale, sel, modes) of an attention case as float64
    tensors holding bf16 values; dO None for the forward-only ops."""
    B, H, hd, Lq, Lk = c.B, c.H, c.hd, c.Lq, c.Lk
    klim, _, lf = window(c)
    g = _gen(1, c)
    bwd = c.op in BWD_OPS
    sel = modes = None
    if c.family == "exact":
        sel, modes = _select(c)
        k = _codes(g, B, Lk, H, hd)
        q = torch.gather(k.permute(0, 2, 1, 3), 2, sel.view(B, H, Lq, 1).expand(B, H, Lq, hd)).permute(0, 2, 1, 3)
        v = torch.randint(-8, 9, (B, Lk, H, hd), generator=g).to(F64)
        do = torch.randint(-1, 2, (B, Lq, H, hd), generator=g).to(F64)
        # the smallest lead of a selected key over another attended key fixes the scale
        S = torch.einsum("bqhd,bkhd->bhqk", q, k)
        other = S.masked_fill(~attends(c)[:, None], -math.inf)
        other.scatter_(3, sel.view(B, H, Lq, 1), -math.inf)
        rows = torch.tensor([f > 0 for f in lf]).view(B, 1, 1)
        lead = (hd - other.max(-1).values)[rows.expand(B, H, Lq)]
        lead = float(lead.min()) if lead.numel() else math.inf
        lead = float(hd) if math.isinf(lead) else lead  # (no row has a second attended key)
        assert lead >= 2, c.what()
        scale = 2.0 ** math.ceil(math.log2(GAP_LOG2 / (LOG2E * lead)))
    else:
        amp = 4.0 if c.family == "peaky" else 1.0
        q = torch.randn(B, Lq, H, hd, generator=g)
        q[..., 0] = 0.5 + q[..., 0].abs()  # (positive: a trap key's logit beats every valid key's for every query)
        q = q * amp
        k = torch.randn(B, Lk, H, hd, generator=g)
        if c.family.startswith("ramp"):
            j = torch.arange(Lk, dtype=torch.float32)
            ramp = (j if c.family == "ramp_up" else (Lk - 1 - j)) * (math.sqrt(hd) / 16)
            k = 0.125 * k
            k[..., 0] = ramp.view(1, Lk, 1)
        v = torch.randn(B, Lk, H, hd, generator=g)
        do = torch.randn(B, Lq, H, hd, generator=g)
        scale = 1.0 / math.sqrt(hd)
    q, k, v, do = (t.to(BF16).to(F64) for t in (q, k, v, do))
    # trap rows: inside the tensor, outside the key window
    tg = _gen(2, c)
    for b in range(B):
        if lf[b] == 0 or klim[b] >= Lk:
            continue
        n = Lk - klim[b]
        if c.family == "exact":
            idx = torch.arange(klim[b], Lk) % Lq
            k[b, klim[b]:] = 2 * q[b, idx]
        else:
            k[b, klim[b]:] = 0
            k[b, klim[b]:, :, 0] = float(torch.tensor(64 * math.sqrt(hd)).to(BF16))
        v[b, klim[b]:] = (torch.randint(0, 2, (n, H, hd), generator=tg) * 2 - 1).to(F64) * TRAP_V
    scale = float(torch.tensor(scale, dtype=F32))
    return q, k, v, (do if bwd else None), scale, sel, modes


def c_of(scale):
    """c = scale * LOG2E as the kernels form it: an f32 product."""
    return float(torch.tensor(scale, dtype=F32) * torch.tensor(LOG2E, dtype=F32))


# --------------------------------------------------------------------------- the mathematics, in any dtype
MUTANTS = ("window_wide", "window_narrow", "diag_excluded", "diag_plus1", "lse_natural", "kv0_nothing",
           "kv0_causal_prefix", "kv0_keeps_scale", "no_delta", "dk_unscaled", "dq_scaled_twice",
           "rescale_skipped", "v_swap16", "tail_rows_unwritten", "row_at_Lq", "dkdv_tail_unwritten",
           "p_unrounded")
ACCEPTED_MUTANTS = ("p_unrounded",)  # the bound is one-sided: a kernel more exact than the design passes
# which operations a mutant can change at all
MUTANT_OPS = {
    "window_wide": FWD_OPS + BWD_OPS + ("probs",), "window_narrow": FWD_OPS + BWD_OPS + ("probs",),
    # (cross-attention is never causal)
    "diag_excluded": ("fwd", "qkv_self", "probs") + BWD_OPS, "diag_plus1": ("fwd", "qkv_self", "probs") + BWD_OPS,
    "lse_natural": FWD_OPS + BWD_OPS,
    "kv0_nothing": FWD_OPS + BWD_OPS + ("probs",), "kv0_causal_prefix": ("fwd", "qkv_self", "probs") + BWD_OPS,
    "kv0_keeps_scale": FWD_OPS + BWD_OPS + ("probs",),
    "no_delta": BWD_OPS, "dk_unscaled": BWD_OPS, "dq_scaled_twice": BWD_OPS,
    "rescale_skipped": ("fwd",),  # (the fused-projection kernels take all <= 128 keys as one tile)
    "v_swap16": FWD_OPS + BWD_OPS,
    "tail_rows_unwritten": FWD_OPS + BWD_OPS + ("probs",), "row_at_Lq": FWD_OPS + BWD_OPS + ("probs",),
    "dkdv_tail_unwritten": BWD_OPS, "p_unrounded": FWD_OPS + BWD_OPS,
}


def _bf(x):
    return x.to(BF16).to(x.dtype)


def _ftz(p):
    """v_exp_f32 as the kernels use it (attn_impl.h fast_exp2): results below
    2^-126 are flushed to zero. Part of the semantics: it is what makes the
    exact family's P one-hot."""
    return torch.where(p < 2.0 ** -126, torch.zeros_like(p), p)


def fwd_math(c: Case, q, k, v, scale, dt=F64, mutant=None, rounded=False):
    """Forward in dtype dt. rounded: the design's bf16 P operand (the
    unnormalised exp2, divided by the unrounded sum). Returns a dict: z = c S
    (kv_len == 0 rows: 0), att, P, O [B, Lq, H, hd], lse [B, H, Lq]."""
    q, k, v = (t.to(dt) for t in (q, k, v))
    if mutant == "v_swap16":
        v = _swap16(v)
    _, _, lf = window(c, mutant)
    att = attends(c, mutant)[:, None]
    cc = torch.tensor(c_of(scale), dtype=dt) * torch.tensor(lf, dtype=dt).view(c.B, 1, 1, 1)
    z = torch.einsum("bqhd,bkhd->bhqk", q, k) * cc
    zm = z.masked_fill(~att, -math.inf)
    m = zm.max(-1, keepdim=True).values
    mu = m
    if mutant == "rescale_skipped":  # every 64-key tile keeps the maximum it met
        nt = cdiv(c.Lk, 64)
        pad = torch.full(z.shape[:3] + (nt * 64 - c.Lk,), -math.inf, dtype=dt)
        tmax = torch.cat([zm, pad], -1).view(*z.shape[:3], nt, 64).max(-1).values
        mu = torch.cummax(tmax, -1).values.repeat_interleave(64, -1)[..., :c.Lk]
    mu = torch.where(torch.isfinite(mu), mu, torch.zeros_like(mu))
    p = torch.where(att, _ftz(torch.exp2(z - mu)), torch.zeros_like(z))
    l = p.sum(-1, keepdim=True)
    inv = torch.where(l > 0, 1 / l, torch.zeros_like(l))
    pv = _bf(p) if (rounded and mutant != "p_unrounded") else p
    O = (torch.einsum("bhqk,bkhd->bqhd", pv, v) * inv.squeeze(-1).permute(0, 2, 1).unsqueeze(-1))
    mf = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    lse = torch.where(l > 0, mf + torch.log2(l.clamp_min(1e-300)), torch.full_like(l, math.inf)).squeeze(-1)
    if mutant == "lse_natural":
        lse = lse / LOG2E
    return dict(z=z, att=att, P=p * inv, O=O, lse=lse)


def _swap16(v):
    """Keys 3 and 5 of every whole 16-key group swapped."""
    v = v.clone()
    n = v.shape[1] // 16
    if n:
        a = torch.arange(n) * 16 + 3
        b = a + 2
        va = v[:, a].clone()
        v[:, a] = v[:, b]
        v[:, b] = va
    return v


def bwd_math(c: Case, q, k, v, o, do, lse, scale, dt=F64, mutant=None, rounded=False):
    """Backward as a function of (q, k, v, o, dO, lse) in dtype dt. rounded:
    the design's bf16 P / dS operands. Returns dq, dk, dv, delta [B, H, Lq],
    P, dS (unrounded)."""
    q, k, v, o, do, lse = (t.to(dt) for t in (q, k, v, o, do, lse))
    if mutant == "v_swap16":
        v = _swap16(v)
    _, _, lf = window(c, mutant)
    att = attends(c, mutant)[:, None]
    cc = torch.tensor(c_of(scale), dtype=dt) * torch.tensor(lf, dtype=dt).view(c.B, 1, 1, 1)
    z = torch.einsum("bqhd,bkhd->bhqk", q, k) * cc
    L = lse.unsqueeze(-1)
    if mutant == "lse_natural":
        L = L * LOG2E
    P = torch.where(att, _ftz(torch.exp2(z - L)), torch.zeros_like(z))
    delta = (do * o).sum(-1).permute(0, 2, 1)
    dP = torch.einsum("bqhd,bkhd->bhqk", do, v)
    dS = P * (dP if mutant == "no_delta" else dP - delta.unsqueeze(-1))
    rnd = rounded and mutant != "p_unrounded"
    Pr, dSr = (_bf(P), _bf(dS)) if rnd else (P, dS)
    s = torch.tensor(scale, dtype=dt)
    dv = torch.einsum("bhqk,bqhd->bkhd", Pr, do)
    dq = torch.einsum("bhqk,bkhd->bqhd", dSr, k) * (s * s if mutant == "dq_scaled_twice" else s)
    dk = torch.einsum("bhqk,bqhd->bkhd", dSr, q) * (1 if mutant == "dk_unscaled" else s)
    return dict(dq=dq, dk=dk, dv=dv, delta=delta, P=P, dS=dS)


def probs_math(c: Case, q, k, scale, dt=F64, mutant=None):
    """attn_probs: the softmax rows [B, H, Lq, Lk] (natural exponent)."""
    q, k = q.to(dt), k.to(dt)
    _, _, lf = window(c, mutant)
    att = attends(c, mutant)[:, None]
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) * (torch.tensor(scale, dtype=dt) *
                                                 torch.tensor(lf, dtype=dt).view(c.B, 1, 1, 1))
    sm = s.masked_fill(~att, -math.inf)
    m = sm.max(-1, keepdim=True).values
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = torch.where(att, _ftz(torch.exp(s - m)), torch.zeros_like(s))
    l = e.sum(-1, keepdim=True)
    return e * torch.where(l > 0, 1 / l, torch.zeros_like(l)), s, att


# --------------------------------------------------------------------------- builder
@functools.lru_cache(maxsize=8)
def build(c: Case) -> Built:
    B, H, hd, Lq, Lk = c.B, c.H, c.hd, c.Lq, c.Lk
    d = H * hd
    kv = None if c.kv is None else torch.tensor(c.kv, dtype=torch.int32)
    pools, vals = {}, {}
    fused = c.layout == "fused"

    def put(pool, f, **tensors):
        pools[pool] = f
        for n, t in tensors.items():
            if t is not None:
                f.t.as_strided(*f.views[n]).copy_(t.to(f.t.dtype))

    if c.op in ("qkv_self", "qkv_cross"):
        g = _gen(3, c)
        npj = 3 if c.op == "qkv_self" else 1
        M = B * Lq
        x = torch.randn(M, d, generator=g)
        w = torch.randn(npj * d, d, generator=g) / math.sqrt(d)
        if c.family == "peaky":
            w[:d] *= 4.0
        bias = 0.1 * torch.randn(npj * d, generator=g)
        put("x", _rows2d("x", M, d, False), x=x)
        put("w", _rows2d("w", npj * d, d, False), w=w)
        fb = Flat(npj * d + 5, F32, False)
        fb.cut("bias", (npj * d,), (1,), 0)
        put("bias", fb, bias=bias)
        put("qkv", _rows2d("qkv", M, npj * d, True, pad=0))
        put("o", _gap("o", B, Lq, H, hd, True))
        put("lse", _vec("lse", (B, H, Lq), True))
        scale = float(torch.tensor(1.0 / math.sqrt(hd), dtype=F32))
        if c.op == "qkv_cross":
            gk = _gen(4, c)
            k = torch.randn(B, Lk, H, hd, generator=gk).to(BF16).to(F64)
            v = torch.randn(B, Lk, H, hd, generator=gk).to(BF16).to(F64)
            klim, _, lf = window(c)
            qp = (x.to(BF16).double() @ w.to(BF16).double().T + bias.double()).view(B, Lq, H, hd)
            for b in range(B):  # trap rows: K along the sign pattern of one projected query each
                if lf[b] and klim[b] < Lk:
                    n = Lk - klim[b]
                    k[b, klim[b]:] = 4.0 * torch.sign(qp[b, torch.arange(klim[b], Lk) % Lq]) + 0.0
                    v[b, klim[b]:] = (torch.randint(0, 2, (n, H, hd), generator=gk) * 2 - 1).to(F64) * TRAP_V
            put("kvl", _kvlayers(("k", "v"), B, Lk, H, hd, False), k=k, v=v)
        bt = Built(c, scale, pools, {}, kv)
    else:
        q, k, v, do, scale, sel, modes = _inputs(c)
        if fused and Lq == Lk:
            put("qkv_in", _fused3(("q", "k", "v"), B, Lq, H, hd, False), q=q, k=k, v=v)
        else:
            put("q", _gap("q", B, Lq, H, hd, False), q=q)
            if fused:
                put("kv_in", _kvlayers(("k", "v"), B, Lk, H, hd, False), k=k, v=v)
            else:
                put("k", _gap("k", B, Lk, H, hd, False), k=k)
                put("v", _gap("v", B, Lk, H, hd, False), v=v)
        if c.op == "probs":
            put("probs", _vec("probs", (B, H, Lq, Lk), True))
        elif c.op == "fwd":
            put("o", _gap("o", B, Lq, H, hd, True))
            put("lse", _vec("lse", (B, H, Lq), True))
        else:
            f = fwd_math(c, q, k, v, scale)
            put("o", _gap("o", B, Lq, H, hd, False), o=f["O"])
            put("lse", _vec("lse", (B, H, Lq), False), lse=f["lse"])
            if c.op == "bwd":
                put("do", _gap("do", B, Lq, H, hd, False), do=do)
            else:  # FDO: dO = dy2 @ wo per head, formed in the kernel
                gw = _gen(5, c)
                if c.family == "exact":  # a signed permutation: dO is dy2's small integers, exactly
                    wo = torch.zeros(d, d)
                    wo[torch.arange(d), torch.randperm(d, generator=gw)] = \
                        (torch.randint(0, 2, (d,), generator=gw) * 2 - 1).float()
                    dy = do.reshape(B * Lq, d).float() @ wo.T
                else:
                    wo = torch.randn(d, d, generator=gw) / math.sqrt(d)
                    dy = torch.randn(B * Lq, d, generator=gw)
                put("dy2", _rows2d("dy2", B * Lq, d, False), dy2=dy)
                put("wo", _rows2d("wo", d, d, False), wo=wo)
            if fused and Lq == Lk:
                put("dqkv", _fused3(("dq", "dk", "dv"), B, Lq, H, hd, True))
            else:
                put("dq", _gap("dq", B, Lq, H, hd, True))
                if fused:
                    put("dkv", _kvlayers(("dk", "dv"), B, Lk, H, hd, True))
                else:
                    put("dk", _gap("dk", B, Lk, H, hd, True))
                    put("dv", _gap("dv", B, Lk, H, hd, True))
            put("delta", _vec("delta", (B, H, Lq), True))
        bt = Built(c, scale, pools, {}, kv, sel, modes)
        if c.op in BWD_OPS and c.arm.family in ("bwd_fused", "bwd_fdo"):
            # delta is the workspace the dQ kernel of the two-launch arms fills for the dK/dV
            # kernel; the fused kernel keeps it in LDS and must not write the buffer it is given
            bt.untouched = ("delta",)
        if c.family == "exact":
            bt.exact_rows = torch.tensor([x > 0 for x in window(c)[2]])
    for p, f in pools.items():
        for n in f.views:
            assert n not in bt.where
            bt.where[n] = p
    if c.family == "exact":
        _assert_exact(bt)
    return bt


def exact_expect(bt: Built, do=None):
    """What the exact family gives bitwise in the batch elements of
    bt.exact_rows: O = the selected V rows; dV = the scatter-add of the dO
    rows onto their selected keys; dQ = dK = 0."""
    c = bt.case
    v = bt.val("v")
    idx = bt.sel.view(c.B, c.H, c.Lq, 1).expand(c.B, c.H, c.Lq, c.hd)
    O = torch.gather(v.permute(0, 2, 1, 3), 2, idx).permute(0, 2, 1, 3)
    out = dict(O=O)
    if do is not None:
        dv = torch.zeros(c.B, c.H, c.Lk, c.hd, dtype=F64)
        dv.scatter_add_(2, idx, do.to(F64).permute(0, 2, 1, 3))
        out["dv"] = dv.permute(0, 2, 1, 3)
    return out


def dout_f32(bt: Built):
    """The bf16 dO a backward case works on: the given one, or for FDO the
    float32 dy2 @ wo rounded to bf16, as linear_dgrad stores it."""
    c = bt.case
    if c.op == "bwd":
        return bt.view("do")
    y = (bt.view("dy2").to(F32) @ bt.view("wo").to(F32)).to(BF16)
    return y.view(c.B, c.Lq, c.H, c.hd)


def _assert_exact(bt: Built):
    """The exact family's premises: P one-hot on the selected key wherever the
    row is not uniform, distinct V rows, dV representable in bf16."""
    c = bt.case
    q, k, v = bt.val("q"), bt.val("k"), bt.val("v")
    f = fwd_math(c, q, k, v, bt.scale)
    rows = bt.exact_rows
    onehot = torch.zeros_like(f["P"]).scatter_(3, bt.sel.view(c.B, c.H, c.Lq, 1), 1.0)
    assert bool(((f["P"] - onehot).abs()[rows] < 2.0 ** -150).all()), c.what()
    for b in range(c.B):
        for h in range(c.H):
            assert torch.unique(v[b, :, h], dim=0).shape[0] == c.Lk, c.what()
    if c.op in BWD_OPS:
        dv = exact_expect(bt, dout_f32(bt))["dv"]
        assert bool((dv.to(BF16).to(F64) == dv).all()), c.what() + ": dV not representable"


def check_pristine(bt: Built):
    """Guards, poison and traps are in place before any kernel runs."""
    c = bt.case
    for p, f in bt.pools.items():
        ins = f.inside()
        assert bool(ins.any()) and not bool(ins.all())
        if f.out:
            R.exact(f.t, sentinel(f.t.numel(), f.t.dtype == F32), f"{p} before the launch")
        else:
            assert bool(f.t[~ins].isnan().all()) and bool(torch.isfinite(f.t[ins]).all()), (c.what(), p)
        for n, (shape, strides, off) in f.views.items():
            if len(shape) == 4 and f.t.dtype == BF16:
                assert strides[1] > c.H * c.hd and strides[1] % 8 == 0 and strides[0] > shape[1] * strides[1], (p, n)
    if c.op in ("fwd", "bwd", "fdo", "probs", "qkv_cross") and c.kv is not None:
        klim, _, lf = window(c)
        for b in range(c.B):
            if lf[b] and klim[b] < c.Lk and c.op != "probs":
                assert bool((bt.val("v")[b, klim[b]:].abs() == TRAP_V).all())


# --------------------------------------------------------------------------- comparators
def _fail(what, msg):
    raise Mismatch(f"{what}: {msg}")


FRACTION: dict = {}  # entry -> the largest err / bound any element reached


def close_bf16(got, ref, scale, key, what, scale32=None):
    """bf16 output against the float64 reference, every element:
    |got - ref| <= 2^-8 |ref| + 2^-8 scale + tol(key) scale32 (scale32 = scale
    unless given: see grad_scales). Records the part of the error beyond the
    two 2^-8 terms, / scale32 (the unit of E32)."""
    if got.dtype != BF16:
        _fail(what, f"dtype {got.dtype}")
    g, ref, scale = got.to(F64), ref.to(F64), scale.to(F64)
    scale32 = scale if scale32 is None else scale32.to(F64)
    if g.shape != ref.shape:
        _fail(what, f"shape {tuple(g.shape)} vs {tuple(ref.shape)}")
    if not bool(torch.isfinite(g).all()):
        _fail(what, f"{int((~torch.isfinite(g)).sum())} non-finite values")
    err = (g - ref).abs()
    base = BF16_ULP * (ref.abs() + scale)
    bound = base + tol(key) * scale32
    excess = (err - base).clamp_min(0)
    ratio = torch.where(excess > 0, excess / scale32.clamp_min(1e-300), torch.zeros_like(err))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    R._note(key, worst)
    frac = torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    FRACTION[key] = max(FRACTION.get(key, 0.0), min(float(frac.max()) if frac.numel() else 0.0, 1e30))
    if worst > tol(key):
        i = int(ratio.argmax())
        idx = tuple(int(x) for x in torch.unravel_index(torch.tensor(i), g.shape))
        _fail(what, f"[{key}] at {idx}: got {g.flatten()[i].item()!r} ref {ref.flatten()[i].item()!r} scale "
                    f"{scale.flatten()[i].item():.3e} / {scale32.flatten()[i].item():.3e}: excess {worst:.3e} > "
                    f"{tol(key):.3e} (x scale32)")
    return worst


def report():
    return R.report() + "  | fraction of the bound used: " + \
        "  ".join(f"{k}={v:.2f}" for k, v in sorted(FRACTION.items()))


def _same_values(got, ref, what):
    """Equal as numbers, element by element (bitwise up to the sign of zero)."""
    g, r = got.to(F64), ref.to(F64)
    ok = g == r
    if not bool(ok.all()):
        i = int((~ok).flatten().nonzero()[0])
        idx = tuple(int(x) for x in torch.unravel_index(torch.tensor(i), g.shape))
        _fail(what, f"{int((~ok).sum())} elements differ from the exact result, first at {idx}: "
                    f"{g.flatten()[i].item()!r} vs {r.flatten()[i].item()!r}")


def check_guards(bt: Built, after: dict):
    """Every output buffer: bytes outside the views bitwise unchanged, no
    sentinel left inside. Every input buffer: unchanged."""
    what = bt.case.what()
    for p, f in bt.pools.items():
        a = after[p].cpu()
        if a.dtype != f.t.dtype or a.numel() != f.t.numel():
            _fail(what, f"{p}: buffer changed type or size")
        ai, bi = G._as_int(a), G._as_int(f.t)
        if not f.out:
            if not bool((ai == bi).all()):
                _fail(what, f"input buffer {p} was written")
            continue
        ins = f.inside()
        if p in bt.untouched:
            ins = torch.zeros_like(ins)
        bad = (ai != bi) & ~ins
        if bool(bad.any()):
            i = int(bad.nonzero()[0])
            _fail(what, f"{p}: guard overwritten at flat element {i} ({int(bad.sum())} in all); views "
                        f"{f.views}")
        sent = SENT_F32 if a.dtype == F32 else SENT_BF16
        for n, (shape, strides, off) in ({} if p in bt.untouched else f.views).items():
            left = ai.as_strided(shape, strides, off) == sent
            if bool(left.any()):
                i = int(left.flatten().nonzero()[0])
                idx = tuple(int(x) for x in torch.unravel_index(torch.tensor(i), shape))
                _fail(what, f"{n}: {int(left.sum())} elements never written, first at {idx}")


def _o_scale(P, v):
    return torch.einsum("bhqk,bkhd->bqhd", P, v.abs())


def grad_scales(r, q, k, v, o, do, s):
    """The comparator scales of a backward result r = bwd_math(...), float64.
    dv: sum_q P |dO|. dq / dk: `scale` sum |dS| |K| (|Q|), what the bf16
    rounding of the dS operand acts on -- and, for the tol term alone, the
    same sums over P (sum_d |dO||V| + sum_d |dO||o|) in place of |dS|: dS =
    P (dP - delta) is a difference, exactly 0 in a row that attends one key
    (P = 1, o = V), and no float32 evaluation of dP and delta, PyTorch's or a
    kernel's, leaves less than their own rounding there."""
    ds32 = r["P"] * (torch.einsum("bqhd,bkhd->bhqk", do.abs(), v.abs()) +
                     (do * o).abs().sum(-1).permute(0, 2, 1).unsqueeze(-1))
    return dict(
        dv=torch.einsum("bhqk,bqhd->bkhd", r["P"], do.abs()),
        dq=s * torch.einsum("bhqk,bkhd->bqhd", r["dS"].abs(), k.abs()),
        dk=s * torch.einsum("bhqk,bqhd->bkhd", r["dS"].abs(), q.abs()),
        dq32=s * torch.einsum("bhqk,bkhd->bqhd", ds32, k.abs()),
        dk32=s * torch.einsum("bhqk,bqhd->bkhd", ds32, q.abs()),
        delta=(do * o).abs().sum(-1).permute(0, 2, 1))


def _check_fwd(bt: Built, q, k, v, got_o, got_lse, what):
    c = bt.case
    f = fwd_math(c, q, k, v, bt.scale)
    close_bf16(got_o, f["O"], _o_scale(f["P"], v), "attn_o", what + " O")
    zmax = f["z"].abs().masked_fill(~f["att"], 0.0).max(-1).values
    R.close_f32(got_lse, f["lse"], "attn_lse", what + " lse", scale=zmax)
    if bt.exact_rows is not None:
        rows = bt.exact_rows
        _same_values(got_o[rows], exact_expect(bt)["O"][rows], what + " O (selected V rows)")
    return f


def check(bt: Built, after: dict, dout=None, o=None, lse=None):
    """Everything a launch on bt's buffers must satisfy. after: pool name ->
    flat tensor after the launch. dout (FDO): the bf16 dO [B, Lq, H, hd] the
    kernel's in-kernel projection stands for. o / lse: what the backward was
    given instead of the built bf16(ref O) / f32(ref lse) (the chained test)."""
    c = bt.case
    what = c.what()
    after = {p: t.cpu() for p, t in after.items()}
    check_guards(bt, after)
    got = lambda n: bt.view(n, after)  # noqa: E731
    if c.op == "probs":
        ref, s, att = probs_math(c, bt.val("q"), bt.val("k"), bt.scale)
        g = got("probs")
        smax = s.abs().masked_fill(~att, 0.0).max(-1, keepdim=True).values
        R.close_f32(g, ref, "attn_probs", what + " probs", scale=ref * smax)
        if bool((g.masked_select(~att.expand_as(g)) != 0).any()):
            _fail(what, "probability outside the key window not exactly 0")
        dev = (g.to(F64).sum(-1) - 1).abs().max()
        if float(dev) > (c.Lk + 4) * 2.0 ** -24:
            _fail(what, f"rows do not sum to 1: off by {float(dev):.3e}")
        return
    if c.op in ("qkv_self", "qkv_cross"):
        d = c.H * c.hd
        x, w, bias = bt.val("x"), bt.val("w"), bt.val("bias")
        pre = x @ w.T + bias
        ref = G.Ref(pre, pre, x.abs() @ w.abs().T, None)
        G.close_out(got("qkv"), ref, 1.0, 0.0, torch.zeros_like(pre), what + " projection", "tile")
        # the attention reference starts from the kernel's own bf16 projection
        proj = got("qkv").to(F64)
        if c.op == "qkv_self":
            p5 = proj.view(c.B, c.Lq, 3, c.H, c.hd)
            q, k, v = p5[:, :, 0], p5[:, :, 1], p5[:, :, 2]
        else:
            q, k, v = proj.view(c.B, c.Lq, c.H, c.hd), bt.val("k"), bt.val("v")
        _check_fwd(bt, q, k, v, got("o"), got("lse"), what)
        return
    q, k, v = bt.val("q"), bt.val("k"), bt.val("v")
    if c.op == "fwd":
        _check_fwd(bt, q, k, v, got("o"), got("lse"), what)
        return
    do = (dout_f32(bt) if dout is None else dout.cpu()).to(F64)
    o_in = bt.val("o") if o is None else o.cpu().to(F64)
    lse_in = bt.val("lse") if lse is None else lse.cpu().to(F64)
    r = bwd_math(c, q, k, v, o_in, do, lse_in, bt.scale)
    gs = grad_scales(r, q, k, v, o_in, do, bt.scale)
    close_bf16(got("dv"), r["dv"], gs["dv"], "attn_dv", what + " dV")
    close_bf16(got("dq"), r["dq"], gs["dq"], "attn_dq", what + " dQ", gs["dq32"])
    close_bf16(got("dk"), r["dk"], gs["dk"], "attn_dk", what + " dK", gs["dk32"])
    if "delta" not in bt.untouched:
        R.close_f32(got("delta"), r["delta"], "attn_delta", what + " delta", scale=gs["delta"])
    # rows of dK / dV at or past kv_len: exactly +-0
    klim, _, lf = window(c)
    for b in range(c.B):
        if lf[b] and klim[b] < c.Lk:
            for n in ("dk", "dv"):
                if bool((got(n)[b, klim[b]:].to(F64) != 0).any()):
                    _fail(what, f"{n} rows at or past kv_len of batch element {b} not zero")
    if bt.exact_rows is not None and o is None:
        rows = bt.exact_rows
        _same_values(got("dv")[rows], exact_expect(bt, do)["dv"][rows], what + " dV (scatter-add of dO)")
        for n in ("dq", "dk"):
            _same_values(got(n)[rows], torch.zeros_like(got(n)[rows]), what + f" {n} (exactly 0)")


def rejected(bt, after, **given):
    try:
        check(bt, after, **given)
    except Mismatch:
        return True
    return False


# --------------------------------------------------------------------------- float32 evaluation
def attn_f32(bt: Built, mutant=None):
    """The operation in plain float32 PyTorch with the design's bf16 operand
    and store roundings on bt's buffers, as a launch would leave them: pool
    name -> flat tensor."""
    assert mutant is None or mutant in MUTANTS
    c = bt.case
    after = {p: f.t.clone() for p, f in bt.pools.items()}
    dst = lambda n: bt.view(n, after)  # noqa: E731

    def store(n, val):
        """Write a [B, L, ...] result; the output-side mutants act here."""
        t = dst(n)
        L = t.shape[1] if n != "probs" and t.dim() == 4 else None
        val = val.to(t.dtype)
        if mutant == "tail_rows_unwritten" and n in ("o", "dq", "probs", "lse", "delta") and c.Lq % 16:
            keep = 16 * (c.Lq // 16)
            if n in ("o", "dq"):
                t[:, :keep] = val[:, :keep]
            elif n == "probs":
                t[:, :, :keep] = val[:, :, :keep]
            else:
                t[..., :keep] = val[..., :keep]
            return
        if mutant == "dkdv_tail_unwritten" and n in ("dk", "dv") and c.kv is not None:
            klim, _, lf = window(c)
            for b in range(c.B):
                e = klim[b] if lf[b] else c.Lk
                t[b, :e] = val[b, :e]
            return
        t.copy_(val)
        if mutant == "row_at_Lq" and n in ("o", "dq", "probs"):
            pool = after[bt.where[n]]
            shape, strides, off = bt.pools[bt.where[n]].views[n]
            if n == "probs":  # the row after the last one of the last (b, h)
                pool[off + math.prod(shape): off + math.prod(shape) + c.Lk] = 0.25
            else:
                b = c.B - 1
                start = off + b * strides[0] + L * strides[1]
                pool[start:start + c.hd] = val[b, L - 1, 0]

    if c.op == "probs":
        p, _, _ = probs_math(c, bt.view("q"), bt.view("k"), bt.scale, F32, mutant)
        store("probs", p)
        return after
    rnd = lambda x: x.to(BF16)  # noqa: E731
    if c.op in ("qkv_self", "qkv_cross"):
        proj = rnd(bt.view("x").to(F32) @ bt.view("w").to(F32).T + bt.view("bias"))
        dst("qkv").copy_(proj.to(BF16))
        proj = proj.to(F32)
        if c.op == "qkv_self":
            p5 = proj.view(c.B, c.Lq, 3, c.H, c.hd)
            q, k, v = p5[:, :, 0], p5[:, :, 1], p5[:, :, 2]
        else:
            q, k, v = proj.view(c.B, c.Lq, c.H, c.hd), bt.view("k"), bt.view("v")
    else:
        q, k, v = bt.view("q"), bt.view("k"), bt.view("v")
    if c.op in FWD_OPS:
        f = fwd_math(c, q, k, v, bt.scale, F32, mutant, True)
        store("o", rnd(f["O"]))
        store("lse", f["lse"])
        return after
    r = bwd_math(c, q, k, v, bt.view("o"), dout_f32(bt), bt.view("lse"), bt.scale, F32, mutant, True)
    for n in ("dq", "dk", "dv"):
        store(n, rnd(r[n]))
    if "delta" not in bt.untouched:
        store("delta", r["delta"])
    return after


def measure_e32(bt: Built, worst: dict):
    """Fold this case's ratios of the plain float32 evaluation (no bf16
    rounding) against the float64 reference into `worst` (the unit of E32)."""
    c = bt.case

    def fold(key, got, ref, scale, rel):
        err = (got.to(F64) - ref).abs()
        den = (ref.abs() + scale) if rel else scale
        ratio = torch.where(err > 0, err / den.clamp_min(1e-300), torch.zeros_like(err))
        worst[key] = max(worst.get(key, 0.0), float(ratio.max()))

    if c.op == "probs":
        ref, s, att = probs_math(c, bt.val("q"), bt.val("k"), bt.scale)
        smax = s.abs().masked_fill(~att, 0.0).max(-1, keepdim=True).values
        fold("attn_probs", probs_math(c, bt.view("q"), bt.view("k"), bt.scale, F32)[0], ref, ref * smax, True)
        return
    if c.op in ("qkv_self", "qkv_cross"):
        # (the projection is ref_gemm's; the attention starts from its bf16 output)
        proj = (bt.view("x").to(F32) @ bt.view("w").to(F32).T + bt.view("bias")).to(BF16).to(F64)
        if c.op == "qkv_self":
            p5 = proj.view(c.B, c.Lq, 3, c.H, c.hd)
            q, k, v = p5[:, :, 0], p5[:, :, 1], p5[:, :, 2]
        else:
            q, k, v = proj.view(c.B, c.Lq, c.H, c.hd), bt.val("k"), bt.val("v")
    else:
        q, k, v = bt.val("q"), bt.val("k"), bt.val("v")
    if c.op in FWD_OPS:
        f = fwd_math(c, q, k, v, bt.scale)
        g = fwd_math(c, q, k, v, bt.scale, F32)
        fold("attn_o", g["O"], f["O"], _o_scale(f["P"], v), False)
        zmax = f["z"].abs().masked_fill(~f["att"], 0.0).max(-1).values
        fold("attn_lse", g["lse"], f["lse"], zmax, True)
        return
    do = dout_f32(bt).to(F64)
    o_in, lse_in = bt.val("o"), bt.val("lse")
    r = bwd_math(c, q, k, v, o_in, do, lse_in, bt.scale)
    g = bwd_math(c, q, k, v, o_in, do, lse_in, bt.scale, F32)
    gs = grad_scales(r, q, k, v, o_in, do, bt.scale)
    fold("attn_dv", g["dv"], r["dv"], gs["dv"], False)
    fold("attn_dq", g["dq"], r["dq"], gs["dq32"], False)
    fold("attn_dk", g["dk"], r["dk"], gs["dk32"], False)
    if "delta" not in bt.untouched:
        fold("attn_delta", g["delta"], r["delta"], gs["delta"], True)
