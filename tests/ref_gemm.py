"""Float64 / exact references, comparators, case tables and mutants for the
bf16 MFMA GEMM family (csrc/kernels/gemm_impl.h, gemm_pipe.h,
csrc/include/tdg_gemm.h, gemm_{nn,nt,tn,tt}.hip), the ragged 256x256 kernel's
fused bias sums and the column sums (gemm.hip). No GPU needed.

Two input families come from one builder (`build`):

  exact      ternary operands in {-1, 0, 1} (thinned for long K), small-integer
             bias and C_old, alpha in {1, 0.5}. The builder asserts that every
             expected output and every intermediate t = epi(alpha * acc + bias)
             survives a round trip through the output dtype, so a correct
             kernel's result is BITWISE the reference on every arm and under
             any summation order.
  toleranced bf16-rounded randn operands, compared through close_out below.

Every buffer is built with one row before and one row after it. Operand
padding (the K tail of a K-contiguous operand, the columns [mn, ld) of an
MN-contiguous one, the rows around it, what follows the bias) is NaN: a K
tail that is not zeroed in both LDS images shows as 0 * NaN. C's guards
(columns [N, ldc), the rows around it, and with beta == 0 the interior too)
hold a quiet NaN with a recognisable payload: after a launch the guards must
be bitwise untouched and the interior must hold no sentinel, which also
catches a tile the XCD raster never visited.

The kernels' rounding contract (what close_out's bf16 budget states), with
h(x) = half the spacing of bf16 at |x| (2^-9 |x| <= h(x) <= 2^-8 |x|; a
budget of 2^-9 |x| itself is below what round-to-nearest needs wherever |x| is
not a power of two, so it is h that is used):
  * f32 out: no rounding beyond the f32 accumulation.
  * bf16 out, beta == 0: one rounding, h(ref).
  * bf16 out, beta != 0, tile kernels: EpiLds rounds t to bf16 into its LDS
    image, adds beta * C_old and rounds again: h(ref) + h(t), a 1-ulp
    budget. A third rounding does not fit it.
  * bf16 out, split-K reduce: splitk_reduce_kernel rounds once, h(ref).

`gemm_f32` is the plain float32 PyTorch evaluation of the same operation on
the built buffers; with `mutant=...` it is wrong in one line.
tests/test_gemm_refs_cpu.py shows that `check` accepts the former and rejects
every mutant, so tests/test_gpu_gemm.py cannot pass vacuously.
`expected_arm` mirrors launch_tiles' choice of kernel; it exists only so the
GPU tests can assert that the arm a case is named after is the arm that ran.
"""
from __future__ import annotations

import functools
import math
from collections import namedtuple
from dataclasses import dataclass

import torch

import ref_tail as R
from ref_tail import BF16, F32, F64, MARGIN, Mismatch, exact, tol  # noqa: F401

# --------------------------------------------------------------------------- tolerances
# Same form and discipline as ref_tail.E32: E32 is the worst ratio of the
# float32 PyTorch evaluation against the float64 reference over this file's
# toleranced cases (test_gemm_refs_cpu.py::test_e32_table_is_measured), the
# tolerance is MARGIN = 8 times it, `kernel` is the worst ratio of the HIP
# kernels on the MI355X in the same unit.
#
#   entry          E32       kernel     what
E32 = {
    "gemm_acc":   1.2e-7,  # 1.1e-7   |got - ref| / (|ref| + |alpha| S + |beta C_old|), S = |A| @ |B|;
                           #          bf16 out: the part of the error beyond the rounding budget above
    "gemm_bsum":  1.6e-8,  # 1.5e-8   ragged fused bias sums; scale sum_t |dy| + |beta old|
    "colsum":     5.9e-8,  # 3.0e-8   colsum / colsum_grouped; scale sum_m |x| + |beta old|
}
R.register(E32)


def half_ulp_bf16(x):
    """Half the spacing of bf16 (8 significand bits) at |x|: the bound of one
    round-to-nearest. 0 at 0."""
    m, e = torch.frexp(x.abs().to(F64))  # |x| = m 2^e, m in [0.5, 1): spacing 2^(e - 8)
    return torch.where(x != 0, torch.ldexp(torch.ones_like(m), e - 9), torch.zeros_like(m))


EPI_NONE, EPI_BIAS, EPI_BIAS_RELU, EPI_DRELU, EPI_BIAS_RELU_BITS, EPI_DRELU_BITS = range(6)
EPI_NAMES = ("none", "bias", "bias_relu", "drelu", "bias_relu_bits", "drelu_bits")
# layout -> (a_kc, b_kc)
LAYOUTS = {"nt": (True, True), "nn": (True, False), "tn": (False, False), "tt": (False, True)}
BK, PK = 64, 32
# launch_tiles' tables: cfg -> (BM, BN, STAGES) / (BM, BN, NS, wave tile columns)
LOCK = {0: (128, 128, 2), 1: (128, 64, 3), 2: (64, 128, 3), 3: (64, 64, 4), 4: (128, 128, 3),
        5: (256, 128, 2), 6: (128, 256, 2), 7: (64, 128, 2), 8: (64, 64, 2), 9: (256, 128, 3),
        10: (128, 256, 3), 11: (128, 128, 4), 13: (128, 128, 4), 14: (128, 128, 5)}
PIPE = {20: (256, 256, 4, 64), 21: (256, 128, 6, 32), 22: (128, 256, 6, 64), 23: (256, 256, 4, 128),
        24: (256, 256, 5, 128), 25: (256, 128, 6, 64), 26: (128, 256, 6, 128)}
R256 = 12
ALL_CFGS = tuple(sorted(LOCK)) + (R256,) + tuple(sorted(PIPE))
MAXG = 32

Arm = namedtuple("Arm", "family bm bn depth splits")
FAMILY_CODE = {0: "lock", 1: "r256", 2: "pipe"}  # tdg_gemm_last_plan's family word


def epis_of(layout, cfg=0):
    """(epi, out_f32) pairs dispatch_epi instantiates for the layout (the
    bitmap epilogues: no one-wave-per-SIMD pipelined tiles)."""
    a_kc, b_kc = LAYOUTS[layout]
    e = [(EPI_NONE, False), (EPI_NONE, True), (EPI_BIAS, False), (EPI_BIAS, True),
         (EPI_BIAS_RELU, False), (EPI_DRELU, False)]
    if cfg <= 22:
        if a_kc and b_kc:
            e.append((EPI_BIAS_RELU_BITS, False))
        if a_kc:
            e.append((EPI_DRELU_BITS, False))
    return e


def has_256(layout, epi, f32):
    a_kc, b_kc = LAYOUTS[layout]
    if a_kc and b_kc:
        return (not f32) or epi == EPI_NONE
    if a_kc and not b_kc:
        return (not f32) and epi in (EPI_NONE, EPI_DRELU, EPI_DRELU_BITS)
    if not a_kc and not b_kc:
        return epi == EPI_NONE
    return False


def split_count(K, splits):
    """launch_cfg's effective split-K count."""
    if splits <= 1:
        return 1
    kps = -(-(-(-K // splits)) // BK) * BK
    return -(-K // kps)


def expected_arm(cfg, layout, epi, f32, K, splits=1, grouped=False):
    """The kernel launch_tiles picks: family, tile, depth, effective splits."""
    if 20 <= cfg <= 26:
        if not grouped and splits <= 1:
            bm, bn, ns, wtn = PIPE[cfg]
            if not (epi >= EPI_BIAS_RELU_BITS and wtn > 64) and K % PK == 0:
                return Arm("pipe", bm, bn, ns, 1)
        cfg = 13
    if cfg == R256:
        if splits <= 1 and has_256(layout, epi, f32) and K % BK == 0:
            return Arm("r256", 256, 256, 2, 1)
        cfg = 13
    bm, bn, st = LOCK.get(cfg, LOCK[8])
    return Arm("lock", bm, bn, st, 1 if grouped else split_count(K, splits))


def plan_arm(plan):
    """tdg_gemm_last_plan's five words as an Arm."""
    return Arm(FAMILY_CODE.get(int(plan[0]), "?"), *(int(x) for x in plan[1:5]))


def tile_of(cfg):
    if cfg == R256:
        return 256, 256
    return (LOCK.get(cfg) or PIPE[cfg])[:2]


def nk_class(family, depth, K):
    """Which prologue / steady / drain path of the main loop K takes."""
    if family == "lock":
        nk = -(-K // BK)
        return f"nk{'<' if nk < depth else ('=' if nk == depth else '>')}depth" + \
               (f":{nk}" if nk <= depth + 2 else ":long") + (":tail" if K % BK else "")
    if family == "r256":
        nk = K // BK
        return f"nk{min(nk, 4)}"
    nk = K // PK
    return f"nk{nk}" if nk <= depth + 3 else "long"


# --------------------------------------------------------------------------- case tables
def mn_pairs(bm, bn):
    return [(1, 1), (bm - 1, bn + 1), (bm, bn), (2 * bm + 17, 2 * bn + 24), (3 * bm, 5 * bn)]


def k_list(cfg):
    """Exact-family K values of a config (what its own arm needs; K = 40 and
    the K tails make the pipelined / 256 configs fall back on purpose)."""
    if cfg == R256:
        return [64, 128, 192, 256, 320, 72]
    if cfg in PIPE:
        n = PIPE[cfg][2]
        return [PK * j for j in range(1, n + 4)] + [40]
    s = LOCK[cfg][2]
    return sorted({BK * j for j in range(1, s + 3)} | {BK * j + 8 for j in range(0, s + 2)} |
                  {BK * (s + 1) + 36, 20})


TOL_KS = (72, 1000, 4096)
SPLITK = ((512, 8), (136, 3), (200, 4), (64, 8))
LDC_MODES = ("n", "pad", "odd", "unal")
LD_MODES = ("tight", "pad")
AB = ((1.0, 0.0), (0.5, 0.0), (1.0, 1.0), (0.5, 1.0))


@dataclass(frozen=True)
class Case:
    family: str      # "exact" | "tol"
    cfg: int
    layout: str
    M: int
    N: int
    K: int
    epi: int
    f32: bool
    alpha: float
    beta: float
    ld: str          # operand leading dimensions: "tight" (round8) | "pad" (+8)
    ldc: str         # "n" | "pad" (round8(N) + 8) | "odd" (N + 3) | "unal" (N, one element off 16 bytes)
    splits: int = 1
    grouped: bool = False
    seed: int = 0

    @property
    def arm(self):
        return expected_arm(self.cfg, self.layout, self.epi, self.f32, self.K, self.splits, self.grouped)

    def what(self):
        return (f"{self.family} cfg{self.cfg} {self.layout} {self.M}x{self.N}x{self.K} {EPI_NAMES[self.epi]} "
                f"{'f32' if self.f32 else 'bf16'} alpha={self.alpha} beta={self.beta} ld={self.ld} "
                f"ldc={self.ldc} splits={self.splits}")


def _mk(family, cfg, layout, M, N, K, epi, f32, alpha, beta, ld, ldc, **kw):
    if epi >= EPI_BIAS_RELU_BITS:
        # the launcher takes N % 8 == 0, ldc % 8 == 0 and an aligned C only
        N = -(-N // 8) * 8
        if ldc in ("odd", "unal"):
            ldc = "pad"
        if epi == EPI_BIAS_RELU_BITS:
            beta = 0.0  # bits = (stored bf16 > 0) is a statement about the ReLU output itself
    return Case(family, cfg, layout, M, N, K, epi, f32, alpha, beta, ld, ldc, **kw)


def _walk(family, cfg, layout, points, per_point, abs_):
    """`per_point` cases per (M, N, K) point, walking epilogue x dtype x
    (alpha, beta) in order and the ld / ldc variants at other strides, so
    every factor meets every other over a config's table."""
    combos = [(e, f, a, b) for (e, f) in epis_of(layout, cfg) for (a, b) in abs_]
    out, k = [], 0
    for (M, N, K) in points:
        for _ in range(per_point):
            e, f, a, b = combos[k % len(combos)]
            turn = k // len(combos)
            ldc = LDC_MODES[(k + turn) % 4]
            ld = LD_MODES[(k // 4 + turn) % 2]
            out.append(_mk(family, cfg, layout, M, N, K, e, f, a, b, ld, ldc))
            k += 1
    return out


@functools.lru_cache(maxsize=None)
def exact_cases(cfg, layout):
    bm, bn = tile_of(cfg)
    pts = [(M, N, K) for K in k_list(cfg) for (M, N) in mn_pairs(bm, bn)]
    return tuple(_walk("exact", cfg, layout, pts, 4, AB))


@functools.lru_cache(maxsize=None)
def tol_cases(cfg, layout):
    bm, bn = tile_of(cfg)
    pts = [(M, N, K) for K in TOL_KS for (M, N) in ((bm - 1, bn + 1), (2 * bm + 17, 2 * bn + 24))]
    return tuple(_walk("tol", cfg, layout, pts, 6, ((1.0, 0.0), (0.5, 1.0))))


SPLIT_CFGS = (0, 3, 13, 12, 20)  # 12 / 20: split-K falls back to cfg 13


@functools.lru_cache(maxsize=None)
def splitk_cases(family):
    """Every epilogue splitk_reduce_kernel has, both output dtypes, through
    the binding; cfg 12 / 20 fall back to the lock-step cfg 13."""
    out, k = [], 0
    for (K, s) in SPLITK:
        for cfg in SPLIT_CFGS:
            bm, bn = tile_of(13 if cfg in (12, 20) else cfg)
            for layout in LAYOUTS:
                for (e, f) in epis_of(layout, 99):
                    a, b = AB[k % 4]
                    M, N = mn_pairs(bm, bn)[1 + k % 3]
                    out.append(_mk(family, cfg, layout, M, N, K, e, f, a, b, LD_MODES[k % 2],
                                   LDC_MODES[(k // 2) % 4], splits=s))
                    k += 1
    if family == "tol":
        out = [c for i, c in enumerate(out) if i % 5 == 0]
    return tuple(out)


GROUP_GS = (1, 2, 32)
GROUP_CFGS = (0, 7, 12, 20)


@functools.lru_cache(maxsize=None)
def grouped_cases(layout):
    """(Case of problem 0, G): tdg_gemm_grouped, plain epilogue."""
    out, k = [], 0
    for cfg in GROUP_CFGS:
        bm, bn = tile_of(cfg)
        for G in GROUP_GS:
            for K in (64, 200, 320):
                for f in (False, True):
                    a, b = AB[k % 4]
                    M, N = ((bm - 1, bn + 1), (2 * bm + 17, 2 * bn + 24))[k % 2] if G < 32 else (bm - 1, bn + 1)
                    out.append((_mk("exact", cfg, layout, M, N, K, EPI_NONE, f, a, b, LD_MODES[k % 2],
                                    ("n", "pad", "odd")[k % 3], grouped=True), G))
                    k += 1
    return tuple(out)


# --------------------------------------------------------------------------- inputs
SENT_BF16, SENT_F32 = 0x7FA5, 0x7FC0A5A5  # quiet NaNs with a payload
BITS_FILL = 0xA5                          # what a bitmap buffer holds before the producer runs


def _gen(idx, c):
    return torch.Generator().manual_seed((idx * 1000003 + c.M * 7919 + c.N * 104729 + c.K * 1299709 +
                                          c.seed * 15485863) % (2 ** 31 - 1))


def sentinel(n, f32):
    if f32:
        return torch.full((n,), SENT_F32, dtype=torch.int32).view(F32)
    return torch.full((n,), SENT_BF16, dtype=torch.int16).view(BF16)


def round8(v):
    return -(-v // 8) * 8


@functools.lru_cache(maxsize=64)
def _operands(family, M, N, K, seed):
    """a [M, K], b [N, K] (bf16 values as float64), acc = a @ b^T, S = |a| @ |b|^T."""
    c = Case(family, 0, "nt", M, N, K, 0, False, 1.0, 0.0, "tight", "n", seed=seed)
    if family == "exact":
        p = min(1.0, math.sqrt(64.0 / K))  # thinned: about 64 nonzero products at most
        def tern(g, r):
            v = torch.randint(-1, 2, (r, K), generator=g).to(F64)
            return v if p >= 1.0 else v * (torch.rand(r, K, generator=g) < p)
        a, b = tern(_gen(1, c), M), tern(_gen(2, c), N)
    else:
        a = torch.randn(M, K, generator=_gen(1, c)).to(BF16).to(F64)
        b = torch.randn(N, K, generator=_gen(2, c)).to(BF16).to(F64)
    return a, b, a @ b.T, a.abs() @ b.abs().T


AUX_SPECIALS_BITS = (0x0000, 0x8000, 0x0001, 0x8001, 0x7F80, 0xFF80, 0x7FC0)  # +-0, +-min subnormal, +-inf, NaN


def _aux_values(c):
    """bf16 ReLU input of EPI_DRELU: ordinary values with +0, -0, the
    smallest subnormals, +-inf and NaN among them. The mask is x > 0."""
    g = _gen(5, c)
    x = torch.randn(c.M, c.N, generator=g).to(BF16)
    xi = x.view(torch.int16).clone()
    pick = torch.randint(0, 3 * len(AUX_SPECIALS_BITS), (c.M, c.N), generator=g)
    for i, bits in enumerate(AUX_SPECIALS_BITS):
        xi[pick == i] = bits - 0x10000 if bits >= 0x8000 else bits
    return xi.view(BF16)


Ref = namedtuple("Ref", "pre t S bits")


def ref_gemm(acc, S, alpha, beta, cold, bias, mask, epi):
    """Float64 reference from the accumulation acc = A @ B^T of exactly the
    values the kernel gets: (pre-rounding result, t = epi(alpha * acc + bias)
    before beta * C_old, S, expected bitmap or None)."""
    v = alpha * acc
    if epi in (EPI_BIAS, EPI_BIAS_RELU, EPI_BIAS_RELU_BITS):
        v = v + bias[None, :]
    if epi in (EPI_BIAS_RELU, EPI_BIAS_RELU_BITS):
        v = v.clamp_min(0.0)
    if epi in (EPI_DRELU, EPI_DRELU_BITS):
        v = torch.where(mask, v, torch.zeros_like(v))
    t = v + 0.0  # (-0 -> +0: the kernels' accumulators start from +0)
    pre = t + (beta * cold if beta != 0 else 0.0)
    bits = None
    if epi == EPI_BIAS_RELU_BITS:
        bits = pack_bits(t.to(F32).to(BF16) > 0)  # (beta == 0: t rounded is the stored bf16)
    return Ref(pre, t, S, bits)


def pack_bits(m, big=False):
    """bool [M, N] (N % 8 == 0) -> uint8 [M, N / 8], bit e of byte c = column 8c + e."""
    M, N = m.shape
    w = torch.tensor([1 << (7 - e if big else e) for e in range(8)], dtype=torch.int32)
    return (m.view(M, N // 8, 8).to(torch.int32) * w).sum(-1).to(torch.uint8)


@dataclass
class Built:
    case: Case
    A: torch.Tensor      # flat bf16 buffers; the operand starts at *_off
    a_off: int
    lda: int
    B: torch.Tensor
    b_off: int
    ldb: int
    C: torch.Tensor      # flat, out dtype
    c_off: int
    ldc: int
    bias: torch.Tensor   # f32 [N] + NaN tail, or None
    aux: torch.Tensor    # flat bf16 or None
    aux_off: int
    ldaux: int
    bits: torch.Tensor   # flat uint8 or None
    bits_off: int
    ldbits: int
    a: torch.Tensor      # values, float64
    b: torch.Tensor
    cold: torch.Tensor
    biasv: torch.Tensor
    mask: torch.Tensor
    ref: Ref

    def dev(self, name, device):
        """The tensor the binding takes: the flat buffer from its offset on."""
        t = getattr(self, name)
        if t is None:
            return None, None
        d = t.to(device)
        off = {"A": self.a_off, "B": self.b_off, "C": self.c_off, "aux": self.aux_off,
               "bits": self.bits_off, "bias": 0}[name]
        return d, d[off:]


def _operand(vals, kc, ld_mode):
    """[mn, K] values -> flat NaN-padded buffer in the operand's layout."""
    mn, K = vals.shape
    rows, cols = (mn, K) if kc else (K, mn)
    ld = round8(cols) + (8 if ld_mode == "pad" else 0)
    buf = torch.full(((rows + 2) * ld,), float("nan"), dtype=BF16)
    v = buf[ld:(rows + 1) * ld].view(rows, ld)
    v[:, :cols] = (vals if kc else vals.T).to(BF16)
    return buf, ld, ld


def c_geometry(c):
    q = 4 if c.f32 else 8
    ldc = {"n": c.N, "unal": c.N, "pad": round8(c.N) + 8, "odd": c.N + 3}[c.ldc]
    off = -(-ldc // q) * q + (1 if c.ldc == "unal" else 0)
    return ldc, off, off + c.M * ldc + ldc + q


def interior(flat, off, M, N, ld):
    return flat.as_strided((M, N), (ld, 1), off)


def build(c: Case) -> Built:
    a_kc, b_kc = LAYOUTS[c.layout]
    a, b, acc, S = _operands(c.family, c.M, c.N, c.K, c.seed)
    A, a_off, lda = _operand(a, a_kc, c.ld)
    Bm, b_off, ldb = _operand(b, b_kc, c.ld)
    odt = F32 if c.f32 else BF16
    exactf = c.family == "exact"
    # bias, C_old
    biasv = bias = None
    if c.epi in (EPI_BIAS, EPI_BIAS_RELU, EPI_BIAS_RELU_BITS):
        g = _gen(3, c)
        biasv = (torch.randint(-4, 5, (c.N,), generator=g).to(F64) if exactf
                 else torch.randn(c.N, generator=g).to(F32).to(F64))
        bias = torch.cat([biasv.to(F32), torch.full((5,), float("nan"), dtype=F32)])
    else:
        biasv = torch.zeros(c.N, dtype=F64)
    g = _gen(4, c)
    cold = (torch.randint(-8, 9, (c.M, c.N), generator=g).to(F64) if exactf
            else torch.randn(c.M, c.N, generator=g).to(odt).to(F64))
    ldc, c_off, c_len = c_geometry(c)
    C = sentinel(c_len, c.f32)
    if c.beta != 0:
        interior(C, c_off, c.M, c.N, ldc).copy_(cold.to(odt))
    # ReLU mask: bf16 aux (same stride and misalignment as C) or bitmap
    aux = bits = mask = None
    aux_off = ldaux = bits_off = ldbits = 0
    if c.epi == EPI_DRELU:
        x = _aux_values(c)
        mask = x.to(F64) > 0
        ldaux = ldc
        aux_off = -(-ldaux // 8) * 8 + (1 if c.ldc == "unal" else 0)
        aux = torch.full((aux_off + c.M * ldaux + ldaux + 8,), float("nan"), dtype=BF16)
        interior(aux, aux_off, c.M, c.N, ldaux).copy_(x)
    if c.epi >= EPI_BIAS_RELU_BITS:
        ldbits = c.N // 8 + (3 if c.ld == "pad" else 0)
        bits_off = -(-ldbits // 16) * 16
        n = bits_off + c.M * ldbits + ldbits + 16
        if c.epi == EPI_DRELU_BITS:
            mask = torch.rand(c.M, c.N, generator=_gen(6, c)) < 0.5
            bits = torch.full((n,), 0xFF, dtype=torch.uint8)  # padding bits set: they must not unmask
            interior(bits, bits_off, c.M, c.N // 8, ldbits).copy_(pack_bits(mask))
        else:
            bits = torch.full((n,), BITS_FILL, dtype=torch.uint8)
    ref = ref_gemm(acc, S, c.alpha, c.beta, cold, biasv, mask, c.epi)
    if exactf:
        for name, v in (("t", ref.t), ("out", ref.pre)):
            assert bool((v.to(odt).to(F64) == v).all()), f"{c.what()}: {name} not representable in {odt}"
    return Built(c, A, a_off, lda, Bm, b_off, ldb, C, c_off, ldc, bias, aux, aux_off, ldaux, bits,
                 bits_off, ldbits, a, b, cold, biasv, mask, ref)


def check_pristine(bt: Built):
    """Guards and poison are in place before any kernel runs."""
    c = bt.case
    a_kc, b_kc = LAYOUTS[c.layout]
    for flat, off, ld, kc, mn in ((bt.A, bt.a_off, bt.lda, a_kc, c.M), (bt.B, bt.b_off, bt.ldb, b_kc, c.N)):
        rows, cols = (mn, c.K) if kc else (c.K, mn)
        v = flat[off:off + rows * ld].view(rows, ld)
        assert off == ld and flat.numel() == (rows + 2) * ld
        assert bool(flat[:off].isnan().all()) and bool(flat[off + rows * ld:].isnan().all())
        assert bool(v[:, cols:].isnan().all()) and not bool(v[:, :cols].isnan().any())
    if bt.bias is not None:
        assert bool(bt.bias[c.N:].isnan().all()) and bt.bias.numel() > c.N
    blank = sentinel(bt.C.numel(), c.f32)
    keep = blank.clone()
    if c.beta != 0:
        interior(keep, bt.c_off, c.M, c.N, bt.ldc).copy_(bt.cold.to(keep.dtype))
    exact(bt.C, keep, "C before the launch")
    q = 4 if c.f32 else 8
    assert (bt.c_off % q == 1) == (c.ldc == "unal") and bt.c_off >= bt.ldc
    if bt.aux is not None:
        assert (bt.aux_off % 8 == 1) == (c.ldc == "unal")
        m = torch.ones(bt.aux.numel(), dtype=torch.bool)
        interior(m, bt.aux_off, c.M, c.N, bt.ldaux).fill_(False)
        assert bool(bt.aux[m].isnan().all())
    if bt.bits is not None:
        m = torch.ones(bt.bits.numel(), dtype=torch.bool)
        interior(m, bt.bits_off, c.M, c.N // 8, bt.ldbits).fill_(False)
        assert bool((bt.bits[m] == (0xFF if c.epi == EPI_DRELU_BITS else BITS_FILL)).all())


# --------------------------------------------------------------------------- comparators
def _fail(what, msg):
    raise Mismatch(f"{what}: {msg}")


def _as_int(t):
    return t.view({2: torch.int16, 4: torch.int32, 1: torch.uint8}[t.element_size()])


def close_acc(got, ref: Ref, alpha, beta, cold, what, key="gemm_acc"):
    """f32 out: |got - ref| <= tol * (|ref| + |alpha| S + |beta C_old|)."""
    return close_out(got, ref, alpha, beta, cold, what, rounding=None, key=key)


def close_out(got, ref: Ref, alpha, beta, cold, what, rounding, key="gemm_acc"):
    """rounding None: f32 out. "tile": bf16 out of a tile kernel (half an ulp
    of ref, and of t too when beta != 0: two roundings). "split": bf16 out
    of the split-K reduce (one rounding)."""
    g = got.to(F64)
    if not bool(torch.isfinite(g).all()):
        _fail(what, "non-finite values")
    den = ref.pre.abs() + abs(alpha) * ref.S + (beta * cold).abs()
    err = (g - ref.pre).abs()
    if rounding is not None:
        budget = half_ulp_bf16(ref.pre) + (half_ulp_bf16(ref.t) if (beta != 0 and rounding == "tile") else 0.0)
        err = (err - budget).clamp_min(0)
    ratio = torch.where(err > 0, err / den.clamp_min(1e-300), torch.zeros_like(err))
    worst = float(ratio.max())
    R._note(key, worst)
    if worst > tol(key):
        i = int(ratio.argmax())
        _fail(what, f"[{key}] ratio {worst:.3e} > {tol(key):.3e} at {divmod(i, g.shape[1])}: got "
                    f"{g.flatten()[i].item()!r} ref {ref.pre.flatten()[i].item()!r}")
    return worst


def check(bt: Built, C_after, bits_after=None, rounding="tile"):
    """Everything a launch on bt's buffers must satisfy: guards bitwise
    untouched, no sentinel left inside, the values (bitwise for the exact
    family), the bitmap and its padding."""
    c = bt.case
    what = c.what()
    C_after = C_after.cpu()
    odt = F32 if c.f32 else BF16
    if C_after.dtype != odt or C_after.numel() != bt.C.numel():
        _fail(what, "C buffer changed type or size")
    inside = torch.zeros(bt.C.numel(), dtype=torch.bool)
    interior(inside, bt.c_off, c.M, c.N, bt.ldc).fill_(True)
    gi, bi = _as_int(C_after), _as_int(bt.C)
    if not bool((gi[~inside] == bi[~inside]).all()):
        i = int(((gi != bi) & ~inside).nonzero()[0])
        r, col = divmod(i - bt.c_off, bt.ldc)
        _fail(what, f"guard overwritten at row {r} column {col} (M={c.M} N={c.N} ldc={bt.ldc})")
    got = interior(C_after, bt.c_off, c.M, c.N, bt.ldc)
    sent = SENT_F32 if c.f32 else SENT_BF16
    left = interior(gi, bt.c_off, c.M, c.N, bt.ldc) == sent
    if bool(left.any()):
        i = int(left.flatten().nonzero()[0])
        _fail(what, f"{int(left.sum())} interior elements never written, first at {divmod(i, c.N)}")
    if c.family == "exact":
        exact(got.contiguous(), bt.ref.pre.to(odt), what)
    else:
        close_out(got, bt.ref, c.alpha, c.beta, bt.cold, what, None if c.f32 else rounding)
    if bt.bits is not None:
        if bits_after is None:
            _fail(what, "no bitmap")
        want = bt.bits.clone()
        if c.epi == EPI_BIAS_RELU_BITS:
            interior(want, bt.bits_off, c.M, c.N // 8, bt.ldbits).copy_(bt.ref.bits)
        exact(bits_after.cpu(), want, what + " bitmap and its padding")


# --------------------------------------------------------------------------- float32 evaluation
MUTANTS = ("last_k_dropped", "ktail_kept", "stale_tile", "row_clamped", "bias_shift", "alpha_after_bias",
           "beta_ignored", "beta_twice", "relu_ge", "mask_row_off", "subtile_transposed", "trunc_bf16",
           "third_rounding", "guard_write", "unwritten_tile", "bits_big_endian")


def _trunc_bf16(x):
    return (x.to(F32).contiguous().view(torch.int32) & -65536).view(F32)


def gemm_f32(bt: Built, mutant=None, rounding="tile"):
    """The operation in plain float32 PyTorch on bt's buffers, as a launch
    would leave them: (C flat buffer, bitmap flat buffer or None)."""
    c = bt.case
    M, N, K = c.M, c.N, c.K
    a, b = bt.a.to(F32), bt.b.to(F32)
    if mutant == "last_k_dropped":
        a = a.clone(); a[:, K - 1] = 0
    if mutant == "stale_tile" and K > BK:
        a, b = a.clone(), b.clone()
        w = min(BK, K - BK)
        a[:, BK:BK + w] = a[:, :w]; b[:, BK:BK + w] = b[:, :w]
    acc = a @ b.T
    if mutant == "ktail_kept" and K % 8:
        acc = acc + 1.0  # one padding element of each operand taken as 1.0
    if mutant == "row_clamped" and M >= 2:
        acc[M - 1] = acc[M - 2]
    if mutant == "subtile_transposed" and M >= 16 and N >= 16:
        acc[:16, :16] = acc[:16, :16].T.clone()
    if mutant == "third_rounding":
        acc = acc.to(BF16).to(F32)
    alpha, beta = torch.tensor(c.alpha, dtype=F32), torch.tensor(c.beta, dtype=F32)
    has_bias = c.epi in (EPI_BIAS, EPI_BIAS_RELU, EPI_BIAS_RELU_BITS)
    if has_bias:
        bias = bt.bias[1:N + 1] if mutant == "bias_shift" else bt.bias[:N]
        v = alpha * (acc + bias) if mutant == "alpha_after_bias" else alpha * acc + bias
    else:
        v = alpha * acc
    if c.epi in (EPI_BIAS_RELU, EPI_BIAS_RELU_BITS):
        v = v.clamp_min(0.0)
    if c.epi in (EPI_DRELU, EPI_DRELU_BITS):
        if c.epi == EPI_DRELU:
            x = interior(bt.aux, bt.aux_off, M, N, bt.ldaux).to(F32)
            mask = (x >= 0) if mutant == "relu_ge" else (x > 0)
        else:
            mask = bt.mask
        if mutant == "mask_row_off" and M >= 2:
            mask = mask.roll(1, 0)
        v = torch.where(mask, v, torch.zeros_like(v))
    v = v + 0.0
    rnd = _trunc_bf16 if mutant == "trunc_bf16" else (lambda x: x.to(BF16).to(F32))
    bits = None
    if c.epi == EPI_BIAS_RELU_BITS:
        bits = bt.bits.clone()
        interior(bits, bt.bits_off, M, N // 8, bt.ldbits).copy_(
            pack_bits(rnd(v) > 0, big=(mutant == "bits_big_endian")))
    elif bt.bits is not None:
        bits = bt.bits.clone()
    old = interior(bt.C, bt.c_off, M, N, bt.ldc).to(F32)
    if c.beta != 0 and mutant != "beta_ignored":
        bo = (2 * beta if mutant == "beta_twice" else beta) * old
        if c.f32:
            out = v + bo
        elif rounding == "tile":
            out = rnd(rnd(v) + bo)
        else:
            out = rnd(v + bo)
    else:
        out = v if c.f32 else rnd(v)
    Cf = bt.C.clone()
    dst = interior(Cf, bt.c_off, M, N, bt.ldc)
    if mutant == "unwritten_tile":
        keep = dst[-16:, -16:].clone()
        dst.copy_(out.to(Cf.dtype))
        dst[-16:, -16:] = keep
    else:
        dst.copy_(out.to(Cf.dtype))
    if mutant == "guard_write":
        Cf[bt.c_off + N] = 1.0  # column N of row 0 (ldc == N: element (1, 0), or the row after C)
        if bt.ldc == N and M > 1:
            Cf[bt.c_off + M * bt.ldc] = 1.0
    return Cf, bits


def rejected(bt, Cf, bits, rounding="tile"):
    try:
        check(bt, Cf, bits, rounding)
    except Mismatch:
        return True
    return False


# --------------------------------------------------------------------------- ragged 256x256 launches, column sums
# wgrad problems dw[N, Kx] (+)= dy[T, N]^T @ x[T, Kx] (both operands MN-contiguous, T the shared token
# count = the GEMM's K) with optional fused bias sums db[N] (+)= sum_t dy[t, :].
RAGGED_KS = (64, 128, 192, 256, 320)
RAGGED_SHAPES = ((8, 8), (255, 257), (264, 520), (256, 256), (40, 300), (300, 40), (520, 8), (16, 272))
RAGGED_MUTANTS = ("problem_swapped", "range_off_by_one", "bias_sum_all_tn")


@dataclass
class WgradProblem:
    dy: torch.Tensor    # bf16 [T, N] view with row stride ld (NaN padding)
    x: torch.Tensor     # bf16 [T, Kx]
    dw: torch.Tensor    # f32 flat buffer with guards (sentinel / old values)
    dw_off: int
    ldw: int
    N: int
    Kx: int
    db: torch.Tensor    # f32 [N] + sentinel tail, or None
    old_w: torch.Tensor  # float64 [N, Kx]
    old_b: torch.Tensor  # float64 [N] or None
    ref_w: torch.Tensor  # float64
    S_w: torch.Tensor
    ref_b: torch.Tensor
    S_b: torch.Tensor


def _padded(vals, pad):
    """bf16 [T, n] values -> a [T, n] view of a NaN-padded buffer (row stride round8(n) + pad)."""
    T, n = vals.shape
    ld = round8(n) + pad
    buf = torch.full(((T + 2) * ld,), float("nan"), dtype=BF16)
    v = buf.as_strided((T, n), (ld, 1), ld)
    v.copy_(vals.to(BF16))
    return v


def wgrad_problem(N, Kx, T, beta, with_bias, seed, exactf=True, pad=0, ldw_pad=0):
    c = Case("exact" if exactf else "tol", 0, "tn", N, Kx, T, 0, True, 1.0, beta, "tight", "n", seed=seed)
    dyv, xv, acc, S = _operands(c.family, N, Kx, T, seed)  # [N, T], [Kx, T]
    dy, x = _padded(dyv.T, pad), _padded(xv.T, pad)
    g = _gen(4, c)
    old_w = torch.randint(-8, 9, (N, Kx), generator=g).to(F64) if exactf else torch.randn(N, Kx, generator=g).to(F32).to(F64)
    ldw = Kx + ldw_pad
    off = -(-ldw // 4) * 4
    dw = sentinel(off + N * ldw + ldw + 4, True)
    if beta != 0:
        interior(dw, off, N, Kx, ldw).copy_(old_w.to(F32))
    db = old_b = ref_b = S_b = None
    if with_bias:
        old_b = torch.randint(-8, 9, (N,), generator=g).to(F64)
        db = sentinel(N + 4, True)
        if beta != 0:
            db[:N] = old_b.to(F32)
        ref_b = dyv.sum(1) + (beta * old_b if beta != 0 else 0.0)
        S_b = dyv.abs().sum(1) + (beta * old_b).abs()
    return WgradProblem(dy, x, dw, off, ldw, N, Kx, db, old_w, old_b,
                        acc + (beta * old_w if beta != 0 else 0.0), S + (beta * old_w).abs(), ref_b, S_b)


def tiles_of(N, Kx):
    return -(-N // 256) * -(-Kx // 256)


def tile_rect(N, Kx, t):
    """Rows / columns of tile t in gemm256_kernel's enumeration, and whether it is a tn == 0 tile."""
    tm_n, tn_n = -(-N // 256), -(-Kx // 256)
    if tn_n <= tm_n:
        tn, tm = t % tn_n, t // tn_n
    else:
        tm, tn = t % tm_n, t // tm_n
    return slice(256 * tm, min(N, 256 * tm + 256)), slice(256 * tn, min(Kx, 256 * tn + 256)), tn == 0


def ragged_f32(probs, beta, ranges=None, mutant=None):
    """A ragged launch in float32 on the problems' buffers: [(dw flat, db or None)]."""
    out = []
    n = len(probs)
    for i, p in enumerate(probs):
        j = i ^ 1  # problem_swapped: neighbours of one shape class trade operands
        src = probs[j] if (mutant == "problem_swapped" and j < n and probs[j].N == p.N and
                           probs[j].Kx == p.Kx) else p
        full = src.dy.to(F32).T @ src.x.to(F32)
        bsum = src.dy.to(F32).sum(0)
        dw = p.dw.clone()
        dst = interior(dw, p.dw_off, p.N, p.Kx, p.ldw)
        db = None if p.db is None else p.db.clone()
        first, count = (0, tiles_of(p.N, p.Kx)) if ranges is None or ranges[i] is None else ranges[i]
        if mutant == "range_off_by_one" and ranges is not None and ranges[i] is not None:
            first = min(first + 1, tiles_of(p.N, p.Kx) - 1)
        for t in range(first, first + count):
            if t >= tiles_of(p.N, p.Kx):
                continue
            rs, cs, tn0 = tile_rect(p.N, p.Kx, t)
            dst[rs, cs] = full[rs, cs] + (beta * dst[rs, cs] if beta != 0 else 0.0)
            if db is not None and (tn0 or mutant == "bias_sum_all_tn"):
                db[rs] = bsum[rs] + (beta * db[rs] if beta != 0 else 0.0)
        out.append((dw, db))
    return out


def check_wgrad(p: WgradProblem, dw_after, db_after, what, exactf=True, rows=None, touched_bias=True):
    """One problem of a ragged launch (whole: rows None)."""
    dw_after = dw_after.cpu()
    inside = torch.zeros(p.dw.numel(), dtype=torch.bool)
    interior(inside, p.dw_off, p.N, p.Kx, p.ldw).fill_(True)
    gi, bi = _as_int(dw_after), _as_int(p.dw)
    if not bool((gi[~inside] == bi[~inside]).all()):
        _fail(what, "dw guard overwritten")
    got = interior(dw_after, p.dw_off, p.N, p.Kx, p.ldw)
    if bool((interior(gi, p.dw_off, p.N, p.Kx, p.ldw) == SENT_F32).any()):
        _fail(what, "dw elements never written")
    if exactf:
        exact(got.contiguous(), p.ref_w.to(F32), what)
    else:
        R.close_f32(got, p.ref_w, "gemm_acc", what, scale=p.S_w)
    if p.db is not None:
        db_after = db_after.cpu()
        exact(db_after[p.N:], p.db[p.N:], what + " bias guard")
        if touched_bias:
            if exactf:
                exact(db_after[:p.N], p.ref_b.to(F32), what + " bias sums")
            R.close_f32(db_after[:p.N], p.ref_b, "gemm_bsum", what + " bias sums", scale=p.S_b)
        else:
            exact(db_after[:p.N], p.db[:p.N], what + " bias untouched")


COLSUM_NS = (1, 63, 64, 65, 200)


def colsum_ms(rpb):
    return (1, 31, 32, 33, rpb - 1, rpb + 1, 2 * rpb + 3)


def colsum_case(M, N, beta, odd_ld, seed=0):
    """(x view bf16 [M, N] inside a NaN-padded buffer, out f32 [N] + sentinel, ref, scale)."""
    c = Case("tol", 0, "nt", M, N, 1, 0, True, 1.0, beta, "tight", "n", seed=seed)
    xv = torch.randn(M, N, generator=_gen(1, c)).to(BF16)
    ld = (round8(N) + 3) if odd_ld else round8(N)
    buf = torch.full(((M + 2) * ld + 8,), float("nan"), dtype=BF16)
    x = buf.as_strided((M, N), (ld, 1), ld if not odd_ld else round8(ld))
    x.copy_(xv)
    old = torch.randn(N, generator=_gen(2, c)).to(F32)
    out = sentinel(N + 4, True)
    if beta != 0:
        out[:N] = old
    ref = xv.to(F64).sum(0) + (beta * old.to(F64) if beta != 0 else 0.0)
    scale = xv.to(F64).abs().sum(0) + (beta * old.to(F64)).abs()
    return x, out, ref, scale


def colsum_f32(x, out, N, beta, mutant=None):
    o = out.clone()
    s = x.to(F32).sum(0)
    if mutant == "last_row_dropped":
        s = x[:-1].to(F32).sum(0) if x.shape[0] > 1 else s * 0
    o[:N] = s + (beta * out[:N] if beta != 0 else 0.0)
    return o


def check_colsum(got, out0, ref, scale, N, what, key="colsum"):
    got = got.cpu()
    exact(got[N:], out0[N:], what + " guard after out[N]")
    R.close_f32(got[:N], ref, key, what, scale=scale)
