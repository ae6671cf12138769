"""bf16 GEMM family (csrc/kernels/gemm*.hip): tile heuristic, tuned table,
the linear-layer forms, grouped / ragged weight gradients, column sums."""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import torch

from tensorflow_distributed_on_gke_amd.ops import tuning
from tensorflow_distributed_on_gke_amd.ops._ext import C
from tensorflow_distributed_on_gke_amd.ops.kernels.workspace import NUM_CU, workspace

EPI_NONE, EPI_BIAS, EPI_BIAS_RELU, EPI_DRELU = 0, 1, 2, 3

# tile configs (see csrc/kernels/gemm.hip): 0=128x128, 1=128x64, 2=64x128, 3=64x64
_TILES = {0: (128, 128), 1: (128, 64), 2: (64, 128), 3: (64, 64), 4: (128, 128), 5: (256, 128),
          6: (128, 256), 7: (64, 128), 8: (64, 64), 9: (256, 128), 10: (128, 256), 11: (128, 128),
          12: (256, 256), 13: (128, 128), 14: (128, 128),
          20: (256, 256), 21: (256, 128), 22: (128, 256)}
_CFG_OVERRIDE: Dict[Tuple[int, int, int, bool, bool], Tuple[int, int]] = {}


def set_gemm_config(M: int, N: int, K: int, a_kc: bool, b_kc: bool, cfg: int, splits: int) -> None:
    _CFG_OVERRIDE[(M, N, K, a_kc, b_kc)] = (cfg, splits)


def choose_gemm(M: int, N: int, K: int, a_kc: bool = True, b_kc: bool = True) -> Tuple[int, int]:
    """Tile config (and split-K) for a shape with no tuned entry -- no timed
    search at run time. From the in-tree sweep on MI355X
    (scripts/gemm_vs_blas.py, profiles/gemm/r3_tile_sweep_*.txt): 256x256
    tiles once they fill the chip (>= 192 tiles, K % 64 == 0); for the
    d_model-wide dgrads (N = 1024) 128x256 tiles, 8 waves; otherwise 128x128
    tiles, 8 waves, 3-4 stages. Weight gradients (K = tokens, small output,
    normally the ragged launch) split K to fill 256 CUs."""
    o = _CFG_OVERRIDE.get((M, N, K, a_kc, b_kc))
    if o is not None:
        return o
    if not a_kc and not b_kc:  # weight gradient: split K (= tokens)
        t128 = math.ceil(M / 128) * math.ceil(N / 128)
        splits = 1
        while t128 * splits < NUM_CU and K // (splits * 2) >= 512:
            splits *= 2
        return 0, splits
    if K % 64 == 0 and math.ceil(M / 256) * math.ceil(N / 256) >= 192:
        return 12, 1
    if a_kc and not b_kc and N >= 1024 and math.ceil(M / 128) * math.ceil(N / 256) >= NUM_CU:
        return 6, 1
    return (13, 1) if not b_kc else (4, 1)


_TUNED: Dict[tuple, Tuple[int, int]] = {}
_CANDIDATES = [(0, 1), (4, 1), (5, 1), (6, 1), (9, 1), (10, 1), (12, 1), (13, 1), (14, 1),
               (20, 1), (21, 1), (22, 1)]


def _autotune(key, run) -> Tuple[int, int]:
    """Time the candidate tile configs once for this problem
    (tuning.time_candidates) and keep the fastest."""
    M, N, K, a_kc, b_kc = key[:5]
    cands = list(_CANDIDATES)
    if not a_kc and not b_kc:
        cands = [(c, s) for c in (0, 7, 8) for s in (1, 2, 4, 8) if K // s >= 256] + [(12, 1)]
    return tuning.time_candidates(cands, run, 5)


def _key_str(k: tuple) -> str:
    M, N, K, a_kc, b_kc, epi, dt, ld8, beta = k
    return f"{M},{N},{K},{int(a_kc)},{int(b_kc)},{epi},{str(dt).replace('torch.', '')},{int(ld8)},{int(beta)}"


def _parse_key(ks: str) -> tuple:
    M, N, K, a, b, epi, dt, ld8, beta = ks.split(",")
    return (int(M), int(N), int(K), bool(int(a)), bool(int(b)), int(epi), getattr(torch, dt),
            bool(int(ld8)), bool(int(beta)))


def save_tuned(path: str) -> None:
    """Persist the autotuned GEMM choices (JSON) so later runs are
    deterministic and skip tuning."""
    tuning.save_table(path, ((_key_str(k), list(v[0]))
                             for k, v in sorted(_TUNED.items(), key=lambda kv: str(kv[0]))))


def load_tuned(path: str) -> int:
    table = tuning.load_table(path, _parse_key, lambda v: ((int(v[0]), int(v[1])),) * 2)
    _TUNED.update(table)
    return len(table)


TUNED_FILE = tuning.table_file("TDG_GEMM_TUNED_FILE", "gemm_tuned_gfx950.json")
load_tuned(TUNED_FILE)


def _tok_bucket(v: int) -> int:
    return -(-v // 1024) * 1024


def gemm(A, B, Cout, M, N, K, lda, ldb, ldc, a_kc, b_kc, epi=EPI_NONE, bias=None, aux=None,
         ldaux=0, alpha=1.0, beta=0.0, cfg: Optional[Tuple[int, int]] = None,
         relu_bits: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Every GEMM of the model: the in-tree MFMA kernels (csrc/kernels/gemm.hip)
    with the tile config from the tuned table, else the heuristic.

    relu_bits: the ReLU mask as a uint8 bitmap [M, >= N / 8] (bit e of byte c =
    column 8c + e, i.e. numpy.packbits(h > 0, axis=1, bitorder="little")):
    EPI_BIAS_RELU writes it, EPI_DRELU reads it instead of aux. N % 8 == 0;
    the tuning key is that of the plain epilogue."""

    def run(c, out=Cout):
        tile, splits = c
        ws = workspace("splitk", splits * M * ldc, A.device) if splits > 1 else None
        if relu_bits is None:
            C().gemm(A, B, out, bias, aux, M, N, K, lda, ldb, ldc, ldaux, a_kc, b_kc, epi, alpha,
                     beta, tile, splits, ws)
        else:
            C().gemm(A, B, out, bias, aux, M, N, K, lda, ldb, ldc, ldaux, a_kc, b_kc, epi, alpha,
                     beta, tile, splits, ws, relu_bits=relu_bits, ldbits=relu_bits.stride(0))

    if cfg is None:
        # token-count dimensions (M of forward / dgrad, K of wgrad) are bucketed
        # to multiples of 1024 for the tuning key, so variable-length text
        # batches reuse a handful of tunings instead of re-tuning every length
        Mk, Kk = (M, _tok_bucket(K)) if (not a_kc and not b_kc) else (_tok_bucket(M), K)
        key = (Mk, N, Kk, a_kc, b_kc, epi, Cout.dtype, ldc % 8 == 0, beta != 0.0)
        ent = _TUNED.get(key)
        if ent is None:
            o = _CFG_OVERRIDE.get((M, N, K, a_kc, b_kc))
            if o is not None:
                ent = (o, o)
        if ent is None and tuning.AUTOTUNE and A.is_cuda and not torch.cuda.is_current_stream_capturing():
            if beta != 0.0:
                # accumulate into C: tune on a scratch copy so C is untouched
                scratch = workspace("tune_c", Cout.numel(), A.device, Cout.dtype)[: Cout.numel()]
                scratch = scratch.view_as(Cout)
                best = _autotune(key, lambda c: run(c, scratch))
            else:
                best = _autotune(key, run)
            ent = (best, best)
            _TUNED[key] = ent
        if ent is None:
            cfg = choose_gemm(M, N, K, a_kc, b_kc)
        else:
            cfg = ent[0]
    run(cfg)
    return Cout


def tuned_table() -> Dict[str, str]:
    return {f"{k[0]}x{k[1]}x{k[2]} a_kc={k[3]} b_kc={k[4]} epi={k[5]}": f"cfg{v[0]} split{v[1]}"
            for k, v in _TUNED.items()}


def pack_relu_bits(h: torch.Tensor) -> torch.Tensor:
    """The ReLU bitmap [M, N / 8] of a hidden activation h [M, N] (N % 8 == 0),
    as the bias+ReLU epilogue writes it: bit e of byte c = (h[:, 8c + e] > 0)."""
    M, N = h.shape
    w = (1 << torch.arange(8, device=h.device, dtype=torch.int32))
    return ((h > 0).view(M, N // 8, 8).to(torch.int32) * w).sum(-1).to(torch.uint8)


def linear_fwd(x2: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], relu: bool = False,
               out: Optional[torch.Tensor] = None, ldc: Optional[int] = None,
               relu_bits: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y[M,N] = x[M,K] @ w[N,K]^T + bias (bf16 out). relu_bits (with relu):
    also writes the ReLU bitmap (y > 0) into this uint8 [M, >= N / 8] tensor."""
    M, K = x2.shape
    N = w.shape[0]
    ldc = ldc or N
    if out is None:
        out = torch.empty(M, ldc, dtype=torch.bfloat16, device=x2.device)
    epi = EPI_BIAS_RELU if relu else (EPI_BIAS if bias is not None else EPI_NONE)
    if relu_bits is not None and not relu:
        raise ValueError("linear_fwd: relu_bits needs relu=True")
    return gemm(x2, w, out, M, N, K, x2.stride(0), w.stride(0), ldc, True, True, epi, bias=bias,
                relu_bits=relu_bits)


def linear_dgrad(dy2: torch.Tensor, w: torch.Tensor, N: int, relu_aux: Optional[torch.Tensor] = None,
                 out: Optional[torch.Tensor] = None, beta: float = 0.0,
                 relu_bits: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dx[M,K] = dy[M,N] @ w[N,K] (optionally * (relu_aux > 0), the mask given
    as the bf16 activation relu_aux or as its bitmap relu_bits)."""
    M = dy2.shape[0]
    K = w.shape[1]
    if out is None:
        out = torch.empty(M, K, dtype=torch.bfloat16, device=dy2.device)
    if relu_bits is not None:
        relu_aux = None
    epi = EPI_DRELU if (relu_aux is not None or relu_bits is not None) else EPI_NONE
    return gemm(dy2, w, out, M, K, N, dy2.stride(0), w.stride(0), out.stride(0), True, False, epi,
                aux=relu_aux, ldaux=(relu_aux.stride(0) if relu_aux is not None else 0), beta=beta,
                relu_bits=relu_bits)


def transpose_grouped(srcs, dsts) -> None:
    """dsts[g] = srcs[g].T for same-shape bf16 matrices, one launch per 64."""
    for c0 in range(0, len(srcs), 64):
        C().transpose_grouped(list(srcs[c0:c0 + 64]), list(dsts[c0:c0 + 64]))


def linear_dgrad_t(dy2: torch.Tensor, w_t: torch.Tensor, relu_aux: Optional[torch.Tensor] = None,
                   out: Optional[torch.Tensor] = None,
                   relu_bits: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dx[M,N] = dy[M,K] @ w[K,N] computed against the weight's transposed copy
    w_t [N, K] (K-contiguous): the forward (NT) operand layout, whose kernels
    are faster than the N-contiguous dgrad ones; optional ReLU-backward mask."""
    M, K = dy2.shape
    N = w_t.shape[0]
    if out is None:
        out = torch.empty(M, N, dtype=torch.bfloat16, device=dy2.device)
    if relu_bits is not None:
        relu_aux = None
    epi = EPI_DRELU if (relu_aux is not None or relu_bits is not None) else EPI_NONE
    return gemm(dy2, w_t, out, M, N, K, dy2.stride(0), w_t.stride(0), out.stride(0), True, True, epi,
                aux=relu_aux, ldaux=(relu_aux.stride(0) if relu_aux is not None else 0),
                relu_bits=relu_bits)


def linear_wgrad(dy2: torch.Tensor, x2: torch.Tensor, N: int, dw: torch.Tensor,
                 beta: float = 0.0) -> torch.Tensor:
    """dw[N,K] (f32) (+)= dy[M,N]^T @ x[M,K]."""
    M, K = x2.shape
    return gemm(dy2, x2, dw, N, K, M, dy2.stride(0), x2.stride(0), dw.stride(0), False, False,
                EPI_NONE, beta=beta)


_GROUP_TUNED: Dict[tuple, int] = {}
_GROUP_CANDS = (0, 4, 5, 6, 7, 8, 2, 12)


def wgrad_grouped(dys, xs, dws, beta: float = 0.0) -> None:
    """dws[i][N,K] (f32) (+)= dys[i][M,N]^T @ xs[i][M,K] for up to 32 same-shape
    problems in ONE launch (blockIdx.y = problem): whole-K tiles over the
    whole chip, no split-K slabs."""
    M, K = xs[0].shape
    N = dws[0].shape[0]
    lda, ldb, ldc = dys[0].stride(0), xs[0].stride(0), dws[0].stride(0)

    def run(c):
        C().gemm_grouped(dys, xs, dws, N, K, M, lda, ldb, ldc, False, False, 1.0, beta, c)

    key = (M, N, K, len(dys), lda, ldb, beta != 0.0)
    cfg = _GROUP_TUNED.get(key)
    if cfg is None:
        if tuning.AUTOTUNE and not torch.cuda.is_current_stream_capturing():
            scratch = [workspace(f"gw{i}", d.numel(), d.device)[: d.numel()].view_as(d)
                       for i, d in enumerate(dws)]

            def trial(c):
                C().gemm_grouped(dys, xs, scratch, N, K, M, lda, ldb, ldc, False, False, 1.0, 0.0, c)

            cfg = tuning.time_candidates(_GROUP_CANDS, trial, 3)
        else:
            cfg = 0
        _GROUP_TUNED[key] = cfg
    run(cfg)


RAGGED_MAX_PROBLEMS, RAGGED_MAX_SHAPES = 64, 8


def wgrad_ragged(dys, xs, dws, beta: float = 0.0, biases=None, ranges=None) -> None:
    """dws[i][N_i,K_i] (f32) (+)= dys[i][M,N_i]^T @ xs[i][M,K_i] for up to 64
    problems of up to 8 shapes sharing the token count M, as ONE launch of
    256x256 tiles (ragged grouping, csrc/kernels/gemm.hip gemm256_kernel).
    Problems of equal shape must be adjacent. biases[i] (f32 [N_i] or None):
    the bias gradient sum_m dys[i][m] (+ beta * old), summed inside the same
    launch from the dY fragments the MFMAs consume (no second pass over dY).
    ranges[i] = (t_first, t_count) or None: only those 256x256 tiles of
    problem i (in the kernel's enumeration of its tile grid); a cut problem
    gets a shape class of its own."""
    M = xs[0].shape[0]
    shapes = []
    for i, (dy, x, dw) in enumerate(zip(dys, xs, dws)):
        if x.shape[0] != M or dy.shape[0] != M:
            raise ValueError("wgrad_ragged: all problems must share the token count")
        r = ranges[i] if ranges is not None else None
        shapes += [dw.shape[0], x.shape[1], dy.stride(0), x.stride(0), dw.stride(0)]
        shapes += [0, -1] if r is None else [int(r[0]), int(r[1])]
    C().gemm_ragged(list(dys), list(xs), list(dws), shapes, M, False, False, 1.0, beta,
                    list(biases) if biases is not None else [])


def colsum_grouped(xs, outs, beta: float = 0.0) -> None:
    """outs[i][N] (+)= column sums of bf16 xs[i][M, N] (same shape), one
    partial pass + one fold for the whole group."""
    M, N = xs[0].shape[0], outs[0].numel()
    rpb = 256
    part = workspace("colsum_g", len(xs) * math.ceil(M / rpb) * N, xs[0].device)
    C().colsum_grouped(xs, outs, part, M, N, xs[0].stride(0), rpb, beta)


def colsum(x2: torch.Tensor, N: int, out: torch.Tensor, beta: float = 0.0) -> torch.Tensor:
    """out[N] (+)= sum over rows of bf16 x2[M, N]."""
    M = x2.shape[0]
    rpb = 128
    part = workspace("colsum", math.ceil(M / rpb) * N, x2.device)
    C().colsum(x2, out, part, M, N, x2.stride(0), rpb, beta)
    return out
