#!/usr/bin/env python3
"""Isolated timing of the FFN ReLU-backward dgrad shapes (8192x2048x512 and
8192x4096x1024, NN, cfg 12): EPI_DRELU with the bf16 mask, EPI_NONE, and
EPI_DRELU with the mask as a bitmap (skipped on a build without relu_bits:
set TDG_PKG_ROOT to time another copy of the package) -- back to back (warm)
and with a 512 MB fill between reps (cold). HIP events around single
launches, median and min; an optional argument names a JSON file to write
the table to. Results: profiles/relu_bits/."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if os.environ.get("TDG_PKG_ROOT"):  # another copy of the package (and its built _C)
    sys.path.insert(0, os.path.abspath(os.environ["TDG_PKG_ROOT"]))
from tensorflow_distributed_on_gke_amd.ops import kernels as kk  # noqa: E402

DEV = "cuda"
FLUSH = torch.empty(128 * 1024 * 1024, dtype=torch.float32, device=DEV)


def timeit(fn, reps=30, cold=True):
    ts = []
    for r in range(reps + 3):
        if cold:
            FLUSH.fill_(float(r))
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if r >= 3:
            ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return round(ts[len(ts) // 2], 2), round(ts[0], 2)


def main():
    torch.manual_seed(0)
    out = {}
    for (M, N, K) in ((8192, 2048, 512), (8192, 4096, 1024)):
        A = torch.randn(M, K, device=DEV).bfloat16()
        B = (torch.randn(K, N, device=DEV) * 0.05).bfloat16()
        aux = torch.randn(M, N, device=DEV).bfloat16()
        C = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)

        def drelu():
            kk.gemm(A, B, C, M, N, K, K, N, N, True, False, epi=kk.EPI_DRELU, aux=aux, ldaux=N, cfg=(12, 1))

        def none():
            kk.gemm(A, B, C, M, N, K, K, N, N, True, False, epi=kk.EPI_NONE, cfg=(12, 1))

        row = {}
        for cold in (False, True):
            tag = "cold" if cold else "warm"
            row[f"drelu_{tag}_us(med,min)"] = timeit(drelu, cold=cold)
            row[f"none_{tag}_us(med,min)"] = timeit(none, cold=cold)
        if hasattr(kk, "pack_relu_bits"):
            bits = kk.pack_relu_bits(aux)
            ref = C.clone()
            drelu()
            ref.copy_(C)

            def dbits():
                kk.gemm(A, B, C, M, N, K, K, N, N, True, False, epi=kk.EPI_DRELU, relu_bits=bits, cfg=(12, 1))
            dbits()
            row["bits_equal"] = bool(torch.equal(ref.view(torch.int16), C.view(torch.int16)))
            for cold in (False, True):
                tag = "cold" if cold else "warm"
                row[f"dbits_{tag}_us(med,min)"] = timeit(dbits, cold=cold)
        out[f"{M}x{N}x{K}"] = row
        print(json.dumps({f"{M}x{N}x{K}": row}), flush=True)
    if len(sys.argv) > 1:  # also keep the table as JSON
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        json.dump(out, open(sys.argv[1], "w"), indent=1)


if __name__ == "__main__":
    main()
