"""The weight EMA's numerical contract, shared by the CPU and the GPU tests.

One update from identical f32 inputs is compared with a float64 reference
that takes `decay` and `d_eff` rounded to f32:

    d_eff = decay, or with warm-up min(decay, (1 + count) / (10 + count))
    e'    = e + (p - e) * (1 - d_eff)             (count == 0: e' = p)

The error must be at most 8 * 2^-24 * (|p| + |e|) elementwise: the f32
arithmetic rounds three times (subtract, multiply, add), `1 - d_eff` carries
up to two more ulps from the warm-up division, and each is at most half an
ulp of a quantity no larger than |p| + |e| -- fewer than 8 half-ulps.

Multi-step checks apply the bound step by step (the EMA after step k against
the one-step reference from the code's own EMA after step k - 1 and the
weights after step k), so nothing compounds.
"""
import torch

ULP = 2.0 ** -24


def d_eff32(decay: float, warmup: bool, count: int) -> torch.Tensor:
    """The decay of the update that follows `count` earlier ones, formed in f32."""
    d = torch.tensor(decay, dtype=torch.float32)
    if warmup:
        c = torch.tensor(float(count), dtype=torch.float32)
        d = torch.minimum(d, (torch.tensor(1.0) + c) / (torch.tensor(10.0) + c))
    return d


def one_step64(p: torch.Tensor, e: torch.Tensor, decay: float, warmup: bool, count: int) -> torch.Tensor:
    """float64 EMA after one update of e (f32, before) from p (f32)."""
    if count == 0:
        return p.double()
    d = d_eff32(decay, warmup, count).double().to(p.device)
    return e.double() + (p.double() - e.double()) * (1.0 - d)


def bound(p: torch.Tensor, e: torch.Tensor) -> torch.Tensor:
    return 8 * ULP * (p.double().abs() + e.double().abs())


def check_one_step(got: torch.Tensor, p: torch.Tensor, e_before: torch.Tensor, decay: float,
                   warmup: bool, count: int, what: str = "") -> float:
    """Assert the contract for one update; returns the largest error / bound."""
    want = one_step64(p, e_before, decay, warmup, count)
    if count == 0:
        assert torch.equal(got.view(torch.int32), p.view(torch.int32)), f"{what}: first update is not a bitwise copy"
        return 0.0
    err = (got.double() - want).abs()
    lim = bound(p, e_before)
    assert torch.isfinite(got).all(), f"{what}: non-finite EMA"
    worst = float((err / lim.clamp_min(1e-300)).max())
    print(f"{what}: count {count} d_eff {float(d_eff32(decay, warmup, count)):.8f} "
          f"max err / bound {worst:.3f}")
    assert bool((err <= lim).all()), f"{what}: EMA off the float64 reference by {worst:.2f} x the bound"
    return worst
