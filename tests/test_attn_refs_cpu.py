"""tests/ref_attn.py on the CPU: its backward formulas are float64 autograd of
its forward (the kv_len == 0 row included, and that row agrees with
ops/kernels/attention._ref_attn_fwd); its comparators accept the plain float32
evaluation of every case table and reject every mutant on the tables
tests/test_gpu_attn.py runs; its exact builder's premises hold (build()
asserts them), its guards, poison and traps are in place; its tolerance table
is measured; and its case tables reach every arm of the bf16 attention family
at every head dim it exists for, and every edge the launchers and tiles have
(walked with expected_arm, the Python mirror of the launchers)."""
import math

import pytest
import torch

import ref_attn as A
import ref_tail as R
from ref_attn import F32, F64

TABLES = [(arm, hd, H) for arm, hd, H, _ in A.all_tables()]


def _id(t):
    return f"{t[0]}-hd{t[1]}-H{t[2]}"


@pytest.mark.parametrize("table", TABLES, ids=_id)
def test_f32_evaluation_passes_and_cases_are_sound(table):
    """The float32 evaluation passes every comparator (bitwise in the exact
    family: check() holds O, dV, dQ, dK of its one-hot rows to the selected V
    rows, the scatter-add and 0); guards, poison and traps are in place
    before any kernel would run."""
    arm, hd, H = table
    for c in A.cases(arm, hd, H):
        assert c.arm.family == arm and c.arm.hd == hd, c.what()
        bt = A.build(c)
        A.check_pristine(bt)
        A.check(bt, A.attn_f32(bt))


def _differs(bt, x, y):
    return any(not bool((A.G._as_int(x[p]) == A.G._as_int(y[p])).all()) for p in bt.outputs())


@pytest.mark.parametrize("table", TABLES, ids=_id)
def test_every_mutant_is_rejected(table):
    """Every mutant that can change an operation at all is rejected by some
    case of every arm's table; the unrounded-P evaluation is accepted
    everywhere (the bound is one-sided)."""
    arm, hd, H = table
    tab = A.cases(arm, hd, H)
    op = A.ARM_OP[arm]
    todo = [m for m in A.MUTANTS if op in A.MUTANT_OPS[m] and m not in A.ACCEPTED_MUTANTS]
    hit = {}
    for c in tab:
        if len(hit) == len(todo):
            break
        bt = A.build(c)
        clean = None
        for m in todo:
            if m in hit:
                continue
            if clean is None:
                clean = A.attn_f32(bt)
            mut = A.attn_f32(bt, mutant=m)
            if _differs(bt, mut, clean) and A.rejected(bt, mut):
                hit[m] = c.what()
    assert sorted(hit) == sorted(todo), f"{arm} hd{hd}: accepted everywhere: {sorted(set(todo) - set(hit))}"
    if op in A.MUTANT_OPS["p_unrounded"]:
        n = 0
        for c in [c for c in tab if c.family != "exact"][::4]:
            bt = A.build(c)
            mut = A.attn_f32(bt, mutant="p_unrounded")
            n += _differs(bt, mut, A.attn_f32(bt))
            A.check(bt, mut)
        assert n > 0


def test_mutant_table_is_complete():
    assert set(A.MUTANT_OPS) == set(A.MUTANTS) and set(A.ACCEPTED_MUTANTS) <= set(A.MUTANTS)
    for m, ops in A.MUTANT_OPS.items():
        assert set(ops) <= set(A.ARM_OP.values()), m
    # every operation is met by a window, a diagonal (where it can be causal), a kv_len == 0,
    # an unwritten-row and a guard mutant
    for op in set(A.ARM_OP.values()):
        for m in ("window_wide", "window_narrow", "kv0_nothing", "kv0_keeps_scale", "tail_rows_unwritten",
                  "row_at_Lq"):
            assert op in A.MUTANT_OPS[m], (op, m)


def test_e_table_is_measured():
    """Every tolerance is 8 x an E32 that this machine reproduces: not below
    what the float32 evaluation needs, and not inflated."""
    got = {}
    for arm, hd, H, tab in A.all_tables():
        for c in tab:
            A.measure_e32(A.build(c), got)
    print("measured E32:", {k: f"{v:.2e}" for k, v in sorted(got.items())})
    assert set(got) == set(A.E32)
    for k, e in A.E32.items():
        # (the same bounds as tests/test_loss_optim_refs_cpu.py::test_e32_table_is_measured)
        assert got[k] <= 1.5 * e, f"{k}: measured {got[k]:.3e} above the table's {e:.3e}"
        assert got[k] >= e / 4, f"{k}: the table's {e:.3e} is more than 4x the measured {got[k]:.3e}"
    assert A.MARGIN == R.MARGIN == 8.0 and all(math.isclose(R.tol(k), 8 * e) for k, e in A.E32.items())
    assert not set(A.E32) & set(R.E32)


# --------------------------------------------------------------------------- the formulas against the mathematics
def _f32_absorbed(x):
    """x as float32 holds it, with the gradient of x: what the model's float32
    `logits + mask * -1e9` does to a masked logit (the sum is -1e9 exactly for
    every |logit| < 32, and the add passes the gradient through)."""
    return x + (x.to(F32).to(F64) - x).detach()


def _model_forward(c, q, k, v, scale):
    """softmax(scale Q K^T + mask * -1e9) V in float64, the mask the maximum
    of the padding and the look-ahead mask, as the model writes it."""
    # the kernels' exponent is exp2(c S): the same softmax as exp(c S ln 2)
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) * (A.c_of(scale) * math.log(2.0))
    keys = torch.arange(c.Lk)
    mask = torch.zeros(c.B, 1, c.Lq, c.Lk, dtype=F64)
    if c.kv is not None:
        mask = mask + (keys.view(1, 1, 1, -1) >= torch.tensor(c.kv).view(-1, 1, 1, 1)).to(F64)
    if c.causal:
        mask = torch.maximum(mask, (keys.view(1, -1) > torch.arange(c.Lq).view(-1, 1)).to(F64).view(1, 1, c.Lq, c.Lk))
    logits = torch.where(mask > 0, _f32_absorbed(s + mask * -1e9), s)
    p = torch.softmax(logits, -1)
    return torch.einsum("bhqk,bkhd->bqhd", p, v), p


AUTOGRAD_CASES = [
    A.Case("bwd", "flat", 16, 17, 17, "pad+causal", (17, 0, 1, 16), "gap"),
    A.Case("bwd", "peaky", 32, 33, 65, "pad", (65, 0, 1, 64), "gap"),
    A.Case("bwd", "ramp_up", 64, 70, 130, "none", None, "gap"),
    A.Case("bwd", "flat", 128, 5, 5, "causal", None, "gap"),
]


@pytest.mark.parametrize("c", AUTOGRAD_CASES, ids=lambda c: c.what().replace(" ", "_"))
def test_backward_reference_is_float64_autograd(c):
    """With unrounded float64 o and lse, bwd_math equals float64 autograd of
    the forward written as the model writes it, kv_len == 0 row included; the
    forward reference equals that forward, and its kv_len == 0 row agrees with
    ops/kernels/attention._ref_attn_fwd."""
    from tensorflow_distributed_on_gke_amd.ops.kernels.attention import _ref_attn_fwd

    bt = A.build(c)
    q, k, v, do = (bt.val(n).clone().requires_grad_(n != "do") for n in ("q", "k", "v", "do"))
    O, P = _model_forward(c, q, k, v, bt.scale)
    (O * do).sum().backward()
    f = A.fwd_math(c, q.detach(), k.detach(), v.detach(), bt.scale)
    assert float((f["O"] - O.detach()).abs().max()) <= 1e-12 * float(O.detach().abs().max())
    assert float((f["P"] - P.detach()).abs().max()) <= 1e-12
    r = A.bwd_math(c, q.detach(), k.detach(), v.detach(), f["O"], do, f["lse"], bt.scale)
    # (dQ / dK carry `scale`, the exponent scale * f32(log2 e): equal to 2^-25)
    for name, g in (("dq", q.grad), ("dk", k.grad), ("dv", v.grad)):
        err = float((r[name] - g).abs().max())
        assert err <= 1e-7 * float(g.abs().max()), (name, err)
    # lse is log2 of the sum over the attended keys
    z = f["z"].masked_fill(~f["att"], -math.inf)
    assert float((f["lse"] - torch.logsumexp(z * math.log(2.0), -1) / math.log(2.0)).abs().max()) <= 1e-10
    if c.kv is not None and 0 in c.kv:
        b = c.kv.index(0)
        assert float((f["P"][b] - 1.0 / c.Lk).abs().max()) <= 1e-15  # uniform over all Lk keys, causal off
        assert float((f["lse"][b] - math.log2(c.Lk)).abs().max()) <= 1e-12
        assert float(r["dq"][b].abs().max()) > 0 and float(r["dk"][b].abs().max()) > 0  # the real scale
        o32, p32 = _ref_attn_fwd(bt.view("q").float(), bt.view("k").float(), bt.view("v").float(),
                                 torch.tensor(c.kv), c.causal, bt.scale)
        assert float((p32[b].double() - f["P"][b]).abs().max()) <= 1e-6
        assert float((o32.double() - f["O"]).abs().max()) <= 1e-4 * float(f["O"].abs().max())


# --------------------------------------------------------------------------- what the tables reach
def test_expected_arm_mirrors_the_launchers():
    E = A.expected_arm
    assert E("fwd", 64, 64, 200) == A.Arm("fwd64", 64, 12, 256, 0)
    assert E("fwd", 64, 65, 1) == A.Arm("fwd128", 64, 12, 256, 0)
    assert E("fwd", 64, 128, 1) == A.Arm("fwd128", 64, 12, 256, 0)
    assert E("fwd", 64, 129, 1) == A.Arm("fwd_pipe", 64, 24, 512, 0)
    assert E("fwd", 32, 129, 1) == A.Arm("fwd128", 32, 24, 256, 0)
    assert E("fwd", 128, 257, 1) == A.Arm("fwd128w8", 128, 36, 512, 0)
    assert E("probs", 16, 5, 9) == A.Arm("probs", 16, 15, 256, 0)
    assert E("bwd", 64, 128, 128) == A.Arm("bwd_fused", 64, 12, 512, 0)
    assert E("bwd", 64, 129, 1) == A.Arm("bwd_pipe", 64, 24, 256, 12)
    assert E("bwd", 64, 1, 129) == A.Arm("bwd_pipe", 64, 12, 256, 24)
    assert E("bwd", 16, 130, 200) == A.Arm("bwd_split", 16, 36, 256, 48)
    assert E("fdo", 64, 128, 128, H=2) == A.Arm("bwd_fdo", 64, 8, 512, 0)
    assert E("qkv_cross", 64, 37, 128, H=1) == A.Arm("qkv_cross", 64, 4, 512, 0)


def test_case_tables_reach_every_arm_and_edge():
    pts, kvs, masks, fams, lays, modes, heads = {}, {}, {}, {}, {}, {}, {}
    for arm, hd, H, tab in A.all_tables():
        for c in tab:
            assert c.arm.family == arm and c.arm.hd == hd
            assert c.B == 4 and (c.H == 3 or arm.startswith("qkv"))
            assert arm.startswith("qkv") or c.B * c.H % 8 != 0  # grids that the XCD remap does not divide
            assert c.B * max(c.Lq, c.Lk) * c.H * c.hd <= 4 * 321 * 3 * 128
            key = (arm, hd)
            pts.setdefault(key, set()).add((c.Lq, c.Lk, c.causal))
            kvs.setdefault(key, set()).update(["None"] if c.kv is None else
                                              [{c.Lk: "Lk", 0: "0", 1: "1"}.get(n, "edge") for n in c.kv] +
                                              [f"={n}" for n in c.kv])
            masks.setdefault(key, set()).add(c.mask)
            fams.setdefault(key, set()).add(c.family)
            lays.setdefault(key, set()).add(c.layout)
            heads.setdefault(arm, set()).add(c.H)
            if c.family == "exact":
                got = A.build(c).modes
                modes.setdefault(key, set()).update(m for m, n in got.items() if n)
    # every family word at every head dim it exists for
    assert set(pts) == {(arm, hd) for arm, hds in A.ARM_HDS.items() for hd in hds}
    assert heads["qkv_self"] == heads["qkv_cross"] == {1, 2, 3}  # d = 64, 128, 192: 1, 2, 3 projection K tiles

    def has(key, lqs, lks):
        got = {(q, k) for q, k, _ in pts[key]}
        assert got >= {(q, k) for q in lqs for k in lks}, (key, sorted({(q, k) for q in lqs for k in lks} - got))

    def causal_at(key, ls):
        assert {q for q, k, cz in pts[key] if cz and q == k} >= set(ls), key

    for hd in A.HDS:
        has(("fwd64", hd), (1, 16, 17, 63, 64), (1, 63, 64, 65, 129))
        arm = "fwd128" if hd <= 64 else "fwd128w8"
        has((arm, hd), (65, 127, 128) if hd == 64 else (65, 128, 129, 257), (1, 127, 128, 129, 257))
        causal_at((arm, hd), (65, 128) if hd == 64 else (65, 128, 129))
        has(("bwd_fused", hd), (1, 16, 17, 33, 127, 128), (1, 17, 64, 65, 128))
        causal_at(("bwd_fused", hd), (1, 17, 128))
        assert {k for _, k, _ in pts[("probs", hd)]} == {1, 63, 64, 65, 200}
    has(("fwd_pipe", 64), (129, 256, 257), (1, 64, 65, 128, 129, 192, 193, 257))  # 1 to 5 key tiles, 3-slot ring
    causal_at(("fwd_pipe", 64), (129, 193, 257))
    has(("bwd_fdo", 64), (1, 16, 17, 33, 127, 128), (1, 17, 64, 65, 128))
    for hd in (16, 32, 128):
        assert {(q, k) for q, k, _ in pts[("bwd_split", hd)]} == {(1, 129), (129, 1), (129, 129), (130, 200), (200, 65)}
        causal_at(("bwd_split", hd), (129,))
    assert {(q, k) for q, k, _ in pts[("bwd_pipe", 64)]} == \
        {(1, 129), (129, 1), (129, 64), (64, 129), (129, 129), (257, 193), (193, 257), (321, 321)}
    causal_at(("bwd_pipe", 64), (129, 321))
    assert {q for q, _, _ in pts[("qkv_self", 64)]} == {1, 17, 64, 65, 127, 128}
    assert {(q, k) for q, k, _ in pts[("qkv_cross", 64)]} == {(1, 128), (128, 1), (65, 64), (64, 65), (37, 128), (128, 77)}
    # the shapes no earlier test drove: a decoder batch of many targets over few sources and the reverse
    assert any(q > 128 and k <= 64 for q, k, _ in pts[("bwd_pipe", 64)] | pts[("fwd_pipe", 64)])
    assert any(q == 1 and k > 128 for q, k, _ in pts[("bwd_pipe", 64)])
    for key in pts:
        assert kvs[key] >= {"None", "Lk", "0", "1"}, (key, kvs[key])
        assert lays[key] == set(A.LAYOUTS), key
        arm = key[0]
        want = {"none", "pad"} | (set() if arm == "qkv_cross" else {"causal", "pad+causal"})
        assert masks[key] == want, (key, masks[key])
        assert fams[key] == ({"flat", "peaky"} if arm.startswith("qkv") else set(A.FAMILIES)), (key, fams[key])
        if arm in ("fwd64", "fwd128", "fwd128w8", "fwd_pipe", "bwd_fused", "bwd_fdo", "bwd_split", "bwd_pipe"):
            assert modes[key] == set(A.SEL_MODES), (key, set(A.SEL_MODES) - modes[key])
            assert kvs[key] & {"=64", "=65"}, key  # a key window that ends at / one past a tile edge
        if arm != "probs" and not (arm == "qkv_self"):
            assert "edge" in kvs[key], key


def test_selection_modes_are_what_they_say():
    c = next(c for c in A.cases("fwd_pipe", 64) if c.family == "exact" and c.causal and c.kv is not None)
    bt = A.build(c)
    klim, causal, lf = A.window(c)
    seen = set()
    for b in range(c.B):
        for i in range(c.Lq):
            n = min(klim[b], i + 1) if causal[b] else klim[b]
            for h in range(c.H):
                key = int(bt.sel[b, h, i])
                assert 0 <= key < n
                if key == n - 1:
                    seen.add("last attended")
                if causal[b] and key == i:
                    seen.add("diagonal")
                seen.add({0: "first of 16", 15: "last of 16"}.get(key % 16, ""))
                seen.add({0: "first of 64", 63: "last of 64"}.get(key % 64, ""))
                seen.add("earlier tile" if key // 64 < (n - 1) // 64 else "last tile")
    assert seen >= {"last attended", "diagonal", "first of 16", "last of 16", "first of 64", "last of 64",
                    "earlier tile", "last tile"}


def test_ramps_move_the_row_maximum_as_they_say():
    """ramp_up: every 64-key tile raises the row maximum (the online rescale
    runs on every tile); ramp_down: no tile after the first does (the
    __ballot(mn > m) skip is taken)."""
    for fam in ("ramp_up", "ramp_down"):
        c = next(c for c in A.cases("fwd_pipe", 64) if c.family == fam and c.Lk >= 192 and not c.causal)
        bt = A.build(c)
        f = A.fwd_math(c, bt.val("q"), bt.val("k"), bt.val("v"), bt.scale)
        z = f["z"].masked_fill(~f["att"], -math.inf)
        klim, _, lf = A.window(c)
        for b in range(c.B):
            nt = klim[b] // 64  # whole tiles
            if not lf[b] or nt < 2:
                continue
            tmax = z[b, :, :, :64 * nt].reshape(c.H, c.Lq, nt, 64).max(-1).values
            d = tmax[..., 1:] - tmax[..., :-1]
            assert bool((d > 0).all()) if fam == "ramp_up" else bool((d < 0).all()), (fam, b)


def test_guards_catch_a_stray_row_and_an_unwritten_one():
    c = A.cases("bwd_fused", 64)[1]
    bt = A.build(c)
    good = A.attn_f32(bt)
    A.check(bt, good)
    for m, pat in (("row_at_Lq", "guard overwritten"), ("tail_rows_unwritten", "never written"),
                   ("dkdv_tail_unwritten", "never written")):
        cc = next(x for x in A.cases("bwd_fused", 64) if x.kv is not None and x.Lq % 16 and x.Lk >= 64)
        b2 = A.build(cc)
        with pytest.raises(A.Mismatch, match=pat):
            A.check(b2, A.attn_f32(b2, mutant=m))
    # an input buffer that a kernel wrote to
    bad = {p: t.clone() for p, t in good.items()}
    pool = bt.where["q"]
    bad[pool][0] = 1.0
    with pytest.raises(A.Mismatch, match="input buffer"):
        A.check(bt, bad)
