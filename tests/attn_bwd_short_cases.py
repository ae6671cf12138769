"""Case tables of tests/test_gpu_attn_bwd_short.py (the fused short attention
backward at its row-band edges), shared with tests/test_attn_bwd_short_cpu.py.
Cases are ref_attn.Case, built with ref_attn.build."""
import ref_attn as A

EDGES = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 96, 127, 128)
FAMS = ("flat", "peaky", "ramp_up", "ramp_down", "exact")
FORMS = ("bwd", "fdo")


def _kv(Lk, mask, k, B):
    """kv_len per batch row of a padded case: B in a row of Lk, 0, 1, Lk - 1,
    the start moving on with every case and once more with every edge (the
    pairs of an edge come four at a time: the same pair shape of the next
    edge starts elsewhere)."""
    if "pad" not in mask:
        return None
    base = [Lk, 0, 1, max(Lk - 1, 1)]
    r = (k + k // 4) % 4
    return tuple((base[r:] + base[:r])[:B])


MASKS = ("none", "pad", "causal", "pad+causal")


def _pairs():
    out = []
    for L in EDGES:
        for other in (128, 1):
            for pt in ((L, other), (other, L)):
                if pt not in out:
                    out.append(pt)
    return out


def table(op, mask):
    """The cases of one form (op: bwd | fdo) under one mask."""
    out = []
    k = MASKS.index(mask)  # (the family and kv_len turns start elsewhere per mask)

    def add(Lq, Lk, B=2, H=2, kv="auto"):
        nonlocal k
        kvt = _kv(Lk, mask, k, B) if kv == "auto" else kv
        out.append(A.Case(op, FAMS[k % len(FAMS)], 64, Lq, Lk, mask, kvt, A.LAYOUTS[(k // 2 + k // 3) % 2], B, H,
                          seed=100 + k))
        k += 1

    for (Lq, Lk) in _pairs():
        add(Lq, Lk)
    if "causal" in mask:
        for L in EDGES[1:-1]:  # (the squares at 1 and 128 are among the pairs)
            add(L, L)
    if mask == "pad":
        add(128, 128, kv=(0, 128))               # a batch row with no valid key
        add(64, 64, kv=(33, 64))                 # the key window ends mid-band
        add(128, 128, B=3, H=1, kv=(128, 33, 0))  # B H odd
    if mask == "pad+causal":
        add(33, 64, kv=(33, 33))
        add(33, 33, B=3, H=1, kv=(33, 17, 1))
    if mask == "none":
        add(65, 33, B=3, H=1)
    return tuple(out)
