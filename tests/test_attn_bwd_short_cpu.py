"""On the CPU: ref_attn's plain float32 evaluation with the design's bf16
roundings (attn_f32) of every case of tests/test_gpu_attn_bwd_short.py passes
ref_attn.check, i.e. the float64 references and the tolerance table hold for
the band-edge shapes, the non-square causal windows and the kv_len rows those
tables add, before any kernel is involved; and the tables hold what the GPU
module's docstring says."""
import pytest

import attn_bwd_short_cases as T
import ref_attn as A


@pytest.mark.parametrize("mask", T.MASKS)
@pytest.mark.parametrize("op", T.FORMS)
def test_reference_inside_tolerance(op, mask):
    for c in T.table(op, mask):
        bt = A.build(c)
        A.check(bt, A.attn_f32(bt))


def test_tables_cover_every_pair_under_every_mask():
    for op in T.FORMS:
        for mask in T.MASKS:
            tab = T.table(op, mask)
            pts = {(c.Lq, c.Lk) for c in tab if (c.B, c.H) == (2, 2)}
            for L in T.EDGES:
                for other in (128, 1):
                    assert (L, other) in pts and (other, L) in pts, (op, mask, L, other)
            assert all(c.mask == mask and c.hd == 64 and c.arm.family == ("bwd_fused", "bwd_fdo")[op == "fdo"]
                       for c in tab)
            if "pad" in mask:
                lens = {(n, c.Lk) for c in tab for n in c.kv}
                assert {(0, 128), (1, 128), (127, 128), (128, 128)} <= lens, (op, mask)
        pad = T.table(op, "pad")
        assert any(c.kv == (0, 128) for c in pad) and any(c.kv == (33, 64) and c.Lk == 64 for c in pad)
        assert any(c.B * c.H % 2 == 1 for c in pad)
