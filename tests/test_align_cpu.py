"""Word alignment on the CPU f32 path: the CPU arm of attn_align against the
float64 reference, `align_pairs` and `Tester.align_pairs` on a tiny random
model, the projection to words, and the `align` / `test --align` commands."""
import os
import re

import pytest
import torch

import ref_align as RA
from tensorflow_distributed_on_gke_amd.__main__ import main
from tensorflow_distributed_on_gke_amd.checkpoint import bundle
from tensorflow_distributed_on_gke_amd.config import load_settings
from tensorflow_distributed_on_gke_amd.infer import align as AL
from tensorflow_distributed_on_gke_amd.infer.greedy import Tester
from tensorflow_distributed_on_gke_amd.infer.tokenizer import END, OFFSET, ByteTokenizer, word_ids
from tensorflow_distributed_on_gke_amd.models.layers import RunCtx
from tensorflow_distributed_on_gke_amd.models.transformer import Transformer, model_config
from tensorflow_distributed_on_gke_amd.ops.kernels import attention as KA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 300
SOURCES = ["muitas pessoas vieram", "olá", "este é um teste mais longo"]
TARGETS = ["many people came", "hello", "this is a longer test"]


@pytest.fixture(scope="module")
def setup():
    cfg = model_config("tiny", src_vocab=V, tgt_vocab=V, max_src_len=40, max_tgt_len=40, layers=3)
    return Transformer(cfg).build("cpu", seed=4), ByteTokenizer(V)


@pytest.mark.parametrize("hd,H,Lq,Lk,with_qlen", [(16, 5, 17, 15, True), (64, 8, 40, 130, False)])
def test_cpu_arm_against_float64(hd, H, Lq, Lk, with_qlen):
    gen = torch.Generator().manual_seed(Lk)
    q, k = (RA.bf(torch.randn(4, L, H, hd, generator=gen)) for L in (Lq, Lk))
    kv_len = torch.tensor([Lk, 1, 2, Lk // 2], dtype=torch.int32)
    q_len = torch.tensor([Lq, 0, 1, Lq // 2], dtype=torch.int32) if with_qlen else None
    got = KA.attn_align(q, k, kv_len, hd ** -0.5, q_len, 1, 1, want_soft=True)
    RA.check(got, RA.reference(q, k, kv_len, hd ** -0.5, q_len, 1, 1), kv_len, q_len, f"cpu hd{hd}")
    with pytest.raises(ValueError):
        KA.attn_align(q, torch.zeros(4, KA.ALIGN_MAX_LK + 1, H, hd), kv_len, 1.0)


def test_align_pairs_ranges_and_default_layer(setup):
    m, tok = setup
    src, tgt = tok.tokenize(SOURCES), tok.tokenize(TARGETS)
    links, soft = AL.align_pairs(m, src, tgt, want_soft=True)
    assert links == AL.align_pairs(m, src, tgt, layer=m.cfg.layers - 1) != AL.align_pairs(m, src, tgt, layer=1)
    for s, t, ls, sf in zip(SOURCES, TARGETS, links, soft):
        ns, nt = len(s.encode()), len(t.encode())  # the real tokens: no [START], no [END]
        assert [x[0] for x in ls] == list(range(nt)) and sf.shape == (nt, ns)
        assert all(0 <= j < ns and c == float(sf[i, j]) == float(sf[i].max()) for i, j, c in ls)
    with pytest.raises(ValueError):
        AL.align_pairs(m, src, tgt, layer=m.cfg.layers + 1)


def test_empty_target_and_truncated_pair(setup):
    m, tok = setup
    t = Tester(tok, m)
    long = "palavra " * 10  # 80 bytes: both sides cut to the 40-position tables
    out = t.align_pairs(["olá", long, "sim"], ["", long, "yes"], words=False)
    assert out[0] == [] and [x[0] for x in out[2]] == [0, 1, 2]
    assert [x[0] for x in out[1]] == list(range(40)) and all(0 <= x[1] < 38 for x in out[1])
    assert AL.align_pairs(m, tok.tokenize(["olá"]), torch.full((1, 1), 2)) == [[]]


def test_word_projection():
    assert word_ids(["the", "un", "##believ", "##able", "end", "##s"]) == [0, 1, 1, 1, 2, 2]
    assert word_ids(list("ab  c"), byte_level=True) == [0, 0, -1, -1, 1]
    tgt_w, src_w = [0, 1, 1, 1, 2, 2], [0, 0, -1, 1, 2]
    links = [(0, 3, 0.5), (1, 0, 0.2), (2, 4, 0.6), (3, 1, 0.6), (4, 2, 0.9), (5, 0, 0.1)]
    # word 1: tokens 2 and 3 tie at 0.6, the first wins; word 2: its best token points at whitespace
    assert AL.project_words(links, tgt_w, src_w) == [(0, 1, 0.5), (1, 2, 0.6), (2, 0, 0.1)]
    assert AL.pharaoh([(0, 1, 0.5), (1, 2, 0.6), (2, 0, 0.1)], 0.3) == "1-0 2-1"


SETS = ["preset=tiny", "src_vocab=300", "tgt_vocab=300", "max_len=64"]


def test_cli_align_and_test_align(tmp_path, capsys):
    from tensorflow_distributed_on_gke_amd.train.loop import build_model

    m = build_model(load_settings(overrides=SETS), "cpu")
    m.final.b.master[[OFFSET + b for b in b"abcdefghij "]] += 20.0
    m.final.b.master[END] += 21.5
    prefix = str(tmp_path / "w" / "model_weights")
    bundle.save_weights(m.store, prefix)
    src, a, b, c = (str(tmp_path / n) for n in ("in.txt", "a.tsv", "b.tsv", "c.tsv"))
    with open(src, "w", encoding="utf-8") as f:
        f.write("\n".join(SOURCES) + "\n")
    base = ["--config", os.path.join(ROOT, "configuration", "settings.yaml"), "--device", "cpu"]
    for kv in SETS:
        base += ["--set", kv]
    assert main(["test"] + base + ["--weights", prefix, "--max-length", "30", "--input", src, "--output", a,
                                   "--align"]) == 0
    assert main(["align"] + base + ["--weights", prefix, "--input", a, "--output", b]) == 0
    assert main(["align"] + base + ["--weights", prefix, "--input", a, "--output", c, "--tokens",
                                    "--min-conf", "0.05"]) == 0
    rows = [[line.rstrip("\n").split("\t") for line in open(p, encoding="utf-8")] for p in (a, b, c)]
    for ra, rb, rc in zip(*rows):
        assert len(ra) == 4 and len(rb) == len(rc) == 3 and ra[:2] == rb[:2] == rc[:2]
        assert ra[3] == rb[2] and all(re.fullmatch(r"\d+-\d+", p) for p in (rb[2] + " " + rc[2]).split())
        pairs = [tuple(map(int, p.split("-"))) for p in rb[2].split()]
        assert [t for _, t in pairs] == list(range(len(ra[1].split())))  # every word, ascending
        assert all(s < len(ra[0].split()) for s, _ in pairs)
        conf = {x[0]: x[2] for x in Tester(ByteTokenizer(V), m).align_pairs([ra[0]], [ra[1]], words=False)[0]}
        assert [int(p.split("-")[1]) for p in rc[2].split()] == [t for t, cf in sorted(conf.items()) if cf >= 0.05]
    assert len(rows[0]) == len(SOURCES)


def test_no_request_leaves_logits_bitwise(setup):
    m, tok = setup
    src, tgt = tok.tokenize(SOURCES), tok.tokenize(TARGETS)[:, :-1]
    site = m.dec_layers[1].site2
    rt = RunCtx(training=False, store=None, align={site: dict(k_lo=1, k_trim=1)})
    assert torch.equal(m.logits(src, tgt, RunCtx(training=False, store=None)), m.logits(src, tgt, rt))
    assert rt.align[site][0].shape == tgt.shape
