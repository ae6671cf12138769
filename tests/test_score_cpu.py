"""Teacher-forced scoring on the CPU f32 path: `Tester.score_pairs` against
`Tester.score`, skipped pairs and batching, and the `score`, `score --rerank`
and `test --n-best` commands on a tiny model with saved weights."""
import math
import os

import pytest
import torch

from tensorflow_distributed_on_gke_amd.__main__ import main
from tensorflow_distributed_on_gke_amd.checkpoint import bundle
from tensorflow_distributed_on_gke_amd.config import load_settings
from tensorflow_distributed_on_gke_amd.infer.ensemble import Ensemble
from tensorflow_distributed_on_gke_amd.infer.greedy import Tester
from tensorflow_distributed_on_gke_amd.infer.score import score_pairs
from tensorflow_distributed_on_gke_amd.infer.tokenizer import END, OFFSET, ByteTokenizer
from tensorflow_distributed_on_gke_amd.models.transformer import PAD_ID, Transformer, model_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 300
TOL = 1e-4  # per token: both sides are f32 log-softmax values of the same logits
SOURCES = ["muitas pessoas vieram à estação.", "olá", "este é um teste mais longo", "sim", "não sei"]
TARGETS = ["many people came to the station.", "hello", "this is a longer test", "yes", "i do not know"]


@pytest.fixture(scope="module")
def setup():
    cfg = model_config("tiny", src_vocab=V, tgt_vocab=V, max_src_len=40, max_tgt_len=40)
    m4 = Transformer(cfg).build("cpu", seed=4)
    m5 = Transformer(cfg).build("cpu", seed=5)
    return m4, m5, ByteTokenizer(V)


@pytest.mark.parametrize("ensemble", (False, True))
def test_score_pairs_is_tester_score(setup, ensemble):
    m4, m5, tok = setup
    t = Tester(tok, Ensemble([m4, m5], [2.0, 1.0]) if ensemble else m4)
    got = t.score_pairs(SOURCES, TARGETS, batch=32, want_top=True)
    want = t.score(tok.tokenize(SOURCES), tok.tokenize(TARGETS))
    for (lp, n, tok_lp, top_lp), w, target in zip(got, want.tolist(), TARGETS):
        assert n == len(target.encode("utf-8")) + 1 and len(tok_lp) == len(top_lp) == n
        assert abs(lp - w) <= TOL * n, (lp, w)
        assert abs(sum(tok_lp) - lp) <= 1e-9 * n  # the f64 sum of the f32 values
        assert all(a <= b for a, b in zip(tok_lp, top_lp))


def test_tokens_after_end_and_pad_are_ignored(setup):
    m4, _, tok = setup
    src, tgt = tok.tokenize(SOURCES[:2]), tok.tokenize(TARGETS[:2])
    sc = score_pairs(m4, src, tgt, want_top=True)
    assert sc.tok_lp.shape == (2, tgt.shape[1] - 1) and sc.sent_lp.dtype == torch.float64
    ignored = tgt[:, 1:] == PAD_ID
    assert ignored.any() and (sc.tok_lp[ignored] == 0).all() and (sc.top_lp[ignored] == 0).all()
    assert torch.equal(sc.n_tok, (~ignored).sum(dim=1)) and sc.logits is None
    # a tail after [END] changes nothing before it and scores nothing itself
    tail = tgt.clone()
    n = int(sc.n_tok[1])  # the [END] of row 1 is label n - 1
    tail[1, 1 + n:] = OFFSET + 65
    sc2 = score_pairs(m4, src, tail, return_logits=True)
    assert len(sc2.logits) == 1 and sc2.top_lp is None
    assert torch.equal(sc2.n_tok, sc.n_tok) and (sc2.tok_lp[1, n:] == 0).all()
    assert torch.allclose(sc2.tok_lp, sc.tok_lp, rtol=0, atol=TOL)


def test_overlong_pairs_are_skipped(setup):
    m4, _, tok = setup
    sources = [SOURCES[0], "s" * 39, SOURCES[1], SOURCES[2]]  # 39 bytes + [START] [END] = 41 > 40
    targets = [TARGETS[0], TARGETS[1], "t" * 40, TARGETS[2]]  # 42 tokens: 41 positions > 40
    got = Tester(tok, m4).score_pairs(sources, targets, batch=2)
    assert [g[1] for g in got] == [len(TARGETS[0]) + 1, 0, 0, len(TARGETS[2]) + 1]
    assert all(math.isnan(got[i][0]) and got[i][2] == [] for i in (1, 2))
    assert all(math.isfinite(got[i][0]) for i in (0, 3))
    # the longest that still fits is scored
    fits = Tester(tok, m4).score_pairs(["s" * 38], ["t" * 39])
    assert fits[0][1] == 40 and math.isfinite(fits[0][0])


def test_input_order_is_kept_across_batches(setup):
    m4, _, tok = setup
    t = Tester(tok, m4)
    alone = [t.score_pairs([s], [h])[0] for s, h in zip(SOURCES, TARGETS)]
    assert len({round(a[0], 3) for a in alone}) == len(alone), "the pairs must differ in score"
    for batch in (1, 2, 32):
        got = t.score_pairs(SOURCES, TARGETS, batch=batch)
        back = t.score_pairs(SOURCES[::-1], TARGETS[::-1], batch=batch)[::-1]
        for a, g, b in zip(alone, got, back):
            assert g[1] == a[1] == b[1]
            assert abs(g[0] - a[0]) <= TOL * a[1] and abs(b[0] - a[0]) <= TOL * a[1]
    with pytest.raises(ValueError):
        t.score_pairs(SOURCES, TARGETS[:-1])


def test_decode_n_best(setup):
    m4, _, tok = setup
    t = Tester(tok, m4)
    src = tok.tokenize(SOURCES[:3])
    one, s1 = t.decode(src, max_length=8, beam=3)
    many, sn = t.decode(src, max_length=8, beam=3, n_best=True)
    assert many.shape[:2] == (3, 3) and sn.shape == (3, 3)
    assert torch.equal(many[:, 0], one[:, 0]) and torch.equal(sn[:, :1], s1)
    flat, sf = t.decode(src, max_length=8, beam=3, alpha=0.0, n_best=True)
    assert (sf[:, :-1] >= sf[:, 1:]).all()  # alpha 0: the ranking score is the score
    with pytest.raises(ValueError):
        t.decode(src, max_length=8, n_best=True)


# ---------------------------------------------------------------- CLI
SETS = ["preset=tiny", "src_vocab=300", "tgt_vocab=300", "max_len=64"]
LINES = ["olá", "este é um teste", "muitas pessoas"]


def _cli(cmd, *args):
    argv = [cmd, "--config", os.path.join(ROOT, "configuration", "settings.yaml"), "--device", "cpu"]
    for kv in SETS:
        argv += ["--set", kv]
    return main(argv + list(args))


@pytest.fixture(scope="module")
def weights(tmp_path_factory):
    """A tiny model whose output bias favours lower-case letters, the space
    and [END]: what it generates is text that survives detokenising and
    tokenising again, and it ends."""
    from tensorflow_distributed_on_gke_amd.train.loop import build_model

    m = build_model(load_settings(overrides=SETS), "cpu")
    keep = [OFFSET + b for b in b"abcdefghijklmnopqrstuvwxyz"]
    m.final.b.master[keep] += 20.0
    m.final.b.master[END] += 22.5
    prefix = str(tmp_path_factory.mktemp("score") / "w" / "model_weights")
    bundle.save_weights(m.store, prefix)
    return prefix


@pytest.fixture(scope="module")
def source_file(tmp_path_factory):
    p = tmp_path_factory.mktemp("in") / "in.txt"
    p.write_text("\n".join(LINES) + "\n", encoding="utf-8")
    return str(p)


def _rows(path):
    with open(path, encoding="utf-8") as f:
        return [line.rstrip("\n").split("\t") for line in f]


def _ntok(hyp):
    return len(hyp.encode("utf-8")) + 1


def test_cli_sample_then_score(weights, source_file, tmp_path, capsys):
    a, b = str(tmp_path / "a.tsv"), str(tmp_path / "b.tsv")
    assert _cli("test", "--weights", weights, "--sample", "3", "--max-length", "40", "--input", source_file,
                "--output", a) == 0
    capsys.readouterr()
    assert _cli("score", "--weights", weights, "--input", a, "--output", b, "--tokens", "--accuracy",
                "--batch", "4") == 0
    summary = capsys.readouterr().out
    ra, rb = _rows(a), _rows(b)
    assert len(ra) == len(rb) == 3 * len(LINES)
    total, tokens = 0.0, 0
    for x, y in zip(ra, rb):
        assert y[:2] == x[:2] and len(y) == 5
        n = int(y[3])
        assert n == _ntok(x[1]) and len(y[4].split()) == n
        assert abs(float(y[2]) - float(x[2])) <= TOL * n + 1e-6, (x, y)  # 6 decimals each
        assert abs(sum(float(v) for v in y[4].split()) - float(y[2])) <= 1e-6 * n + 1e-6
        total += float(y[2])
        tokens += n
    assert f"{len(ra)} pairs (0 skipped), {tokens} tokens" in summary
    ppl = float(summary.split("perplexity ")[1].split(",")[0].split()[0])
    assert abs(ppl - math.exp(-total / tokens)) <= 1e-4 * ppl
    acc = float(summary.split("accuracy ")[1].split()[0])
    assert 0.0 <= acc <= 1.0


def test_cli_n_best_and_rerank(weights, source_file, tmp_path, capsys):
    one, many, flat = (str(tmp_path / n) for n in ("one.tsv", "many.tsv", "flat.tsv"))
    base = ["--weights", weights, "--beam", "3", "--max-length", "12", "--input", source_file, "--output"]
    assert _cli("test", *base, one) == 0
    assert _cli("test", *base, many, "--n-best") == 0
    assert _cli("test", *base, flat, "--n-best", "--length-penalty", "0") == 0
    r1, rn, rf = _rows(one), _rows(many), _rows(flat)
    assert len(r1) == len(LINES) and len(rn) == len(rf) == 3 * len(LINES)
    assert rn[::3] == r1, "without --n-best: the first of every group"
    for g in range(len(LINES)):
        group = rf[3 * g:3 * g + 3]
        assert all(r[0] == LINES[g] for r in group) and len({r[1] for r in group}) == 3
        scores = [float(r[2]) for r in group]
        assert scores == sorted(scores, reverse=True)
    # rescoring and reranking that list
    scored, best = str(tmp_path / "scored.tsv"), str(tmp_path / "best.tsv")
    assert _cli("score", "--weights", weights, "--input", flat, "--output", scored) == 0
    assert _cli("score", "--weights", weights, "--input", flat, "--output", best, "--rerank",
                "--length-penalty", "0") == 0
    rs_, rb = _rows(scored), _rows(best)
    assert len(rs_) == len(rf) and len(rb) == len(LINES)
    for g in range(len(LINES)):
        group = rs_[3 * g:3 * g + 3]
        top = max(group, key=lambda r: float(r[2]))
        assert rb[g][:2] == top[:2] and float(rb[g][2]) == float(top[2])
    # the model's own score of a hypothesis breaks the tie the other way with --mix
    mixed = str(tmp_path / "mixed.tsv")
    assert _cli("score", "--weights", weights, "--input", flat, "--output", mixed, "--rerank",
                "--length-penalty", "0", "--mix", "-2") == 0
    rm = _rows(mixed)
    for g in range(len(LINES)):
        keys = [float(s[2]) - 2.0 * float(f[2]) for s, f in zip(rs_[3 * g:3 * g + 3], rf[3 * g:3 * g + 3])]
        k = max(range(3), key=lambda i: keys[i])
        assert rm[g][1] == rf[3 * g + k][1] and abs(float(rm[g][2]) - keys[k]) <= 1e-5
    capsys.readouterr()


def test_cli_rerank_skips_unscored_pairs(weights, tmp_path, capsys):
    src = str(tmp_path / "in.tsv")
    with open(src, "w", encoding="utf-8") as f:
        f.write("olá\t" + "x" * 70 + "\nolá\thello\nsim\t" + "y" * 70 + "\n")
    out = str(tmp_path / "out.tsv")
    assert _cli("score", "--weights", weights, "--input", src, "--output", out, "--rerank") == 0
    assert "3 pairs (2 skipped)" in capsys.readouterr().out
    rows = _rows(out)
    assert [r[:2] for r in rows] == [["olá", "hello"], ["sim", "y" * 70]] and rows[1][2] == "nan"
    assert _cli("score", "--weights", weights, "--input", src, "--output", out) == 0
    rows = _rows(out)
    assert [r[2:] for r in rows][0] == ["nan", "0"] and int(rows[1][3]) == 6


def test_cli_argument_errors(weights, source_file, tmp_path):
    out = str(tmp_path / "o.tsv")
    pairs = str(tmp_path / "pairs.tsv")
    with open(pairs, "w", encoding="utf-8") as f:
        f.write("olá\thello\n")
    for argv in (["test", "--weights", weights, "--n-best", "--input", source_file, "--output", out],
                 ["test", "--weights", weights, "--n-best", "--beam", "3", "--sentence", "olá"],
                 ["score", "--weights", weights, "--input", pairs, "--output", out, "--rerank", "--mix", "1"],
                 ["score", "--weights", weights, "--input", pairs],
                 ["score", "--weights", weights, "--input", source_file, "--output", out],
                 ["score", "--weights", weights, "--input", pairs, "--output", out, "--mix", "1"]):
        with pytest.raises(SystemExit) as e:
            _cli(*argv)
        assert e.value.code != 0, argv
    assert not os.path.exists(out)
