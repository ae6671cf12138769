"""Sampled decoding (infer/sample.py) on the CPU f32 path: against greedy and
beam-1 decoding, every step replayed through the float64 reference, the
Tester interface and the command line, file mode included."""
import pytest
import torch

import ref_sample as rs
from tensorflow_distributed_on_gke_amd.__main__ import main
from tensorflow_distributed_on_gke_amd.infer.beam import beam_search
from tensorflow_distributed_on_gke_amd.infer.greedy import Tester
from tensorflow_distributed_on_gke_amd.infer.sample import sample_search
from tensorflow_distributed_on_gke_amd.infer.tokenizer import END, START, ByteTokenizer
from tensorflow_distributed_on_gke_amd.models.transformer import PAD_ID, Transformer, model_config

SENTS = ["muitas pessoas vieram à estação.", "olá", "este é um teste mais longo"]
V = 300
MAXLEN = 12
SEED = 23  # the model seed of test_beam_cpu.py; in f32 no two logits tie at a row maximum
OPTS = dict(temperature=0.9, top_k=50, top_p=0.95)


@pytest.fixture(scope="module")
def setup():
    m = Transformer(model_config("tiny", src_vocab=V, tgt_vocab=V)).build("cpu", seed=SEED)
    tester = Tester(ByteTokenizer(V), m)
    return m, tester, tester.src_tok.tokenize(SENTS)


def test_top_k_1_is_greedy(setup):
    m, tester, src = setup
    greedy = tester.greedy_cached(src, max_length=MAXLEN)
    beam1 = beam_search(m, src, START, END, beam=1, max_length=MAXLEN, alpha=0.0)
    tokens, scores, steps = sample_search(m, src, START, END, n=2, max_length=MAXLEN, top_k=1, seed=9,
                                          return_steps=True)
    for lg, _, _ in steps:  # the premise: the row maximum is unique
        top2 = lg[:, :V].topk(2, dim=1).values
        assert (top2[:, 0] > top2[:, 1]).all(), "a tie at the maximum: pick another model seed"
    assert tokens.dtype == torch.int64 and tokens.shape == (3, 2, greedy.shape[1])
    for k in range(2):
        assert torch.equal(tokens[:, k], greedy) and torch.equal(tokens[:, k], beam1[0])
        assert torch.allclose(scores[:, k], beam1[1], rtol=0, atol=1e-4)


def test_steps_replay_through_reference(setup):
    m, _, src = setup
    tokens, scores, steps = sample_search(m, src, START, END, n=3, max_length=MAXLEN, seed=11,
                                          return_steps=True, **OPTS)
    assert tokens.shape[:2] == (3, 3) and scores.shape == (3, 3) and scores.dtype == torch.float32
    share = rs.check_steps(tokens, scores, steps, V, 3, 11, 0, OPTS, MAXLEN)
    print(f"decided rows over the run: {share:.3%}")
    assert share >= 0.9
    again = sample_search(m, src, START, END, n=3, max_length=MAXLEN, seed=11, **OPTS)
    assert torch.equal(again[0], tokens) and torch.equal(again[1], scores)
    other = sample_search(m, src, START, END, n=3, max_length=MAXLEN, seed=12, **OPTS)
    assert other[0].shape != tokens.shape or not torch.equal(other[0], tokens)
    # samples of one sentence differ from each other
    assert not torch.equal(tokens[0, 0], tokens[0, 1])


def test_row_identity(setup):
    m, _, src = setup
    b = int((src != PAD_ID).sum(dim=1).argmax())  # as long alone as in the batch
    t3, s3 = sample_search(m, src, START, END, n=3, max_length=MAXLEN, seed=5, **OPTS)
    t1, s1 = sample_search(m, src[b:b + 1], START, END, n=3, max_length=MAXLEN, seed=5, row_id0=b * 3,
                           **OPTS)
    n1 = min(t3.shape[2], t1.shape[2])
    assert torch.equal(t3[b, :, :n1], t1[0, :, :n1]) and (t3[b, :, n1:] == PAD_ID).all()
    assert torch.allclose(s3[b], s1[0], rtol=0, atol=1e-4)
    # one base per sentence is the same stream
    t3b, _ = sample_search(m, src, START, END, n=3, max_length=MAXLEN, seed=5, row_id0=[0, 3, 6], **OPTS)
    assert torch.equal(t3b, t3)
    with pytest.raises(ValueError):
        sample_search(m, src, START, END, n=3, max_length=MAXLEN, row_id0=[0, 3])
    with pytest.raises(ValueError):
        sample_search(m, src, START, END, n=1, max_length=m.cfg.max_tgt_len)


def test_tester_call_sample(setup):
    _, tester, _ = setup
    text, tokens, attn = tester(SENTS[0], max_length=8, sample=2, top_k=10, seed=1)
    assert isinstance(text, list) and len(text) == 2 and all(isinstance(t, str) for t in text)
    assert len(tokens) == 2 and all(t[0] == "[START]" and len(t) <= 9 for t in tokens)
    assert set(attn) == {f"decoder_layer{i}_block{j}" for i in (1, 2) for j in (1, 2)}
    assert attn["decoder_layer1_block1"].shape[0] == 1  # the first sample's maps
    texts, toks, attn3 = tester(SENTS, max_length=8, sample=2, top_k=10, seed=1)
    assert len(texts) == 3 and all(len(t) == 2 for t in texts) and len(toks) == 3
    assert attn3["decoder_layer2_block2"].shape[0] == 3
    assert texts[0] == text  # sentence 0 is the longest: the same rows, the same stream
    with pytest.raises(ValueError):
        tester(SENTS[0], max_length=8, beam=3, sample=2)
    # sample = 0 is the call without the argument
    t0, k0, _ = tester(SENTS[0], max_length=8)
    t1, k1, _ = tester(SENTS[0], max_length=8, sample=0, top_k=10)
    assert t0 == t1 and k0 == k1


TINY = ["--device", "cpu", "--config", "none.yaml", "--set", "preset=tiny", "--set", f"src_vocab={V}",
        "--set", f"tgt_vocab={V}", "--max-length", "8"]


def test_cli_sample(capsys):
    draw = ["--sample", "2", "--top-k", "10", "--seed", "1"]
    assert main(["test"] + TINY + ["--sentence", "olá"] + draw) == 0
    out = capsys.readouterr().out
    assert out.count("'olá' -> ") == 2 and "attention maps" in out
    with pytest.raises(SystemExit):
        main(["test"] + TINY + ["--sentence", "olá", "--sample", "2", "--beam", "3"])


def _read(path):
    rows = [line.rstrip("\n").split("\t") for line in open(path, encoding="utf-8")]
    assert all(len(r) == 3 for r in rows)
    return rows


def test_cli_file_mode(tmp_path, setup):
    lines = ["este é um teste mais longo", "olá", "muitas pessoas vieram à estação.", "sim", "olá"]
    src_file, out = tmp_path / "src.txt", tmp_path / "out.tsv"
    src_file.write_text("\n".join(lines) + "\n", encoding="utf-8")
    io = ["--input", str(src_file), "--output", str(out)]
    # sample mode: `sample` lines per source, input order, whatever the batching
    assert main(["test"] + TINY + io + ["--sample", "2", "--top-k", "10", "--seed", "1", "--batch", "2"]) == 0
    rows = _read(out)
    assert [r[0] for r in rows] == [s for s in lines for _ in range(2)]
    assert all(float(r[2]) < 0 for r in rows)
    assert rows[2:4] != rows[8:10], "equal lines draw from different streams"
    assert main(["test"] + TINY + io + ["--sample", "2", "--top-k", "10", "--seed", "1", "--batch", "1"]) == 0
    one = _read(out)
    # line 2 is the longest: alone in its batch it is padded as in a batch of two
    assert one[4:6] == rows[4:6]
    # greedy and beam: one line per source, the hypotheses of the sentence-list call
    assert main(["test"] + TINY + io) == 0
    greedy = _read(out)
    assert [r[0] for r in greedy] == lines
    from tensorflow_distributed_on_gke_amd.config import load_settings
    from tensorflow_distributed_on_gke_amd.train.loop import build_model
    settings = load_settings(None, ["preset=tiny", f"src_vocab={V}", f"tgt_vocab={V}"])
    tester = Tester(ByteTokenizer(V), build_model(settings, "cpu"))
    flat = lambda t: t.replace("\t", " ").replace("\n", " ").replace("\r", " ")
    assert [r[1] for r in greedy] == [flat(t) for t in tester(lines, max_length=8)[0]]
    assert greedy[1] == greedy[4] and all(float(r[2]) < 0 for r in greedy)
    assert main(["test"] + TINY + io + ["--beam", "3"]) == 0
    beam = _read(out)
    assert [r[0] for r in beam] == lines and all(float(r[2]) < 0 for r in beam)
    with pytest.raises(SystemExit):
        main(["test"] + TINY + ["--input", str(src_file)])
