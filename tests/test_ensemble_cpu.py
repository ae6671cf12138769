"""Ensemble decoding on the CPU f32 path: the combine step against the float64
reference of ref_ensemble.py, an ensemble against its members in beam search
and sampling, the validation of `Ensemble` and the multi-prefix `test` CLI."""
import os

import pytest
import torch

import ref_ensemble as re_
from tensorflow_distributed_on_gke_amd.__main__ import main
from tensorflow_distributed_on_gke_amd.checkpoint import bundle
from tensorflow_distributed_on_gke_amd.config import load_settings
from tensorflow_distributed_on_gke_amd.infer.beam import beam_search
from tensorflow_distributed_on_gke_amd.infer.ensemble import Ensemble
from tensorflow_distributed_on_gke_amd.infer.greedy import Tester
from tensorflow_distributed_on_gke_amd.infer.sample import sample_search
from tensorflow_distributed_on_gke_amd.infer.tokenizer import END, START, ByteTokenizer
from tensorflow_distributed_on_gke_amd.models.transformer import Transformer, model_config
from tensorflow_distributed_on_gke_amd.ops import kernels as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTS = ["muitas pessoas vieram à estação.", "olá", "este é um teste mais longo"]
V = 300
MAXLEN = 12
SAMPLE = dict(n=3, temperature=0.8, top_k=40, top_p=0.9, seed=1)


# ---------------------------------------------------------------- the combine step
@pytest.mark.parametrize("R", re_.ROWS)
@pytest.mark.parametrize("M", re_.MEMBERS)
@pytest.mark.parametrize("V,ldo", re_.SHAPES)
def test_ensemble_logprobs(V, ldo, M, R):
    for kind in re_.KINDS:
        logits, weights, ref = re_.case(V, ldo, M, R, kind)
        out = K.ensemble_logprobs(list(logits), V, weights)
        assert out.dtype == torch.float32 and out.shape == (R, (V + 7) // 8 * 8)
        err = re_.check_against(out, ref, re_.f32_bound, kind)
        # the probabilities sum to 1 on a row alive in every member (to the
        # weight of the members alive in it where one has no finite logit)
        mass = re_.live_mass(logits, V, weights)
        live = mass > 0
        total = torch.exp(out[:, :V].double()).sum(dim=1)
        print(f"{kind}: max err {err:.3e}, max |sum p - mass| {float((total - mass).abs().max()):.3e}")
        assert bool((mass == 1.0).any()) or (kind == "masked" and R == 1 and M > 1)
        assert ((total - mass).abs() <= 1e-5).all(), kind
        if M == 1:
            x = logits[0][:, :V]
            x = torch.where(x > re_.NINF, x, torch.full_like(x, re_.NINF))
            lsm = torch.log_softmax(x[live], dim=1)
            assert torch.allclose(out[:, :V][live], lsm, rtol=0, atol=1e-5), kind
        into = torch.full((R, ldo), 7.0)
        assert K.ensemble_logprobs(list(logits), V, weights, out=into) is into
        assert torch.equal(into[:, :V], out[:, :V]) and (into[:, V:] == re_.NINF).all()


def test_ensemble_logprobs_rejects():
    x = torch.zeros(2, 8)
    for bad in (dict(logits_list=[]), dict(logits_list=[x] * 9), dict(V=0), dict(V=65537),
                dict(weights=[1.0]), dict(weights=[1.0, 0.0]), dict(weights=[1.0, float("nan")])):
        kw = dict(dict(logits_list=[x, x], V=7, weights=None), **bad)
        with pytest.raises(RuntimeError):
            K.ensemble_logprobs(**kw)


# ---------------------------------------------------------------- decoding
@pytest.fixture(scope="module")
def setup():
    cfg = model_config("tiny", src_vocab=V, tgt_vocab=V)
    m4 = Transformer(cfg).build("cpu", seed=4)
    m5 = Transformer(cfg).build("cpu", seed=5)
    tok = ByteTokenizer(V)
    return m4, m5, tok, tok.tokenize(SENTS)


def test_two_copies_reproduce_the_model(setup):
    m, _, _, src = setup
    one = beam_search(m, src, START, END, beam=4, max_length=MAXLEN)
    two = beam_search(Ensemble([m, m]), src, START, END, beam=4, max_length=MAXLEN)
    assert torch.equal(one[2], two[2]), "beam 4: [m, m] decodes other tokens than m"
    err = (one[3] - two[3]).abs().max().item()
    print(f"beam: max score difference {err:.3e}")
    assert torch.isfinite(one[3]).all() and err <= 1e-4
    s1 = sample_search(m, src, START, END, max_length=MAXLEN, **SAMPLE)
    s2 = sample_search(Ensemble([m, m]), src, START, END, max_length=MAXLEN, **SAMPLE)
    assert torch.equal(s1[0], s2[0]), "sampling: [m, m] draws other tokens than m"
    print(f"sample: max score difference {(s1[1] - s2[1]).abs().max().item():.3e}")


def test_two_models(setup):
    m4, m5, tok, src = setup
    a4 = beam_search(m4, src, START, END, beam=4, max_length=MAXLEN)
    a5 = beam_search(m5, src, START, END, beam=4, max_length=MAXLEN)
    assert a4[0].shape != a5[0].shape or not torch.equal(a4[0], a5[0]), "the members must differ"
    ens = Ensemble([m4, m5])
    tokens, scores, all_tokens, all_scores = beam_search(ens, src, START, END, beam=4, max_length=MAXLEN)
    assert torch.isfinite(scores).all()
    forced = Tester(tok, ens).score(src, tokens)
    print(f"beam score vs teacher-forced: {(scores - forced).abs().max().item():.3e}")
    assert ((scores - forced).abs() <= 1e-3).all()
    # neither member alone gives the mixture's score
    assert ((Tester(tok, m4).score(src, tokens) - forced).abs() > 1e-3).any()
    swapped = beam_search(Ensemble([m5, m4]), src, START, END, beam=4, max_length=MAXLEN)
    assert torch.equal(swapped[2], all_tokens) and torch.equal(swapped[0], tokens)
    copy = beam_search(ens, src, START, END, beam=4, max_length=MAXLEN, reorder="copy")
    assert torch.equal(copy[2], all_tokens) and torch.equal(copy[3], all_scores)


def test_unequal_weights_lean_to_the_heavy_member(setup):
    m4, m5, tok, src = setup
    ens = Ensemble([m4, m5], weights=[999.0, 1.0])
    assert abs(sum(ens.weights) - 1.0) < 1e-12 and abs(ens.weights[0] - 0.999) < 1e-12
    tokens = beam_search(m4, src, START, END, beam=4, max_length=MAXLEN)[0]
    lo, hi = Tester(tok, m4).score(src, tokens), Tester(tok, ens).score(src, tokens)
    even = Tester(tok, Ensemble([m4, m5])).score(src, tokens)
    assert ((hi - lo).abs() < (even - lo).abs()).all()


def test_one_member_is_the_model_bitwise(setup):
    m4, _, tok, src = setup
    for x, y in zip(beam_search(m4, src, START, END, beam=4, max_length=MAXLEN),
                    beam_search(Ensemble([m4]), src, START, END, beam=4, max_length=MAXLEN)):
        assert torch.equal(x, y)
    for x, y in zip(sample_search(m4, src, START, END, max_length=MAXLEN, **SAMPLE),
                    sample_search(Ensemble([m4]), src, START, END, max_length=MAXLEN, **SAMPLE)):
        assert torch.equal(x, y)
    tokens = beam_search(m4, src, START, END, beam=4, max_length=MAXLEN)[0]
    assert torch.equal(Tester(tok, Ensemble([m4])).score(src, tokens), Tester(tok, m4).score(src, tokens))


def test_sample_steps_carry_the_member_logits(setup):
    m4, m5, _, src = setup
    tokens, scores, steps = sample_search(Ensemble([m4, m5]), src, START, END, max_length=4,
                                          return_steps=True, **SAMPLE)
    assert len(steps) == tokens.shape[2] - 1
    for combined, token, fin, member_logits in steps:
        assert len(member_logits) == 2 and token.shape == fin.shape == (9,)
        ref = re_.ensemble_ref(member_logits, V)
        re_.check_against(combined, ref, re_.f32_bound, "step")


def test_tester_modes(setup):
    m4, m5, tok, src = setup
    ens = Ensemble([m4, m5])
    t = Tester(tok, ens)
    greedy, gs = t.decode(src, max_length=MAXLEN)
    b1 = beam_search(ens, src, START, END, beam=1, max_length=MAXLEN, alpha=0.0)
    assert torch.equal(greedy[:, 0], b1[0]) and torch.equal(gs[:, 0], b1[1])
    beam, bs = t.decode(src, max_length=MAXLEN, beam=3)
    assert beam.shape[:2] == (3, 1) and torch.isfinite(bs).all()
    drawn, ds = t.decode(src, max_length=MAXLEN, sample=2, top_k=20, seed=3)
    assert drawn.shape[:2] == (3, 2) and torch.isfinite(ds).all()
    texts, names, attn = t(SENTS, max_length=MAXLEN, beam=2)
    assert len(texts) == 3 and all(isinstance(x, str) for x in texts)
    first = Tester(tok, m4).attention_weights(src, beam[:, 0, :-1])
    got = t.attention_weights(src, beam[:, 0, :-1])
    assert set(got) == set(first) and all(torch.equal(got[k], first[k]) for k in got)
    lines = t.translate_lines(SENTS, batch=2, max_length=MAXLEN)
    assert [len(h) for h in lines] == [1, 1, 1]


# ---------------------------------------------------------------- validation
def test_validation(setup):
    m4, m5, tok, src = setup
    other = Transformer(model_config("tiny", src_vocab=V, tgt_vocab=V + 1)).build("cpu", seed=1)
    for models, weights in (([], None), ([m4] * 9, None), ([m4, other], None), ([m4, m5], [1.0, 0.0]),
                            ([m4, m5], [1.0, -2.0]), ([m4, m5], [1.0]), ([m4, m5], [1.0, float("nan")])):
        with pytest.raises(ValueError):
            Ensemble(models, weights)
    t = Tester(tok, Ensemble([m4, m5]))
    with pytest.raises(ValueError):
        t.decode(src, max_length=MAXLEN, kv_cache=False)
    with pytest.raises(ValueError):
        t(SENTS[0], max_length=MAXLEN, kv_cache=False)
    assert len(Ensemble([m4] * 8)) == 8


# ---------------------------------------------------------------- CLI
TEST_SETS = ["preset=tiny", "src_vocab=300", "tgt_vocab=300", "max_len=64"]


def _cli(*args):
    argv = ["test", "--config", os.path.join(ROOT, "configuration", "settings.yaml"), "--device", "cpu",
            "--max-length", "6"]
    for kv in TEST_SETS:
        argv += ["--set", kv]
    return main(argv + list(args))


@pytest.fixture(scope="module")
def bundles(tmp_path_factory):
    from tensorflow_distributed_on_gke_amd.train.loop import build_model

    d = tmp_path_factory.mktemp("ens")
    m = build_model(load_settings(overrides=TEST_SETS), "cpu")
    a, b = str(d / "a" / "model_weights"), str(d / "b" / "model_weights")
    bundle.save_weights(m.store, a)
    g = torch.Generator().manual_seed(0)
    m.store.flat.add_(torch.randn(m.store.flat.shape, generator=g) * 0.05)
    bundle.save_weights(m.store, b)
    return a, b


def test_cli_file_mode(bundles, tmp_path, capsys):
    a, b = bundles
    src, out = tmp_path / "in.txt", tmp_path / "out.txt"
    lines = ["olá", "este é um teste", "muitas pessoas"]
    src.write_text("\n".join(lines) + "\n", encoding="utf-8")
    assert _cli("--weights", a, b, "--input", str(src), "--output", str(out), "--beam", "2") == 0
    rows = out.read_text(encoding="utf-8").splitlines()
    assert len(rows) == len(lines)
    for line, row in zip(lines, rows):
        s, hyp, score = row.split("\t")
        assert s == line and float(score) <= 0.0
    # unequal weights, sampling and sentence mode run too
    assert _cli("--weights", a, b, "--ensemble-weights", "3", "1", "--sentence", "olá", "--sample", "2") == 0
    assert _cli("--weights", a, b, "--sentence", "olá") == 0
    assert "->" in capsys.readouterr().out


def test_cli_loads_every_prefix(bundles, monkeypatch):
    a, b = bundles
    loaded = []
    real = bundle.load_weights

    def spy(store, p, *x, **kw):
        loaded.append(p)
        return real(store, p, *x, **kw)

    monkeypatch.setattr(bundle, "load_weights", spy)
    assert _cli("--weights", a, b, "--sentence", "olá", "--beam", "2") == 0
    assert loaded == [a, b]


def test_cli_rejects_bad_ensemble_weights(bundles):
    a, b = bundles
    for extra in (["--ensemble-weights", "1"], ["--ensemble-weights", "1", "0"],
                  ["--ensemble-weights", "1", "-1"]):
        with pytest.raises(SystemExit) as e:
            _cli("--weights", a, b, "--sentence", "olá", *extra)
        assert e.value.code != 0
