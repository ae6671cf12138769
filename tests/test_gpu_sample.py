"""The sampling kernel (csrc/kernels/decode.hip sample_token) against the
float64 reference of ref_sample.py, its binding's validation, and sampled
decoding end to end on the GPU."""
import pytest
import torch

import ref_sample as rs
from tensorflow_distributed_on_gke_amd.infer.greedy import Tester
from tensorflow_distributed_on_gke_amd.infer.sample import sample_search
from tensorflow_distributed_on_gke_amd.infer.tokenizer import END, START, ByteTokenizer
from tensorflow_distributed_on_gke_amd.models.transformer import PAD_ID, Transformer, model_config
from tensorflow_distributed_on_gke_amd.ops import kernels as K
from tensorflow_distributed_on_gke_amd.ops._ext import C

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _launch(c):
    V = c["ref"]["kept"].shape[1]
    rid = None if c["row_id"] is None else c["row_id"].to(DEV)
    return K.sample_token(c["logits"].to(DEV), V, c["score"].to(DEV), c["fin"].to(DEV), rs.END, rs.PAD,
                          temperature=c["T"], top_k=c["top_k"], top_p=c["top_p"], seed=c["seed"],
                          step=c["step"], row_id=rid)


def _check(c, tag, rows=None):
    """Two launches: bitwise equal, and held to the reference on `rows`
    (default all: every live row of a table case is decided)."""
    ref = c["ref"]
    a, b = _launch(c), _launch(c)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (tag, "two launches differ")
    score, token, fin = (t.cpu() for t in a)
    token, fin = token.long(), fin.long()
    rows = torch.ones_like(ref["live"]) if rows is None else rows
    V = ref["kept"].shape[1]
    assert ((token >= 0) & (token < V)).all(), tag
    assert torch.equal(token[rows], ref["token"][rows]), tag
    assert torch.equal(fin[rows], ref["fin"][rows]), tag
    off = ~ref["live"]
    ended = c["fin"] != 0
    assert (token[off] == rs.PAD).all() and (fin[off] == 1).all(), tag
    assert torch.equal(score[ended], c["score"][ended]), (tag, "an ended row's score changed")
    assert (score[off & ~ended] == rs.NINF).all(), tag
    live = ref["live"] & rows
    assert torch.isfinite(score[live]).all(), tag
    err = (score.double() - ref["score"])[live].abs()
    assert (err <= 1e-4 * ref["score"][live].abs().clamp(min=1.0)).all(), tag
    return token, (float(err.max()) if err.numel() else 0.0)


# ---------------------------------------------------------------- kernel against reference
@pytest.mark.parametrize("R", rs.ROWS)
@pytest.mark.parametrize("V,ldl", rs.SHAPES)
def test_sample_token(V, ldl, R):
    worst = 0.0
    for si in range(rs.N_SETTINGS):
        for kind in rs.KINDS:
            c = rs.sample_case(V, ldl, R, si, kind)
            assert torch.equal(rs.decided(c["ref"]), c["ref"]["live"]), (si, kind)
            worst = max(worst, _check(c, (si, kind))[1])
    print(f"max score err {worst:.3e}")


def test_sample_token_largest_row():
    V, ldl, R, si, kind = rs.BIG_CASE
    c = rs.sample_case(V, ldl, R, si, kind)
    assert torch.equal(rs.decided(c["ref"]), c["ref"]["live"])
    print(f"max score err {_check(c, 'big')[1]:.3e}")


@pytest.mark.parametrize("V,ldl,R,si,kind", rs.EDGE_CASES)
def test_sample_token_row_thresholds(V, ldl, R, si, kind):
    c = rs.sample_case(V, ldl, R, si, kind)
    assert torch.equal(rs.decided(c["ref"]), c["ref"]["live"])
    print(f"max score err {_check(c, (V, si))[1]:.3e}")


@pytest.mark.parametrize("V", [7, 300])
@pytest.mark.parametrize("si", range(rs.N_SETTINGS))
def test_distribution_batch(V, si):
    c = rs.dist_case(V, si)
    dec = rs.decided(c["ref"])
    und = 1.0 - dec.double().mean().item()
    print(f"undecided rows {und:.4%}")
    assert und <= 0.01, "the test must not pass by skipping rows"
    token, _ = _check(c, (V, si), rows=dec)
    assert c["ref"]["kept"][0, token].all(), "a token outside the reference's kept set"


# ---------------------------------------------------------------- binding
SENT = 7.0


def _untouched(*tensors):
    torch.cuda.synchronize()
    for t in tensors:
        assert (t.float() == SENT).all().item(), "a rejected call wrote to its output"


def test_sample_token_binding_rejects():
    R, V = 9, 16
    logits = torch.zeros(R, V, dtype=torch.bfloat16, device=DEV)
    score = torch.zeros(R, dtype=torch.float32, device=DEV)
    fin = torch.zeros(R, dtype=torch.int32, device=DEV)
    rid = torch.arange(R, dtype=torch.int32, device=DEV)
    outs = [torch.full((R,), SENT, dtype=torch.float32, device=DEV)] + \
        [torch.full((R,), int(SENT), dtype=torch.int32, device=DEV) for _ in range(2)]

    def call(lg=logits, v=V, sc=score, fn=fin, T=1.0, k=0, p=1.0, ids=rid):
        C().sample_token(lg, v, sc, fn, 3, 0, T, k, p, 1, 2, ids, *outs)

    odd = torch.zeros(R, 20, dtype=torch.bfloat16, device=DEV)  # row stride 20: not a multiple of 8
    bad = [dict(lg=logits.float()), dict(fn=fin.long()), dict(ids=rid.long()), dict(sc=score[:8]),
           dict(lg=odd), dict(v=0), dict(v=65537), dict(T=0.0), dict(T=float("nan")), dict(p=0.0),
           dict(p=1.5), dict(k=-1)]
    for kw in bad:
        with pytest.raises(RuntimeError):
            call(**kw)
    _untouched(*outs)
    call()  # the same call well-formed
    call(ids=None)
    torch.cuda.synchronize()
    assert not (outs[0] == SENT).any() and ((outs[1] >= 0) & (outs[1] < V)).all()
    # equal logits: log(1 / 16) whatever is drawn
    assert torch.allclose(outs[0].cpu(), torch.full((R,), -2.7725887), atol=1e-5)


# ---------------------------------------------------------------- end to end
SENTS = ["muitas pessoas vieram à estação.", "olá", "este é um teste mais longo"]
N, MAXLEN = 3, 12
OPTS = dict(temperature=0.9, top_k=50, top_p=0.95)


@pytest.fixture(scope="module")
def gpu_model():
    m = Transformer(model_config("tiny", src_vocab=300, tgt_vocab=300)).build("cuda:0", seed=4)
    tester = Tester(ByteTokenizer(300), m)
    return m, tester.src_tok.tokenize(SENTS)


@pytest.fixture(scope="module")
def run(gpu_model):
    m, src = gpu_model
    return sample_search(m, src, START, END, n=N, max_length=MAXLEN, seed=11, return_steps=True, **OPTS)


def test_search_replays_through_reference(run):
    tokens, scores, steps = run
    assert tokens.shape[:2] == (3, N) and tokens.dtype == torch.int64 and scores.shape == (3, N)
    assert scores.dtype == torch.float32
    share = rs.check_steps(tokens, scores, steps, 300, N, 11, 0, OPTS, MAXLEN)
    print(f"decided rows over the run: {share:.3%}")
    assert share >= 0.9


def test_search_seed(gpu_model, run):
    m, src = gpu_model
    again = sample_search(m, src, START, END, n=N, max_length=MAXLEN, seed=11, **OPTS)
    assert torch.equal(again[0], run[0]) and torch.equal(again[1], run[1])
    other = sample_search(m, src, START, END, n=N, max_length=MAXLEN, seed=12, **OPTS)
    assert other[0].shape != run[0].shape or not torch.equal(other[0], run[0])


def test_search_row_identity(gpu_model):
    """A sentence alone, with its rows' identities, repeats its rows of a batch
    of sentences of equal length (no padding difference)."""
    m, src = gpu_model
    # the three sentences: the longest one is as long alone as in the batch
    b = int((src != PAD_ID).sum(dim=1).argmax())
    assert (src[b] != PAD_ID).all()
    t3, s3 = sample_search(m, src, START, END, n=N, max_length=MAXLEN, seed=5, **OPTS)
    t1, s1 = sample_search(m, src[b:b + 1], START, END, n=N, max_length=MAXLEN, seed=5, row_id0=b * N,
                           **OPTS)
    n1 = min(t3.shape[2], t1.shape[2])
    assert torch.equal(t3[b, :, :n1], t1[0, :, :n1]) and (t3[b, :, n1:] == PAD_ID).all()
    assert torch.equal(s3[b], s1[0])
    # and in the middle of a batch of sentences of its length
    one = src[b:b + 1]
    g = torch.Generator().manual_seed(3)
    others = torch.randint(4, 300, (2, one.shape[1]), generator=g)
    others[:, 0], others[:, -1] = one[0, 0], one[0, -1]
    batch = torch.cat([others[:1], one, others[1:]], dim=0)
    assert (batch != PAD_ID).all()
    tb, sb = sample_search(m, batch, START, END, n=N, max_length=MAXLEN, seed=5, **OPTS)
    t1, s1 = sample_search(m, one, START, END, n=N, max_length=MAXLEN, seed=5, row_id0=N, **OPTS)
    n1 = min(tb.shape[2], t1.shape[2])
    assert torch.equal(tb[1, :, :n1], t1[0, :, :n1])
    assert (tb[1, :, n1:] == PAD_ID).all() and (t1[0, :, n1:] == PAD_ID).all()
    assert torch.equal(sb[1], s1[0])
