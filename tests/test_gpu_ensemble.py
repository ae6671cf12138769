"""The ensemble's combine kernel (csrc/kernels/decode.hip ensemble_logprobs)
against the float64 reference of ref_ensemble.py, its determinism, its
binding's validation, and ensemble decoding end to end on the GPU."""
import pytest
import torch

import ref_ensemble as re_
import ref_sample as rs
from tensorflow_distributed_on_gke_amd.infer.beam import beam_search
from tensorflow_distributed_on_gke_amd.infer.ensemble import Ensemble
from tensorflow_distributed_on_gke_amd.infer.sample import sample_search
from tensorflow_distributed_on_gke_amd.infer.tokenizer import END, START, ByteTokenizer
from tensorflow_distributed_on_gke_amd.models.transformer import PAD_ID, Transformer, model_config
from tensorflow_distributed_on_gke_amd.ops import kernels as K
from tensorflow_distributed_on_gke_amd.ops._ext import C

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 7.0
MARGIN = 16  # sentinel columns beyond ldo in the allocation the output is a view of


def _bits(t):
    return t.view(torch.int16)


def _members(logits):
    return [x.to(torch.bfloat16).to(DEV) for x in logits]


def _run(members, V, ldo, weights):
    """The kernel into the first ldo columns of a wider, sentinel-filled
    allocation; returns that view after checking the margin."""
    R = members[0].shape[0]
    wide = torch.full((R, ldo + MARGIN), SENT, dtype=torch.bfloat16, device=DEV)
    out = wide[:, :ldo]
    assert K.ensemble_logprobs(members, V, weights, out=out) is out
    torch.cuda.synchronize()
    assert (wide[:, ldo:].float() == SENT).all(), "the kernel wrote beyond column ldo"
    return out


def _check_case(V, ldo, M, R, kind):
    logits, weights, ref = re_.case(V, ldo, M, R, kind)
    out = _run(_members(logits), V, ldo, weights)
    err = re_.check_against(out, ref, re_.bf16_bound, (kind, M, R))
    print(f"{kind}: max err {err:.3e}")


# ---------------------------------------------------------------- kernel against reference
@pytest.mark.parametrize("R", re_.ROWS)
@pytest.mark.parametrize("M", re_.MEMBERS)
@pytest.mark.parametrize("V,ldo", re_.SHAPES)
def test_ensemble_logprobs(V, ldo, M, R):
    for kind in re_.KINDS:
        _check_case(V, ldo, M, R, kind)


@pytest.mark.parametrize("M", re_.MEMBERS)
def test_ensemble_logprobs_largest_row(M):
    V, ldo = re_.BIG_SHAPE
    for kind in re_.KINDS:
        _check_case(V, ldo, M, 2, kind)


@pytest.mark.parametrize("R", re_.ROWS)
def test_mixed_strides(R):
    """Members with row strides 304 and 312 and one that is a column slice of a
    wider tensor (row stride 640, starting 16 columns in)."""
    V, ldo = 300, 304
    logits, weights, ref = re_.case(V, ldo, 3, R, "weights")
    a = logits[0].to(torch.bfloat16).to(DEV)
    b = torch.full((R, 312), 1e4, dtype=torch.bfloat16, device=DEV)
    b[:, :ldo] = logits[1].to(torch.bfloat16)
    wide = torch.full((R, 640), 1e4, dtype=torch.bfloat16, device=DEV)
    c = wide[:, 16:16 + ldo]
    c.copy_(logits[2].to(torch.bfloat16))
    assert (a.stride(0), b.stride(0), c.stride(0)) == (304, 312, 640)
    out = _run([a, b[:, :ldo], c], V, ldo, weights)
    err = re_.check_against(out, ref, re_.bf16_bound, "mixed strides")
    print(f"max err {err:.3e}")
    same = _run(_members(logits), V, ldo, weights)
    assert torch.equal(_bits(out), _bits(same)), "the result depends on the members' strides"


# ---------------------------------------------------------------- determinism
@pytest.mark.parametrize("V,ldo", re_.SHAPES)
def test_two_launches_and_swapped_members(V, ldo):
    for kind in ("random", "peaked", "masked"):
        for M in (2, 8):
            logits, weights, _ = re_.case(V, ldo, M, 5, kind)
            mem = _members(logits)
            a, b = _run(mem, V, ldo, weights), _run(mem, V, ldo, weights)
            assert torch.equal(_bits(a), _bits(b)), (kind, M, "two launches differ")
            if M == 2:  # equal weights: f32 max and a two-term sum commute
                c = _run(mem[::-1], V, ldo, weights)
                assert torch.equal(_bits(a), _bits(c)), (kind, "swapped members differ")


# ---------------------------------------------------------------- binding
def _untouched(*tensors):
    torch.cuda.synchronize()
    for t in tensors:
        assert (t.float() == SENT).all().item(), "a rejected call wrote to its output"


def test_binding_rejects():
    R, V = 3, 16
    x = torch.zeros(R, V, dtype=torch.bfloat16, device=DEV)
    out = torch.full((R, V), SENT, dtype=torch.bfloat16, device=DEV)

    def call(mem=(x, x), v=V, w=(0.5, 0.5), o=out):
        C().ensemble_logprobs(list(mem), v, list(w), o)

    flat = torch.zeros(R * V + 8, dtype=torch.bfloat16, device=DEV)
    off = flat[1:1 + R * V].view(R, V)  # 2 bytes off a 16-byte boundary
    odd = torch.zeros(R, 20, dtype=torch.bfloat16, device=DEV)  # row stride 20: not a multiple of 8
    big = torch.zeros(1, 65544, dtype=torch.bfloat16, device=DEV)
    big_out = torch.full((1, 65544), SENT, dtype=torch.bfloat16, device=DEV)
    bad = [dict(mem=[x] * 9, w=[1 / 9] * 9), dict(mem=[], w=[]), dict(mem=(x, x.float())), dict(mem=(x, off)),
           dict(mem=(x, odd)), dict(mem=(big, big), v=65537, o=big_out),
           dict(v=0), dict(o=out[:2]), dict(o=out[:, :8]), dict(mem=(x, x.cpu())), dict(w=(1.0, 0.0)),
           dict(w=(1.0, float("nan"))), dict(w=(1.0, float("inf"))), dict(w=(1.0, -1.0)), dict(w=(1.0,)),
           dict(mem=(x, x[:2]))]
    for kw in bad:
        with pytest.raises(RuntimeError):
            call(**kw)
        _untouched(kw.get("o", out))
    with pytest.raises(RuntimeError):  # a CPU output
        call(mem=(x.cpu(), x.cpu()), o=torch.full((R, V), SENT, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError):  # an f32 output
        call(o=torch.full((R, V), SENT, dtype=torch.float32, device=DEV))
    _untouched(out)
    call()  # the same call well-formed
    torch.cuda.synchronize()
    # equal logits in both members: log(1 / 16) everywhere
    assert torch.allclose(out.float().cpu(), torch.full((R, V), -2.7725887), atol=2.0 ** -6)


def test_wrapper_rejects():
    x = torch.zeros(2, 8, dtype=torch.bfloat16, device=DEV)
    for kw in (dict(logits_list=[x] * 9), dict(weights=[1.0, 0.0]), dict(weights=[1.0, float("nan")]),
               dict(V=65537)):
        with pytest.raises(RuntimeError):
            K.ensemble_logprobs(**dict(dict(logits_list=[x, x], V=7, weights=None), **kw))


# ---------------------------------------------------------------- end to end
SENTS = ["muitas pessoas vieram à estação.", "olá", "este é um teste mais longo"]
N, MAXLEN = 3, 12
OPTS = dict(temperature=0.9, top_k=50, top_p=0.95)


@pytest.fixture(scope="module")
def gpu_models():
    cfg = model_config("tiny", src_vocab=300, tgt_vocab=300)
    m4 = Transformer(cfg).build("cuda:0", seed=4)
    m5 = Transformer(cfg).build("cuda:0", seed=5)
    tok = ByteTokenizer(300)
    return m4, m5, tok, tok.tokenize(SENTS)


def test_beam_deterministic_copy_and_swap(gpu_models):
    m4, m5, _, src = gpu_models
    ens = Ensemble([m4, m5])
    a = beam_search(ens, src, START, END, beam=4, max_length=MAXLEN, reorder="index")
    b = beam_search(ens, src, START, END, beam=4, max_length=MAXLEN, reorder="index")
    c = beam_search(ens, src, START, END, beam=4, max_length=MAXLEN, reorder="copy")
    d = beam_search(Ensemble([m5, m4]), src, START, END, beam=4, max_length=MAXLEN)
    assert a[0].shape[0] == 3 and a[0].shape[1] <= MAXLEN + 1 and bool((a[0][:, 0] == START).all())
    assert torch.isfinite(a[1]).all()
    for x, y, z, s in zip(a, b, c, d):
        assert torch.equal(x, y), "two beam-4 runs differ"
        assert torch.equal(x, z), "reorder='copy' differs from 'index'"
        assert torch.equal(x, s), "the members' order matters"


def test_one_member_is_the_model_bitwise(gpu_models):
    m4, _, _, src = gpu_models
    for x, y in zip(beam_search(m4, src, START, END, beam=4, max_length=MAXLEN),
                    beam_search(Ensemble([m4]), src, START, END, beam=4, max_length=MAXLEN)):
        assert torch.equal(x, y)
    for x, y in zip(sample_search(m4, src, START, END, n=N, max_length=MAXLEN, seed=11, **OPTS),
                    sample_search(Ensemble([m4]), src, START, END, n=N, max_length=MAXLEN, seed=11, **OPTS)):
        assert torch.equal(x, y)


def test_sample_steps_replay(gpu_models):
    m4, m5, _, src = gpu_models
    tokens, scores, steps = sample_search(Ensemble([m4, m5]), src, START, END, n=N, max_length=MAXLEN,
                                          seed=11, return_steps=True, **OPTS)
    assert tokens.shape[:2] == (3, N) and scores.shape == (3, N) and scores.dtype == torch.float32
    R = 3 * N
    score = torch.zeros(R, dtype=torch.float64)
    fin = torch.zeros(R, dtype=torch.int32)
    rid = torch.arange(R, dtype=torch.int32)
    worst = 0.0
    for t, (combined, token, fin_new, member_logits) in enumerate(steps):
        assert len(member_logits) == 2 and combined.dtype == torch.bfloat16
        ref = re_.ensemble_ref([x.cpu().float() for x in member_logits], 300)
        worst = max(worst, re_.check_against(combined, ref, re_.bf16_bound, f"step {t}"))
        # the selection on the CPU, on the step's own combined logits; rows
        # whose two best keys are within rounding are left out, as for one model
        lg, tok = combined.cpu(), token.cpu().long()
        dec = rs.decided(rs.sample_ref(lg, 300, score.float(), fin, rid, OPTS["temperature"], OPTS["top_k"],
                                       OPTS["top_p"], 11, t))
        _, c_token, c_fin = K.sample_token(lg, 300, score.float(), fin, END, PAD_ID, seed=11, step=t,
                                           row_id=rid, **OPTS)
        ended = fin != 0
        rows = dec | ended
        assert torch.equal(tok[rows], c_token.long()[rows]), f"step {t}"
        assert torch.equal(fin_new.cpu()[rows], c_fin[rows]), f"step {t}"
        x = lg[:, :300].double()
        logp = x.gather(1, tok.view(R, 1)).view(R) - torch.logsumexp(x, dim=1)
        score = torch.where(ended, score, score + logp)
        fin = fin_new.cpu()
    print(f"combined: max err {worst:.3e}")
    share = rs.check_steps(tokens, scores, [s[:3] for s in steps], 300, N, 11, 0, OPTS, MAXLEN)
    print(f"decided rows over the run: {share:.3%}")
    assert share >= 0.9
