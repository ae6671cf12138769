"""The weights of a mixture's members (ops.mixture.normalised_weights): the
default, the normalisation, and the error each of its four callers raises."""
import math

import pytest
import torch

from tensorflow_distributed_on_gke_amd.infer.ensemble import Ensemble
from tensorflow_distributed_on_gke_amd.models.transformer import Transformer, model_config
from tensorflow_distributed_on_gke_amd.ops import kernels as K
from tensorflow_distributed_on_gke_amd.ops.kernels.decode import score_tokens
from tensorflow_distributed_on_gke_amd.ops.mixture import normalised_weights

BAD = {"count": [1.0], "zero": [1.0, 0.0], "negative": [1.0, -2.0], "inf": [1.0, float("inf")],
       "nan": [1.0, float("nan")]}


def test_default_and_normalisation():
    assert normalised_weights(4, None, "x") == [0.25] * 4
    assert normalised_weights(1, [7.0], "x") == [1.0]
    w = [1e16, 1.0, 1.0, 1.0, 1.0]
    total = math.fsum(w)
    assert total != sum(w)  # the plain sum loses the small terms
    assert normalised_weights(5, w, "x") == [x / total for x in w]
    assert normalised_weights(2, (2, 1), "x") == [2.0 / 3.0, 1.0 / 3.0]
    assert K.distill_weights(2, (2, 1)) == [2.0 / 3.0, 1.0 / 3.0]


@pytest.fixture(scope="module")
def model():
    return Transformer(model_config("tiny", src_vocab=40, tgt_vocab=40)).build("cpu", seed=1)


@pytest.mark.parametrize("kind", sorted(BAD))
def test_each_site_keeps_its_error(model, kind):
    w, x, lab = BAD[kind], torch.zeros(2, 8), torch.ones(2, dtype=torch.int64)
    shown = str([float(v) for v in w])
    with pytest.raises(RuntimeError) as e:
        K.ensemble_logprobs([x, x], 7, w)
    assert str(e.value) == f"ensemble_logprobs: needs 2 finite weights > 0, got {shown}"
    with pytest.raises(RuntimeError) as e:
        score_tokens([x, x], 7, lab, w)
    assert str(e.value) == f"score_tokens: needs 2 finite weights > 0, got {shown}"
    with pytest.raises(RuntimeError) as e:
        K.distill_weights(2, w)
    assert str(e.value) == f"xent_distill: needs 2 finite weights > 0, got {shown}"
    with pytest.raises(ValueError) as e:
        Ensemble([model, model], w)
    assert str(e.value) == ("1 weights for 2 ensemble members" if kind == "count" else
                            f"ensemble weights must be finite and > 0, got {shown}")
