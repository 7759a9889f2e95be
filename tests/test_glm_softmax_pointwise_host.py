"""pointwise_kernel= without a device: the value is checked, "glm" refuses by
name whatever is not a design-matrix likelihood passed alone, and "auto" keeps
refusing a softmax likelihood."""
import numpy as np
import pytest

import _glm_softmax as G
import mlx_mcmc_amd as m
import mlx_mcmc_amd.core as mx

D_ = G.data(9, 2, 3)
DRAWS = {"B": np.zeros((1, 2, 2, 3), np.float32)}   # kept draws [C, S, P, K]
softmax = lambda p: mx.sum(m.Categorical(logits=mx.array(D_.X) @ p["B"]).log_prob(D_.y))  # noqa: E731
ENTRIES = [m.diagnostics.waic, m.diagnostics.pointwise_log_likelihood]


@pytest.mark.parametrize("entry", ENTRIES)
def test_an_unknown_value_is_refused(entry):
    with pytest.raises(ValueError, match="pointwise_kernel must be 'auto' or 'glm', not 'mfma'"):
        entry(softmax, DRAWS, pointwise_kernel="mfma")


@pytest.mark.parametrize("like,word", [
    (lambda p: mx.sum(m.Normal(p["B"], 1.0).log_prob(0.5)), "design-matrix likelihood only"),
    (lambda p: softmax(p) + mx.sum(m.Normal(0.0, 2.0).log_prob(p["B"])), "1 term(s) beside"),
])
@pytest.mark.parametrize("entry", ENTRIES)
def test_glm_refuses_other_likelihoods_by_name(entry, like, word):
    with pytest.raises(ValueError) as e:
        entry(like, DRAWS, pointwise_kernel="glm")
    assert str(e.value).startswith("pointwise_kernel='glm'") and word in str(e.value)


def test_auto_keeps_refusing_softmax():
    with pytest.raises(ValueError) as e:
        m.diagnostics.waic(softmax, DRAWS, pointwise_kernel="auto")
    assert "pointwise log-likelihood" in str(e.value) and "pointwise_kernel='glm'" in str(e.value)
