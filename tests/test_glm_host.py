"""Design-matrix GLMs without a device: what traces to a GLM record, what is
refused by name, and the samplers that decline such a model before a launch."""
import numpy as np
import pytest

import _glm
import mlx_mcmc_amd as m
import mlx_mcmc_amd.core as mx
from mlx_mcmc_amd import _lib, _trace

D_ = _glm.data("poisson", 33, 3)
X, Y, OFF = D_.X, D_.y, D_.off
INIT = {"a": np.float32(0.0), "beta": np.zeros(5, np.float32), "s": np.float32(1.0),
        "B": np.zeros((3, 2), np.float32)}
PRIOR = lambda p: mx.sum(m.Normal(0.0, 2.0).log_prob(p["beta"]))   # noqa: E731


@pytest.mark.parametrize("family", _glm.FAMILIES)
def test_accepted_forms_trace_to_one_glm_record(family):
    d = _glm.data(family, 33, 3)
    model = _trace.trace(*_glm.model(_glm.ns_product(), d))
    g, spec = model.c_glm, model.glm
    assert spec.family == _trace.GLM_FAMILIES[family.capitalize()]
    assert (g.n, g.p, g.beta_offset, g.x_pool, g.y_pool) == (33, 3, 1, 0, 99)
    assert g.offset_pool == (132 if family == "poisson" else -1)
    assert (g.intercept.kind, g.intercept.param_offset) == (_lib.MC_OP_PSCALAR, 0)
    np.testing.assert_array_equal(model.data[:99].reshape(33, 3), d.X)
    np.testing.assert_array_equal(model.data[99:132], d.y)
    n_priors = 3 if family == "normal" else 2
    assert len(model.terms) == n_priors and model.n_exprs == 0
    if family == "normal":
        assert (g.scale.kind, g.scale.param_offset, g.scale.transform) == (
            _lib.MC_OP_PSCALAR, 4, _lib.MC_XF_EXP)


def test_sum_order_constants_slices_and_matmul():
    """The offset, a constant and the intercept in any order; beta a slice;
    mx.matmul; a constant beside the intercept joins the offset."""
    def lp(p):
        eta = OFF + ((0.5 + p["a"]) + mx.matmul(X, p["beta"][1:4])) + 0.25
        return mx.sum(m.Poisson(log_rate=eta).log_prob(Y)) + PRIOR(p)
    model = _trace.trace(lp, INIT)
    g = model.c_glm
    assert (g.beta_offset, g.p, g.intercept.kind) == (2, 3, _lib.MC_OP_PSCALAR)
    np.testing.assert_allclose(model.data[g.offset_pool:g.offset_pool + 33], OFF + 0.75, rtol=1e-6)
    assert model.lp_const == np.float32(np.sum(_trace.discrete_norm("Poisson", Y), dtype=np.float64))


@pytest.mark.parametrize("name,lp,msg", [
    ("two matvecs", lambda p: mx.sum(m.Bernoulli(logits=X @ p["beta"][:3] + X @ p["beta"][2:])
                                     .log_prob(Y)), "two matvec terms"),
    ("two likelihoods", lambda p: mx.sum(m.Poisson(log_rate=X @ p["beta"][:3]).log_prob(Y))
     + mx.sum(m.Poisson(log_rate=X @ p["beta"][2:]).log_prob(Y)), "two matvec terms"),
    ("inside an expression", lambda p: mx.sum(m.Poisson(log_rate=2.0 * (X @ p["beta"][:3]))
                                              .log_prob(Y)), "matvec inside another expression"),
    ("mx.exp of it", lambda p: mx.sum(m.Normal(mx.exp(X @ p["beta"][:3]), 1.0).log_prob(Y)),
     "matvec inside another expression"),
    ("traced prior argument", lambda p: mx.sum(m.Poisson(log_rate=X @ p["beta"][:3]).log_prob(Y))
     + m.Normal(p["a"], 1.0).log_prob(p["s"]), "prior with a traced argument"),
    ("probs=", lambda p: mx.sum(m.Bernoulli(probs=X @ p["beta"][:3]).log_prob(Y)), "probs= / rate="),
    ("rate=", lambda p: mx.sum(m.Poisson(rate=X @ p["beta"][:3]).log_prob(Y)), "probs= / rate="),
    ("matrix beta", lambda p: mx.sum(m.Poisson(log_rate=X @ p["B"]).log_prob(Y)),
     "multi-dimensional"),
])
def test_refused_forms_name_the_accepted_one(name, lp, msg):
    with pytest.raises(_trace.TraceError) as e:
        _trace.trace(lp, INIT)
    assert msg in str(e.value) and "a design-matrix model is eta = X @ beta" in str(e.value)


@pytest.mark.parametrize("call", [
    lambda lp, init: m.nuts(lp, init, num_samples=2, num_warmup=2, progress=False),
    lambda lp, init: m.metropolis_hastings(lp, init, num_samples=2),
    lambda lp, init: m.hmc(lp, init, num_samples=2, num_warmup=2, progress=False,
                           adapt_mass_matrix=True),
])
def test_other_samplers_decline_before_any_launch(call):
    with pytest.raises(ValueError, match="run under hmc"):
        call(*_glm.model(_glm.ns_product(), D_))


@pytest.mark.gpu
def test_the_column_cap_is_refused_by_name(gpu):
    d = _glm.data("bernoulli", 4, 257)
    with pytest.raises(_lib.EngineError) as e:
        _trace.compile_model(*_glm.model(_glm.ns_product(), d))
    assert e.value.code == _lib.MC_ERR_UNSUPPORTED and "at most 256" in str(e.value)
