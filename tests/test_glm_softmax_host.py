"""Softmax regression on a design matrix without a device: what traces to an
mc_glm_softmax record, what is refused by name, and the new entry's limits at
the C-ABI boundary."""
import ctypes

import numpy as np
import pytest

import _glm_softmax as G
import mlx_mcmc_amd as m
import mlx_mcmc_amd.core as mx
from mlx_mcmc_amd import _lib, _trace

D_ = G.data(33, 3, 4)
X, Y = mx.array(D_.X), D_.y
INIT = {"s": np.float32(0.0), "B": np.zeros((3, 4), np.float32), "a": np.zeros(4, np.float32),
        "B1": np.zeros((3, 1), np.float32), "B33": np.zeros((3, 33), np.float32),
        "W": np.zeros((257, 4), np.float32)}
cat = lambda eta, y=Y: mx.sum(m.Categorical(logits=eta).log_prob(y))   # noqa: E731


@pytest.mark.parametrize("intercept", [True, False])
def test_the_accepted_form_traces_to_one_softmax_record(intercept):
    model = _trace.trace(*G.model(G.ns_product(), D_, intercept))
    g, spec = model.c_glm, model.glm
    assert isinstance(g, _lib.McGlmSoftmax) and spec.family == _lib.MC_GLM_CATEGORICAL_LOGIT == 3
    assert (g.n, g.p, g.k, g.beta_offset, g.x_pool, g.y_pool) == (33, 3, 4, 0, 0, 99)
    assert g.icpt_offset == (12 if intercept else -1)
    assert model.layout.size == (16 if intercept else 12) and model.n_exprs == 0
    assert [(t.n, t.value.param_offset) for t in model.terms] == [(12, 0), (4, 12)][:1 + intercept]
    np.testing.assert_array_equal(model.data[:99].reshape(33, 3), D_.X)
    np.testing.assert_array_equal(model.data[99:], D_.y)


BAD_Y = np.where(np.arange(33) == 7, 4, D_.y)
HALF_Y = np.where(np.arange(33) == 2, 0.5, D_.y)


@pytest.mark.parametrize("name,lp,msg", [
    ("K = 1", lambda p: cat(X @ p["B1"], np.zeros(33)), "K = 1 classes"),
    ("K = 33", lambda p: cat(X @ p["B33"]), "K = 33 classes"),
    ("P = 257", lambda p: cat(np.zeros((33, 257), np.float32) @ p["W"]), "P = 257 columns"),
    ("sliced B", lambda p: cat(X @ p["B"][:, :2]), "matrix parameter is used whole"),
    ("transformed B", lambda p: cat(X @ mx.exp(p["B"])), "sliced, gathered or transformed"),
    ("probs=", lambda p: mx.sum(m.Categorical(probs=X @ p["B"]).log_prob(Y)), "passed as logits="),
    ("a data vector", lambda p: cat(X @ p["B"] + np.ones(33, np.float32)), "cancels in the softmax"),
    ("a constant", lambda p: cat(0.5 + X @ p["B"]), "cancels in the softmax"),
    ("a scalar parameter", lambda p: cat(X @ p["B"] + p["s"]), "a scalar parameter moves every"),
    ("a sliced intercept", lambda p: cat(X @ p["B"] + p["W"][0:4]), "whole, untransformed 1-D"),
    ("another operator", lambda p: cat(2.0 * (X @ p["B"])), "inside another expression"),
    ("a label out of range", lambda p: cat(X @ p["B"], BAD_Y), "y[7] = 4"),
    ("a fractional label", lambda p: cat(X @ p["B"], HALF_Y), "y[2] = 0.5"),
])
def test_refused_forms_name_the_accepted_one(name, lp, msg):
    with pytest.raises(_trace.TraceError) as e:
        _trace.trace(lp, INIT)
    assert msg in str(e.value) and "Categorical(logits=X @ B [+ a])" in str(e.value)


DRAWS = {"B": np.zeros((1, 2, 2, 3), np.float32)}  # kept draws [C, S, P, K]


@pytest.mark.parametrize("call,word", [
    (lambda lp, i: m.hmc(lp, i, num_samples=2, num_warmup=2, progress=False, glm_kernel="wide"),
     "glm_kernel='wide': softmax"),
    (lambda lp, i: m.nuts(lp, i, num_samples=2, num_warmup=2, progress=False, nuts_kernel="glm"),
     "nuts_kernel='glm': softmax"),
    (lambda lp, i: m.nuts(lp, i, num_samples=2, num_warmup=2, progress=False), "run under hmc"),
    (lambda lp, i: m.hmc(lp, i, num_samples=2, num_warmup=2, progress=False,
                         adapt_mass_matrix=True), "run under hmc"),
    (lambda lp, i: m.metropolis_hastings(lp, i, num_samples=2), "run under hmc"),
    (lambda lp, i: m.diagnostics.waic(lp, DRAWS), "pointwise log-likelihood"),
    (lambda lp, i: m.diagnostics.posterior_predictive(lp, DRAWS, predictive_kernel="glm"),
     "predictive_kernel='glm': softmax"),
    (lambda lp, i: m.diagnostics.loo(lp, DRAWS, loo_kernel="glm"), "loo_kernel='glm': softmax"),
])
def test_other_entry_points_decline_before_any_launch(call, word):
    d = G.data(9, 2, 3)
    like = lambda p: mx.sum(m.Categorical(logits=mx.array(d.X) @ p["B"]).log_prob(d.y))  # noqa: E731
    with pytest.raises(ValueError) as e:
        call(like, {"B": np.zeros((2, 3), np.float32)})
    assert word in str(e.value), str(e.value)


@pytest.mark.parametrize("K,P,code,word", [
    (1, 3, _lib.MC_ERR_UNSUPPORTED, "K = 1 classes"), (33, 3, _lib.MC_ERR_UNSUPPORTED, "K = 33"),
    (4, 257, _lib.MC_ERR_UNSUPPORTED, "at most 256"), (4, 3, _lib.MC_ERR_INVALID, "label 1 is 4")])
def test_the_new_entry_checks_its_limits_before_any_device_work(K, P, code, word):
    lib = _lib.load()
    assert "mc_program_create_glm_softmax" in {n for n, _, _ in _lib.SIGNATURES}
    g = _lib.McGlmSoftmax(beta_offset=0, icpt_offset=-1, n=2, p=P, k=K, x_pool=0, y_pool=2 * P)
    data = np.zeros(2 * P + 2, np.float32)
    data[-1] = 4.0
    h = ctypes.c_void_p()
    rc = lib.mc_program_create_glm_softmax(ctypes.byref(g), None, 0, P * K, 0.0,
                                           data.ctypes.data_as(ctypes.c_void_p), data.size,
                                           ctypes.byref(h))
    assert rc == code and word in lib.mc_last_error().decode()
