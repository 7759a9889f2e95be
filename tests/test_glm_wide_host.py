"""glm_kernel="wide" at the boundaries: what is refused by name before any
device work, and the new entry at the C-ABI boundary."""
import numpy as np
import pytest

import _glm
import mlx_mcmc_amd as m
import mlx_mcmc_amd.core as mx
from mlx_mcmc_amd import _lib, _trace

PLAIN = lambda p: mx.sum(m.Normal(p["x"], 1.0).log_prob(np.zeros(3, np.float32)))  # noqa: E731


@pytest.mark.parametrize("P,kernel,words", [
    (1025, "wide", ("at most 1024",)),
    (257, "auto", ("at most 256", "glm_kernel=\"wide\"", "mc_program_create_glm_wide"))])
def test_the_column_caps_are_refused_by_name(P, kernel, words):
    """Both entries check P before any device work: no device is needed."""
    model = _trace.trace(*_glm.model(_glm.ns_product(), _glm.data("bernoulli", 4, P)))
    with pytest.raises(_lib.EngineError) as e:
        _trace.Program(model, kernel)
    assert e.value.code == _lib.MC_ERR_UNSUPPORTED
    assert all(w in str(e.value) for w in words), str(e.value)


@pytest.mark.parametrize("call", [
    lambda lp, init, **kw: _trace.compile_model(lp, init, **kw),
    lambda lp, init, **kw: m.hmc(lp, init, num_samples=2, num_warmup=2, progress=False, **kw),
    lambda lp, init, **kw: m.nuts(lp, init, num_samples=2, num_warmup=2, progress=False,
                                  nuts_kernel="glm", **kw),
    lambda lp, init, **kw: m.MCMC(lp).run(init, num_samples=2, num_warmup=2, method="hmc",
                                          verbose=False, progress=False, **kw)])
def test_option_values_and_models_are_checked_before_a_launch(call):
    lp, init = _glm.model(_glm.ns_product(), _glm.data("bernoulli", 9, 2))
    with pytest.raises(ValueError, match="glm_kernel must be 'auto' or 'wide'"):
        call(lp, init, glm_kernel="narrow")
    with pytest.raises(ValueError, match="runs design-matrix models only: a likelihood Family"):
        call(PLAIN, {"x": 0.0}, glm_kernel="wide")


def test_the_new_entry_is_bound():
    assert hasattr(_lib.load(), "mc_program_create_glm_wide")
    assert "mc_program_create_glm_wide" in {n for n, _, _ in _lib.SIGNATURES}
    assert _lib.MC_GLM_WIDE_MAX_P == 1024


@pytest.mark.gpu
def test_pointwise_is_refused_on_a_wide_program(gpu):
    d = _glm.data("bernoulli", 9, 2)
    like = lambda p: mx.sum(m.Bernoulli(logits=mx.array(d.X) @ p["beta"]).log_prob(d.y))  # noqa: E731
    prog = _trace.compile_model(like, {"beta": np.zeros(2, np.float32)}, glm_kernel="wide")
    with pytest.raises(_lib.EngineError) as e:
        prog.enable_pointwise()
    assert e.value.code == _lib.MC_ERR_UNSUPPORTED and "mc_program_create_glm_wide" in str(e.value)
