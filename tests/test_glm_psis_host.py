"""loo_kernel at the boundaries that need no device: the option's values, what
each refuses before the device is asked for, and the two entry points at the
C-ABI boundary."""
import ctypes

import numpy as np
import pytest

import _glm
import _glm_pointwise as GP
from mlx_mcmc_amd import _lib, diagnostics


def _loo(fn, c, **kw):
    return diagnostics.loo(fn, c.draws, GP.layout_of(c), group=False, **kw)


def test_the_new_entries_are_bound_with_the_header_signatures():
    lib = _lib.load()
    sig = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    i64, vp, f64 = ctypes.c_int64, ctypes.c_void_p, ctypes.c_double
    assert sig["mc_glm_psis_workspace_bytes"] == (i64, [vp, i64, i64, f64])
    assert sig["mc_glm_psis_loo"] == (ctypes.c_int, [vp, i64, i64, f64, vp, vp, vp, vp, i64, vp])
    assert hasattr(lib, "mc_glm_psis_loo") and hasattr(lib, "mc_glm_psis_workspace_bytes")
    assert lib.mc_glm_psis_workspace_bytes(None, 1, 1, 1.0) == _lib.MC_ERR_INVALID
    assert lib.mc_glm_psis_loo(None, 1, 1, 1.0, None, None, None, None, 0,
                               None) == _lib.MC_ERR_INVALID


def test_what_the_option_refuses_before_the_device_is_asked_for():
    """(without a device require_device raises EngineUnavailable, not ValueError)"""
    import mlx_mcmc_amd as m
    import mlx_mcmc_amd.core as mx

    c = GP.case("bernoulli", 9, 2, 1, 6)
    ns = _glm.ns_product()
    with pytest.raises(ValueError, match="loo_kernel must be 'auto' or 'glm'"):
        _loo(c.log_likelihood, c, loo_kernel="nonsense")
    plain = lambda p: mx.sum(m.Normal(p["w"][0], 1.0).log_prob(np.zeros(3, np.float32)))  # noqa: E731
    with pytest.raises(ValueError, match="loo_kernel='glm' takes a design-matrix likelihood"):
        _loo(plain, c, loo_kernel="glm")
    with pytest.raises(ValueError, match=r"exactly one mx\.sum\(Family\(X @ beta"):
        _loo(lambda p: c.log_likelihood(p) + ns.sum(ns.Normal(0.0, 2.0).log_prob(p["w"])), c,
             loo_kernel="glm")
    with pytest.raises(ValueError, match="LOO.*loo_kernel='glm'"):
        _loo(c.log_likelihood, c)
