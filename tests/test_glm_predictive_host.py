"""predictive_kernel at the boundaries that need no device: the option's values
and the two entry points at the C-ABI boundary."""
import ctypes

import numpy as np
import pytest

from mlx_mcmc_amd import _lib, diagnostics


def test_an_unknown_value_is_refused_before_the_device_is_asked_for():
    """(without a device require_device raises EngineUnavailable, not ValueError)"""
    with pytest.raises(ValueError, match="predictive_kernel must be 'auto' or 'glm'"):
        diagnostics.posterior_predictive(lambda p: p["x"], {"x": np.zeros((1, 2), np.float32)},
                                         group=False, predictive_kernel="mfma")


def test_the_new_entries_are_bound_with_the_header_signatures():
    lib = _lib.load()
    sig = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    i64, vp = ctypes.c_int64, ctypes.c_void_p
    assert sig["mc_glm_predictive_workspace_bytes"] == (i64, [vp, i64, i64, i64])
    assert sig["mc_glm_predictive"] == (
        ctypes.c_int, [vp, i64, i64, i64, ctypes.c_uint64, i64, i64, vp, vp, vp, vp, vp, i64, vp])
    assert hasattr(lib, "mc_glm_predictive") and hasattr(lib, "mc_glm_predictive_workspace_bytes")
    assert lib.mc_glm_predictive_workspace_bytes(None, 1, 1, 1) == _lib.MC_ERR_INVALID
