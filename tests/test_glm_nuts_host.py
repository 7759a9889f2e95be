"""nuts(nuts_kernel="glm") without a GPU: what the option refuses before any
device work, and the new entry points at the C-ABI boundary."""
import ctypes
import os
import re

import numpy as np
import pytest

import _glm
from mlx_mcmc_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                      "mcmc355.h")

NEW = ("mc_nuts_glm_workspace_bytes", "mc_nuts_run_glm", "mc_debug_glm_nuts_stats")


def test_glm_option_is_refused_by_name():
    import mlx_mcmc_amd as m
    import mlx_mcmc_amd.core as mx

    kw = dict(num_samples=2, num_warmup=2, progress=False, nuts_kernel="glm")
    plain = lambda p: mx.sum(m.Normal(p["x"], 1.0).log_prob(np.zeros(3, np.float32)))  # noqa: E731
    with pytest.raises(ValueError, match="design-matrix"):
        m.nuts(plain, {"x": 0.0}, **kw)
    lp, init = _glm.model(_glm.ns_product(), _glm.data("bernoulli", 9, 2))
    with pytest.raises(ValueError, match="mass matrix"):
        m.nuts(lp, init, adapt_mass_matrix=True, **kw)


def test_new_entry_points_are_declared_exported_and_bound():
    lib, text = _lib.load(), open(HEADER).read()
    bound = {n for n, _, _ in _lib.SIGNATURES}
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", text) and hasattr(lib, name) and name in bound, name


def test_null_arguments_fail_before_device_work():
    lib = _lib.load()
    assert lib.mc_nuts_glm_workspace_bytes(None, 4, 5) == -1
    cfg = _lib.McRunConfig()
    rc = lib.mc_nuts_run_glm(None, ctypes.byref(cfg), None, None, None, None, 0, None)
    assert rc == _lib.MC_ERR_INVALID and b"NULL" in lib.mc_last_error()
