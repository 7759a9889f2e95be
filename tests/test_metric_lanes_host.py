"""The metric on the lane-resident NUTS kernel without a GPU: the two symbols
(mc_program_nuts_metric_lanes, mc_nuts_run_metric_lanes) are declared, exported
and bound; the query and the launch's refusal on host-only programs (planned
with the test hook mc_debug_lane_plan_host); ``nuts_kernel`` validation.
``nuts()`` itself compiles its model on the device before it plans, so its routing errors are in
tests/test_gpu_metric_lanes.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import workloads as W
from mlx_mcmc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mc_program_nuts_metric_lanes", "mc_nuts_run_metric_lanes")


def _host_program(lp, init):
    """The model's program with host tables only, planned as one lane-resident
    slice (mc_debug_lane_plan_host: nothing uploaded)."""
    from mlx_mcmc_amd import _trace

    model = _trace.trace(lp, init)
    lib = _lib.load()
    h = ctypes.c_void_p()
    data = np.ascontiguousarray(model.data, np.float32)
    index = np.ascontiguousarray(model.index, np.int32)
    lib.mc_debug_program_host_only(1)
    try:
        _lib.check(lib.mc_program_create_expr(
            model.c_terms, len(model.terms), model.c_affines, model.n_affines, model.c_exprs,
            model.n_exprs, model.c_nodes, model.n_nodes, model.layout.size, model.lp_const,
            data.ctypes.data_as(ctypes.c_void_p), data.size,
            index.ctypes.data_as(ctypes.c_void_p), index.size, ctypes.byref(h)))
    finally:
        lib.mc_debug_program_host_only(0)
    assert lib.mc_debug_lane_plan_host(h, 1) == 0, (lib.mc_last_error() or b"").decode()
    return h, model.layout.size


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "mcmc355.h")).read()
    lib = _lib.load()
    bound = {n: (res, args) for n, res, args in _lib.SIGNATURES}
    for n in NAMES:
        assert re.search(r"^\s*(?:int|int32_t)\s+%s\s*\(" % n, header, flags=re.M), n
        assert hasattr(lib, n) and n in bound
    # mc_nuts_run_metric's signature
    assert bound["mc_nuts_run_metric_lanes"] == bound["mc_nuts_run_metric"]
    assert bound["mc_program_nuts_metric_lanes"] == bound["mc_program_nuts_lanes"]
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in NAMES:
        assert n in text


def test_query_null_program():
    assert _lib.load().mc_program_nuts_metric_lanes(None, 5) == -1


@pytest.mark.parametrize("name, want, why", [
    ("iso", 1, b""),                                   # a direct term
    ("illcond", 1, b""),                               # a data-scale term
    ("hier", 0, b"broadcast parameters or scalar terms"),
])
def test_query_and_refusal_on_host_programs(name, want, why):
    lib = _lib.load()
    ns = W.ns_product()
    lp, init = {"iso": lambda: W.iso_normal(ns, 70), "illcond": lambda: W.illcond_normal(ns, 100),
                "hier": lambda: W.hierarchical(ns, *W.SHAPES["small"])}[name]()
    h, D = _host_program(lp, init)
    try:
        assert lib.mc_program_nuts_metric_lanes(h, 5) == want
        assert (lib.mc_program_nuts_lanes(h, 5) == 2) == (want == 1)
        if want == 1:
            return
        assert why in lib.mc_last_error()
        # the launch refuses before it touches state, metric or the device
        cfg = _lib.McRunConfig()
        cfg.num_chains, cfg.iter_count, cfg.num_warmup, cfg.num_samples = 2, 2, 2, 2
        cfg.max_tree_depth, cfg.step_size, cfg.target_accept = 5, 0.1, 0.65
        dummy = np.zeros(64, np.uint8).ctypes.data_as(ctypes.c_void_p)
        rc = lib.mc_nuts_run_metric_lanes(h, ctypes.byref(cfg), dummy, None, None, None, 0,
                                          dummy, 0, None)
        assert rc == _lib.MC_ERR_UNSUPPORTED
        msg = lib.mc_last_error()
        assert why in msg and b"mc_nuts_run_metric" in msg
        # mc_nuts_run_metric's validations come first, in its order
        rc = lib.mc_nuts_run_metric_lanes(h, ctypes.byref(cfg), dummy, None, None, None, 0,
                                          None, 0, None)
        assert rc == _lib.MC_ERR_INVALID and b"metric buffer is NULL" in lib.mc_last_error()
        cfg.max_tree_depth = 99
        rc = lib.mc_nuts_run_metric_lanes(h, ctypes.byref(cfg), dummy, None, None, None, 0,
                                          dummy, 0, None)
        assert rc == _lib.MC_ERR_UNSUPPORTED and b"max_tree_depth" in lib.mc_last_error()
    finally:
        lib.mc_program_destroy(h)


def test_unknown_nuts_kernel_names_the_three_values(monkeypatch):
    import mlx_mcmc_amd as m

    monkeypatch.setattr(_lib, "require_device", lambda: (_ for _ in ()).throw(AssertionError()))
    lp, init = W.iso_normal(W.ns_product(), 5)
    with pytest.raises(ValueError) as e:
        m.nuts(lp, init, num_samples=5, num_warmup=5, progress=False, nuts_kernel="bogus")
    for v in ("'auto'", "'tape'", "'lanes'", "'bogus'"):
        assert v in str(e.value)
    with pytest.raises(ValueError, match="'lanes'"):
        m.MCMC(lp).run(init, num_samples=5, num_warmup=5, method="nuts", verbose=False,
                       progress=False, nuts_kernel="bogus")
    # "lanes" goes with a mass matrix: alone it is refused before the device too
    with pytest.raises(ValueError, match="nuts_kernel='lanes'.*mass matrix"):
        m.nuts(lp, init, num_samples=5, num_warmup=5, progress=False, nuts_kernel="lanes")
