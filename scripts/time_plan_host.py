#!/usr/bin/env python3
"""Host planning time on the CPU: mc_program_create_expr (host tables only) +
mc_debug_lane_plan_host of the two largest planned shapes, 5 runs each; prints
one JSON line.  Another build: python scripts/ab_lib.py LIB.so scripts/time_plan_host.py
(profiles/plan_refactor/host_plan_time.json)."""
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

import numpy as np  # noqa: E402

import workloads as W  # noqa: E402

CASES = {"hierarchical_large_S16": (lambda ns: W.hierarchical(ns, *W.SHAPES["large"]), 16),
         "varying_intercept_200_100000_S16": (lambda ns: W.varying_intercept(ns, 200, 100_000), 16)}


def main():
    from mlx_mcmc_amd import _lib, _trace

    lib = _lib.load()
    out = {}
    for name, (build, S) in CASES.items():
        model = _trace.trace(*build(W.ns_product()))
        data = np.ascontiguousarray(model.data, np.float32)
        index = np.ascontiguousarray(model.index, np.int32)
        times = []
        for _ in range(5):
            h = ctypes.c_void_p()
            lib.mc_debug_program_host_only(1)
            t0 = time.perf_counter()
            _lib.check(lib.mc_program_create_expr(
                model.c_terms, len(model.terms), model.c_affines, model.n_affines, model.c_exprs,
                model.n_exprs, model.c_nodes, model.n_nodes, model.layout.size, model.lp_const,
                data.ctypes.data_as(ctypes.c_void_p), data.size,
                index.ctypes.data_as(ctypes.c_void_p), index.size, ctypes.byref(h)))
            _lib.check(lib.mc_debug_lane_plan_host(h, S))
            times.append(time.perf_counter() - t0)
            lib.mc_debug_program_host_only(0)
            lib.mc_program_destroy(h)
        out[name] = {"seconds": [round(t, 5) for t in times],
                     "median": round(statistics.median(times), 5),
                     "spread": round(max(times) - min(times), 5)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
