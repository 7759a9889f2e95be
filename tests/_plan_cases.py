"""The planner's pinned cases (tests/test_plan_digests.py, recorded by
scripts/gen_plan_digests.py into tests/golden/plan_digests.json): a program,
a slice count and the environment that steers the planner; per case the
status, the error text and one FNV-1a digest per host table of the slice plan
and the lane plan (mc_debug_plan_digest)."""
import ctypes

import workloads as W
from _jit_models import host_program
from _lane_gather import poly_slopes
from _ragged import PATTERNS, ragged_hier

# the digests' order (include/mcmc355.h mc_debug_plan_digest)
SLICE_TABLES = ["S", "Lp", "Pmax", "Dsh", "nitems", "sdata_floats", "combine",
                "terms", "sterms", "data", "index", "blocks", "gidx"]
LANE_TABLES = ["ok", "rs", "rep", "S", "Dsh", "nitems", "sdata_floats", "shl", "shxf", "shid",
               "n_generic", "fast", "form", "has_xf", "has_expr", "nuts_expr", "bundle",
               "terms", "data", "blocks", "gidx", "sterms", "rng", "gx_off"]
TABLES = ["slice." + n for n in SLICE_TABLES] + ["lane." + n for n in LANE_TABLES]

# the environment variables the planners read (unset unless a case sets them)
PLANNER_ENV = ("MC_LANES_REP", "MC_LANES_RNG", "MC_EXPR_LANES")


def _hier(shape):
    return lambda ns: W.hierarchical(ns, *W.SHAPES[shape])


def _reparam(shape):
    return lambda ns: W.hierarchical_reparam(ns, *W.SHAPES[shape])


# name -> (builder, slices, environment); every case of PLANS returns MC_OK
# with a lane plan
PLANS = {}
for _shape, _slices in (("small", (1, 2, 4)), ("medium", (4, 8)), ("large", (4, 8, 16))):
    for _S in _slices:
        PLANS[f"hier_{_shape}_S{_S}"] = (_hier(_shape), _S, {})
PLANS.update({
    "reparam_medium_S4": (_reparam("medium"), 4, {}),
    "reparam_small_S1": (_reparam("small"), 1, {}),
    "eight_schools_S1": (W.eight_schools, 1, {}),
    "iso_normal_100_S1": (lambda ns: W.iso_normal(ns, 100), 1, {}),
    "linear_regression_S4": (W.linear_regression, 4, {}),
    "ab_testing_S1": (W.ab_testing, 1, {}),
    "event_rates_S1": (W.event_rates, 1, {}),
    "varying_intercept_S1": (lambda ns: W.varying_intercept(ns, 20, 2000), 1, {}),
    "varying_intercept_big_S16": (lambda ns: W.varying_intercept(ns, 200, 100_000), 16, {}),
    "logistic_20000_S8": (lambda ns: W.logistic_regression(ns, 20_000), 8, {}),
    "varying_slopes_S4": (lambda ns: W.varying_slopes(ns, 40, 2600), 4, {}),
    "poly_slopes3_S4": (lambda ns: poly_slopes(ns, 40, 2600, nvec=3), 4, {}),
    "weighted_indexed_S4": (lambda ns: W.weighted_indexed(ns, 64, 2600), 4, {}),
})
for _name in PATTERNS:     # (tests/_ragged.PLAN: each pattern's plan on one slice)
    PLANS["ragged_" + _name] = ((lambda ns, n=_name: ragged_hier(ns, PATTERNS[n])[:2]), 1, {})
PLANS["hier_small_S1_rep1"] = (_hier("small"), 1, {"MC_LANES_REP": "1"})
PLANS["hier_small_S1_norng"] = (_hier("small"), 1, {"MC_LANES_RNG": "0"})

# declines, pinned by status and message
DECLINES = {
    "iso_normal_300_S1": (lambda ns: W.iso_normal(ns, 300), 1, {}),
    "eight_schools_nc_S1": (W.eight_schools_nc, 1, {}),
    "lognormal_S1": (W.lognormal, 1, {}),
    "many_groups_S4": (lambda ns: W.varying_slopes(ns, 600, 3000), 4, {}),
    "five_vectors_S4": (lambda ns: poly_slopes(ns, 20, 2600, nvec=4, extra=1), 4, {}),
    "small_program_S4": (lambda ns: W.varying_slopes(ns), 4, {}),
}

CASES = dict(PLANS, **DECLINES)


def observe(name):
    """{"status", "error", "digests"} of CASES[name] (the caller has set the
    case's environment and unset the rest of PLANNER_ENV)."""
    from mlx_mcmc_amd import _lib

    lib = _lib.load()
    build, S, _ = CASES[name]
    lp, init = build(W.ns_product())
    h = host_program(lp, init)
    try:
        out = (ctypes.c_uint64 * len(TABLES))()
        rc = lib.mc_debug_plan_digest(h, S, out, len(TABLES))
        err = (lib.mc_last_error() or b"").decode() if rc != 0 else ""
        return {"status": int(rc), "error": err,
                "digests": {t: "%016x" % out[i] for i, t in enumerate(TABLES)}}
    finally:
        lib.mc_program_destroy(h)
