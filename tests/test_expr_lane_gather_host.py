"""Gathered-parameter expression terms on the lane-resident layout, on the
CPU (csrc/host.h expr_term_class, plan_slices.hip plan_bundles, plan_lanes.hip deal,
jit.hip gen_lane_term's grouped form; hiprtc cross-compiles gfx950 without a
device): the planner takes `alpha[g] + beta[g] * x` likelihoods, deals whole
bundles of private parameters to a lane's consecutive slots, and the
generated lane code compiles into k_hmc_lr, k_nuts_sl and k_mh_sl at the planned
register slots;
the declines carry their notes; programs without such terms plan exactly as
before (tests/golden/lane_plan_invariance.json, recorded from the build
before grouped terms).  Running the code is tests/test_gpu_expr_lane_gather.py."""
import json
import os

import pytest

import workloads as W
from _jit_models import host_program
from _lane_gather import INVARIANT, lane_source, observe_plan, poly_slopes

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "lane_plan_invariance.json")

# model, slices, lane_bundle, lane_slots
PLANS = {
    "varying_slopes": (lambda ns: W.varying_slopes(ns, 40, 2600), 4, 2, 2),
    "three_vectors": (lambda ns: poly_slopes(ns, 40, 2600, nvec=3), 4, 3, 4),
    "weighted_indexed": (lambda ns: W.weighted_indexed(ns, 64, 2600), 4, 1, 1),
}


@pytest.mark.parametrize("name", list(PLANS))
def test_grouped_terms_plan_and_compile(name):
    from mlx_mcmc_amd import _lib

    lib = _lib.load()
    build, S, bundle, rs = PLANS[name]
    lp, init = build(W.ns_product())
    h = host_program(lp, init)
    try:
        assert lib.mc_debug_lane_plan_host(h, S) == 0, (lib.mc_last_error() or b"").decode()
        assert lib.mc_program_lane_bundle(h) == bundle
        assert lib.mc_program_lane_slots(h) == rs
        assert lib.mc_program_lane_rep(h) == 1
        src = lane_source(h)
        assert "mc_jit_lane_gexpr" in src and "lr_slot_q<RS, " in src and "ex2_fwd(" in src
        # k_hmc_lr at the planned slots (<= 8 slices: 4 waves), with the
        # exchange records in HBM and L2-resident
        kernels = [f"mc::k_hmc_lr<{rs}, 3, 4, false, {xl}>" for xl in ("false", "true")]
        # NUTS and MH: the sliced kernels' run-time forms (one chain per wave)
        kernels += [f"mc::k_nuts_sl<{rs}, 3, 8, 2, -1, false>", f"mc::k_mh_sl<{rs}, 3, 8, 2, -1, true>"]
        assert "mc_jit_lane_gexpr1v" in src and "lr_slot1_q<RS, " in src
        for k in kernels:
            rc = lib.mc_debug_expr_jit_compile(h, k.encode())
            assert rc == 0, (k, (lib.mc_last_error() or b"").decode()[:3000])
    finally:
        lib.mc_program_destroy(h)


DECLINES = {
    # 1200 private parameters over 4 slices: 300 per slice
    "many_groups": (lambda ns: W.varying_slopes(ns, 600, 3000), "256 private parameters"),
    # four coefficient vectors and one more: a bundle of five
    "five_vectors": (lambda ns: poly_slopes(ns, 20, 2600, nvec=4, extra=1),
                     "gathers 5 parameter vectors"),
    # the default varying-slopes program: 1635 elements
    "small_program": (lambda ns: W.varying_slopes(ns), "fewer than 2048"),
}


@pytest.mark.parametrize("name", list(DECLINES))
def test_grouped_terms_decline_with_a_note(name):
    from mlx_mcmc_amd import _lib

    lib = _lib.load()
    build, note = DECLINES[name]
    lp, init = build(W.ns_product())
    h = host_program(lp, init)
    try:
        assert lib.mc_debug_lane_plan_host(h, 4) != 0
        assert note in (lib.mc_last_error() or b"").decode()
        assert lib.mc_program_lane_bundle(h) == 0 and lane_source(h) == ""
    finally:
        lib.mc_program_destroy(h)


@pytest.mark.parametrize("name", list(INVARIANT))
def test_plans_without_grouped_terms_are_unchanged(name):
    with open(GOLDEN) as f:
        want = json.load(f)[name]
    assert observe_plan(name) == want
