"""k_hmc_lf's moment sums from per-run constants on the exchange kernels
(lanes_fast.h lf_moments: M1 = fma(n, d, R), M2 = fma(fma(n, d, 2 R), d, Q),
d = c - theta; the planner's table, plan_lanes.hip lane_moments; no step reads
an observation).

The frame of tests/test_gpu_lf_first_moment.py — its six cases, the +1e3 shift
among them (a dropped or negated 2 d R term leaves the bounds there:
tests/test_lf_second_moment_reference.py) — with an explicit slice count, so
the kernels whose workgroups exchange records run (the automatic plan's dense
route has tests/test_gpu_hmc_dense.py): 12 groups on 2 slices, one lane per
parameter (MC_LANES_REP=1), and the small hierarchical shape as the planner
lays it out on 2 slices (rep > 1: a lane's constants are of its part of the
run).  4 chains, 6 iterations, L = 1 and 3, the compile-time and the run-time
form.

  * the state (position, gradient, log p) against the closed form in float64
    within _ragged.bounds;
  * one launch against launches of 1 + 2 + 3 iterations: byte-identical.
"""
import numpy as np
import pytest

import workloads as W
from _lf_first_moment import PATTERNS, shifted_hier
from _ragged import check_state

pytestmark = pytest.mark.gpu

C = 4
STEPS = (1, 3)
SPLITS = (1, 2, 3)
# (pattern, data order, shift, step size): tests/test_gpu_lf_first_moment.py's
CASES = [("bench", "sorted", 0.0, 0.0305), ("r1_rem3", "shuffled", 0.0, 0.0604),
         ("r2_tail3", "sorted", 0.0, 0.0529), ("r6_exact", "shuffled", 0.0, 0.0312),
         ("short", "sorted", 0.0, 0.11), ("bench", "sorted", 1e3, 0.0305)]
EPS_SMALL = 0.04
_progs = {}


def _hmc_state(prog, q0, splits, L, runtime, eps):
    """Everything an HMC run of sum(splits) iterations leaves behind."""
    import torch

    from mlx_mcmc_amd import _engine, _lib

    n = sum(splits)
    cfg = dict(chain_offset=0, num_warmup=n // 2, num_samples=n - n // 2, sample_begin=0,
               sample_capacity=n - n // 2, seed=5, step_size=eps, target_accept=0.8,
               num_leapfrog_steps=L, adapt_step_size=True)
    if runtime:     # k_hmc_lf reads its form at run time
        _lib.load().mc_debug_lanes_forms(0)
    try:
        cs = _engine.ChainSet(prog, C, q0, eps)
        out = torch.zeros((C, n - n // 2, prog.D), dtype=torch.float32, device=cs.device)
        it = 0
        for k in splits:
            cs.run_hmc(samples=out, iter_begin=it, iter_count=k, **cfg)
            it += k
        torch.cuda.synchronize()
        cs.check_status()
    finally:
        if runtime:
            _lib.load().mc_debug_lanes_forms(1)
    sc = cs.scalars()
    return {"samples": out.cpu().numpy(), "q": cs.positions().cpu().numpy(),
            "g": cs.gradients().cpu().numpy(), "logp": sc["logp"].copy(),
            "step_size": sc["step_size"].copy(),
            "n_accept": sc["n_accept"] + sc["warmup_accept"],
            "n_total": sc["n_total"] + sc["warmup_total"]}


def _check(prog, q0, data, eps, what):
    n = sum(SPLITS)
    assert prog.hmc_dense is None, "an explicit slice count runs the exchange kernels"
    for runtime in (False, True):
        for L in STEPS:
            w = f"{what} runtime={runtime} L={L}"
            one = _hmc_state(prog, q0, (n,), L, runtime, eps)
            print(f"{w}: accepted {one['n_accept'].tolist()} of {n}")
            assert np.all(one["n_total"] == n), w
            assert np.all(one["n_accept"] >= 1), w + ": every chain must have moved"
            check_state(one["q"], one["g"], one["logp"], data, what=w)
            parts = _hmc_state(prog, q0, SPLITS, L, runtime, eps)
            for k in one:
                assert one[k].tobytes() == parts[k].tobytes(), f"{w}: {k} differs over splits"


@pytest.mark.parametrize("name,order,shift,eps", CASES)
def test_state_against_f64_and_launch_splits(gpu, monkeypatch, name, order, shift, eps):
    from mlx_mcmc_amd import _trace

    key = (name, order, shift)
    lp, init, data = shifted_hier(W.ns_product(), PATTERNS[name], order=order, shift=shift)
    if key not in _progs:
        monkeypatch.setenv("MC_LANES_REP", "1")   # (read when the lanes are planned)
        _progs[key] = _trace.compile_model(lp, init, slices=2, slice_kernel="lanes")
    prog = _progs[key]
    assert prog.slice_kernel == "lanes" and prog.lanes_fast, prog.kernel_note
    assert prog.num_slices == 2 and (prog.lane_slots, prog.lane_rep) == (1, 1)
    _check(prog, prog.layout.flatten(init), data, eps, f"{name} {order} +{shift:g}")


def test_small_shape_as_planned_two_slices(gpu):
    from mlx_mcmc_amd import _trace

    G, N = W.SHAPES["small"]
    lp, init = W.hierarchical(W.ns_product(), G, N)
    y, group = W.hierarchical_data(G, N)
    prog = _trace.compile_model(lp, init, slices=2, slice_kernel="lanes")
    assert prog.slice_kernel == "lanes" and prog.lanes_fast and prog.num_slices == 2
    assert prog.lane_rep > 1, prog.lane_rep
    _check(prog, prog.layout.flatten(init), {"y": y, "group": group, "G": G}, EPS_SMALL,
           "small, 2 slices")
