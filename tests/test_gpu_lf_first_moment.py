"""k_hmc_lf's first moment from per-run constants (lanes_fast.h
lf_run_consts / lf_m1: M1 = fma(n, c - theta, R), c and R formed once per
launch from the run's observations; the sweep sums the second moment alone).

Built like tests/test_gpu_lf_sweep_end.py: 12 groups on one slice, one lane
per parameter (MC_LANES_REP=1), 4 chains, 6 iterations, L = 1 and 3, the
compile-time and the run-time form.  Runs: the benchmark's (100 / 101), one
round with an empty group, two rounds with a tail, six rounds exactly, every
run under 16 elements (no round; an empty and a single-element run), and the
benchmark's with the observations shifted by +1e3 (an uncentred sum would
lose them: tests/test_lf_first_moment_reference.py).  And the small
hierarchical shape as the planner lays it out (its parameters replicated over
lane groups, rep > 1: a lane's run is a part of its parameter's), 2 slices.

  * the state (position, gradient, log p) against the closed form in float64
    within _ragged.bounds (the CPU test holds the emulated form inside them at
    these inputs);
  * one launch against launches of 1 + 2 + 3 iterations: byte-identical (the
    constants are formed again by every launch, from the data alone);
  * the compared iterations hold accepted and rejected proposals: the step
    size of a case is about 1.5 / sqrt(2 N), one and a half posterior standard
    deviations of sigma, where the oracle's sampler (oracle/samplers.py hmc,
    the same seed and chains) accepts at least twice and rejects at least once
    in every run, at L = 1 and at L = 3.
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
# (pattern, data order, shift, step size)
CASES = [("bench", "sorted", 0.0, 0.0305), ("r1_rem3", "shuffled", 0.0, 0.0604),
         ("r2_tail3", "sorted", 0.0, 0.0529), ("r6_exact", "shuffled", 0.0, 0.0312),
         ("short", "sorted", 0.0, 0.11), ("bench", "sorted", 1e3, 0.0305)]
EPS_SMALL = 0.04
_models, _progs = {}, {}


def _model(name, order, shift):
    key = (name, order, shift)
    if key not in _models:
        _models[key] = shifted_hier(W.ns_product(), PATTERNS[name], order=order, shift=shift)
    return _models[key]


class _forms:
    """mc_debug_lanes_forms(0) around a launch: k_hmc_lf reads its form at run time."""

    def __init__(self, runtime):
        self.runtime = runtime

    def __enter__(self):
        from mlx_mcmc_amd import _lib

        if self.runtime:
            _lib.load().mc_debug_lanes_forms(0)

    def __exit__(self, *a):
        from mlx_mcmc_amd import _lib

        if self.runtime:
            _lib.load().mc_debug_lanes_forms(1)


def _hmc_state(prog, q0, splits, L, runtime, eps):
    """Everything an HMC run of sum(splits) iterations leaves behind."""
    import torch

    from mlx_mcmc_amd import _engine

    n = sum(splits)
    cfg = dict(chain_offset=0, num_warmup=n // 2, num_samples=n - n // 2, sample_begin=0,
               sample_capacity=n - n // 2, seed=5, step_size=eps, target_accept=0.8,
               num_leapfrog_steps=L, adapt_step_size=True)
    with _forms(runtime):
        cs = _engine.ChainSet(prog, C, q0, eps)
        out = torch.zeros((C, n - n // 2, prog.D), dtype=torch.float32, device=cs.device)
        it = 0
        for k in splits:
            cs.run_hmc(samples=out, iter_begin=it, iter_count=k, **cfg)
            it += k
        torch.cuda.synchronize()
        cs.check_status()
    sc = cs.scalars()
    return {"samples": out.cpu().numpy(), "q": cs.positions().cpu().numpy(),
            "g": cs.gradients().cpu().numpy(), "logp": sc["logp"].copy(),
            "step_size": sc["step_size"].copy(),
            "n_accept": sc["n_accept"] + sc["warmup_accept"],
            "n_total": sc["n_total"] + sc["warmup_total"]}


def _check(prog, q0, data, eps, what):
    n = sum(SPLITS)
    for runtime in (False, True):
        for L in STEPS:
            w = f"{what} runtime={runtime} L={L}"
            one = _hmc_state(prog, q0, (n,), L, runtime, eps)
            print(f"{w}: accepted {one['n_accept'].tolist()} of {n}")
            assert np.all(one["n_total"] == n), w
            assert np.all(one["n_accept"] >= 1), w + ": every chain must have moved"
            assert one["n_accept"].sum() < C * n, w + ": no proposal was rejected"
            check_state(one["q"], one["g"], one["logp"], data, what=w)
            parts = _hmc_state(prog, q0, SPLITS, L, runtime, eps)
            for k in one:
                assert one[k].tobytes() == parts[k].tobytes(), f"{w}: {k} differs over splits"


@pytest.mark.parametrize("name,order,shift,eps", CASES)
def test_state_against_f64_and_launch_splits(gpu, monkeypatch, name, order, shift, eps):
    from mlx_mcmc_amd import _trace

    key = (name, order, shift)
    lp, init, data = _model(*key)
    if key not in _progs:
        monkeypatch.setenv("MC_LANES_REP", "1")   # (read when the lanes are planned)
        _progs[key] = _trace.compile_model(lp, init, slices=1, slice_kernel="lanes")
    prog = _progs[key]
    assert prog.slice_kernel == "lanes" and prog.lanes_fast, prog.kernel_note
    assert prog.num_slices <= 1 and (prog.lane_slots, prog.lane_rep) == (1, 1)
    _check(prog, prog.layout.flatten(init), data, eps, f"{name} {order} +{shift:g}")


def test_small_shape_as_planned_two_slices(gpu):
    """rep > 1: each of a parameter's lanes forms the constants of its own
    part of the run; their first moments are summed over the lane group."""
    from mlx_mcmc_amd import _trace

    G, N = W.SHAPES["small"]
    lp, init = W.hierarchical(W.ns_product(), G, N)
    y, group = W.hierarchical_data(G, N)
    prog = _trace.compile_model(lp, init, slices=2, slice_kernel="lanes")
    assert prog.slice_kernel == "lanes" and prog.lanes_fast and prog.num_slices == 2
    assert prog.lane_rep > 1, prog.lane_rep
    _check(prog, prog.layout.flatten(init), {"y": y, "group": group, "G": G}, EPS_SMALL,
           "small, 2 slices")
