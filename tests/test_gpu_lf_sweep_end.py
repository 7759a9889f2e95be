"""The end of k_hmc_lf's moment sweep (lanes_fast.h lf_moments_pre): the
whole groups and the masked tail after a run's last full round, at one to
six rounds (tests/_lf_ends.py has the cases: zero to three whole groups after
the rounds, tails from nothing to five groups, the benchmark's runs of
100 / 101; tests/_lf_rounds.py's runs never leave a whole group there).

A group not summed, summed twice or masked at the wrong length shows as
observations missing or doubled at the end of a run: the float64 bounds see
one (tests/test_lf_ends_reference.py).

12 groups on one slice with one lane per parameter (MC_LANES_REP=1), the
compile-time form (lf_moments_pre) and the run-time form (lf_moments' own
round loop on the same runs), L = 1, 2, 3, 5 leapfrog steps (the only step;
first and last; one aligning or trailing step between them; the paired bodies
and one more: every sweep site, and the lane RNG plan's draws made an
iteration ahead in the last step).  Four chains, six iterations.

  * the state (position, gradient, log p) against the closed form in float64
    within _ragged.bounds;
  * one launch against launches of 1 + 2 + 3 iterations: byte-identical (a
    launch's first draws are made ahead of its loop, every later iteration's
    in the last step of the one before);
  * against the term interpreter (k_hmc on one slice), as
    tests/test_gpu_lf_sweep_pipeline.py compares: step sizes equal, every
    iteration's log ratio and H within 8 ulp of |H| and the decisions equal
    up to a proven near-tie (tests/_near_tie.py compare_trace); at most one
    chain of four may stop at such a tie; draws of the agreeing prefix
    rtol 1e-3 / atol 1e-4.
"""
import numpy as np
import pytest

import workloads as W
from _lf_ends import CASES, ENDS
from _near_tie import compare_trace, log_u
from _ragged import _evaluate, check_state, perturbed_points, ragged_hier

pytestmark = pytest.mark.gpu

C = 4
STEPS = (1, 2, 3, 5)
SPLITS = (1, 2, 3)
_models, _progs = {}, {}


def _model(name, order):
    if (name, order) not in _models:
        _models[name, order] = ragged_hier(W.ns_product(), ENDS[name][0], order=order)
    return _models[name, order]


def _program(name, order, monkeypatch):
    from mlx_mcmc_amd import _trace

    key = (name, order)
    if key not in _progs:
        monkeypatch.setenv("MC_LANES_REP", "1")   # (read when the lanes are planned)
        lp, init, data = _model(name, order)
        _progs[key] = _trace.compile_model(lp, init, slices=1, slice_kernel="lanes")
    prog = _progs[key]
    assert prog.slice_kernel == "lanes" and prog.lanes_fast, prog.kernel_note
    assert prog.num_slices <= 1 and (prog.lane_slots, prog.lane_rep) == (1, 1)
    return prog


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


def _hmc_state(prog, init, splits, L, runtime, eps=0.02):
    """Everything an HMC run of sum(splits) iterations leaves behind."""
    import torch

    from mlx_mcmc_amd import _engine

    n = sum(splits)
    cfg = dict(chain_offset=0, num_warmup=n // 2, num_samples=n - n // 2, sample_begin=0,
               sample_capacity=n - n // 2, seed=5, step_size=eps, target_accept=0.8,
               num_leapfrog_steps=L, adapt_step_size=True)
    with _forms(runtime):
        cs = _engine.ChainSet(prog, C, prog.layout.flatten(init), eps)
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


@pytest.mark.parametrize("name,order", CASES)
def test_state_against_f64_and_launch_splits(gpu, monkeypatch, name, order):
    prog = _program(name, order, monkeypatch)
    _, init, data = _model(name, order)
    n = sum(SPLITS)
    for runtime in (False, True):
        for L in STEPS:
            what = f"{name} {order} runtime={runtime} L={L}"
            one = _hmc_state(prog, init, (n,), L, runtime)
            assert np.all(one["n_total"] == n), what
            assert np.all(one["n_accept"] >= 1), what + ": every chain must have moved"
            check_state(one["q"], one["g"], one["logp"], data, what=what)
            parts = _hmc_state(prog, init, SPLITS, L, runtime)
            for k in one:
                assert one[k].tobytes() == parts[k].tobytes(), f"{what}: {k} differs over splits"


def _hmc(name, order, kernel, L, runtime=False):
    import mlx_mcmc_amd as m

    lp, init, _ = _model(name, order)
    with _forms(runtime):
        s, _, info = m.hmc(lp, init, num_samples=3, num_warmup=3, step_size=0.02,
                           num_leapfrog_steps=L, key=m.random.key(3), num_chains=C,
                           progress=False, return_info=True, return_trace=True,
                           num_slices=1, slice_kernel=kernel)
    assert info.extra["kernel"] == ("lanes" if kernel == "lanes" else "unsliced"), info.extra
    return s, info


def _h_scale(name, order):
    """The magnitude of log p's summands at the start (tests/_near_tie.py h_scale)."""
    _, init, data = _model(name, order)
    q0 = perturbed_points(init, n=1)[0]
    return float(_evaluate(data, q0, None, np.float64, mags=True)[0])


@pytest.mark.parametrize("name,order", CASES)
def test_matches_term_interpreter(gpu, monkeypatch, name, order):
    monkeypatch.setenv("MC_LANES_REP", "1")
    n = 6
    lu = [log_u(3, c, n) for c in range(C)]
    hs = _h_scale(name, order)
    for L in STEPS:
        a, ia = _hmc(name, order, "interpreter", L)
        assert ia.trace["accepted"].any(), "the chains must move"
        for runtime in (False, True):
            what = f"{name} {order} runtime={runtime} L={L}"
            b, ib = _hmc(name, order, "lanes", L, runtime)
            full = 0
            for c in range(C):
                r = {"accepted": ia.trace["accepted"][c], "ratio": ia.trace["accept_stat"][c],
                     "energy": ia.trace["energy"][c], "step_size": ia.trace["step_size"][c],
                     "log_u": lu[c]}
                g = {"accepted": ib.trace["accepted"][c], "ratio": ib.trace["accept_stat"][c],
                     "energy": ib.trace["energy"][c], "step_size": ib.trace["step_size"][c]}
                same = compare_trace(g, r, f"{what} chain {c}", h_scale=hs)
                full += same == n
                ns = max(0, same - 3)       # draws of the agreeing prefix (3 warmup iterations)
                for k in a:
                    np.testing.assert_allclose(b[k][c, :ns], a[k][c, :ns], rtol=1e-3, atol=1e-4,
                                               err_msg=f"{what} chain {c} {k}")
            assert full >= C - 1, f"{what}: only {full} of {C} chains agree to the end"
