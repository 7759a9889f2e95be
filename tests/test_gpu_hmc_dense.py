"""The dense HMC route (lanes_fast.h k_hmc_lf DN, run_lanes.h launch_hmc_dense):
under automatic slicing a fast-form hierarchical program runs a chain pair per
workgroup — one wave without an exchange, or 4 / 8 waves of two register slots
exchanging their records through LDS with one barrier per step.

Models (tests/_ragged.py's hierarchical Normal over explicit run lengths):
  g300   G = 300, N = 3000: more private parameters than a wave's 4 slots
         hold, 4 waves (75 parameters each) exchanging through LDS;
  g600   G = 600, N = 6000, ragged runs of 5..15 with an empty and a
         one-element group: 8 waves;
  g40    G = 40, N = 2400: one wave, no exchange.
C = 3 chains (the last pair holds a dead chain), 6 iterations, L = 1, 2, 3 and
5 (the only step; first + last; an aligning or trailing step; the paired
bodies).

  * the state against the closed form in float64 within _ragged.bounds;
  * launches of 1 + 2 + 3 iterations byte-identical to one launch;
  * a chain_offset shard — the last chain alone, its pair's other chain dead
    as in the whole run — equal to the same chain of the whole run;
  * against the exchange kernel of the same build (an explicit slice count) by
    tests/_near_tie.py compare_trace: decisions equal up to a proven near-tie,
    at most one chain may stop there, draws of the agreeing prefix at
    rtol 1e-3 / atol 1e-4;
  * after a dense HMC launch, a NUTS launch on the same chains runs the
    program-level sliced kernel and passes its status check.
"""
import numpy as np
import pytest

import workloads as W
from _near_tie import compare_trace, log_u
from _ragged import _evaluate, check_state, perturbed_points, ragged_hier

pytestmark = pytest.mark.gpu

C = 3
STEPS = (1, 2, 3, 5)
SPLITS = (1, 2, 3)
_R600 = [0, 1] + [5 + (7 * i) % 11 for i in range(598)]
_R600[-1] += 6000 - sum(_R600)
# name -> (run lengths, data order, (dense slices, slots), explicit slices, step size):
# about 1.5 / sqrt(2 N), one and a half posterior standard deviations of sigma
# (g600: half of that — with its short runs the longer trajectories of the
# larger step are rejected in every chain, and nothing would be compared)
MODELS = {"g300": ([10] * 300, "sorted", (4, 2), 4, 0.019),
          "g600": (_R600, "shuffled", (8, 2), 8, 0.007),
          "g40": ([60] * 40, "sorted", (1, 1), 2, 0.0217)}
_models, _progs = {}, {}


def _model(name):
    if name not in _models:
        lengths, order = MODELS[name][:2]
        _models[name] = ragged_hier(W.ns_product(), lengths, order=order)
    return _models[name]


def _program(name):
    from mlx_mcmc_amd import _trace

    if name not in _progs:
        lp, init, _ = _model(name)
        _progs[name] = _trace.compile_model(lp, init)
    prog = _progs[name]
    assert prog.slice_kernel == "lanes" and prog.lanes_fast, prog.kernel_note
    assert prog.hmc_dense == MODELS[name][2], prog.hmc_dense
    return prog


def _hmc_state(prog, q0, splits, L, eps, chains=C, offset=0):
    import torch

    from mlx_mcmc_amd import _engine

    n = sum(splits)
    cfg = dict(chain_offset=offset, num_warmup=n // 2, num_samples=n - n // 2, sample_begin=0,
               sample_capacity=n - n // 2, seed=5, step_size=eps, target_accept=0.8,
               num_leapfrog_steps=L, adapt_step_size=True)
    cs = _engine.ChainSet(prog, chains, q0, eps)
    out = torch.zeros((chains, n - n // 2, prog.D), dtype=torch.float32, device=cs.device)
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


@pytest.mark.parametrize("name", sorted(MODELS))
def test_state_splits_and_shards(gpu, name):
    prog = _program(name)
    _, init, data = _model(name)
    q0, eps, n = prog.layout.flatten(init), MODELS[name][4], sum(SPLITS)
    for L in STEPS:
        w = f"{name} L={L}"
        one = _hmc_state(prog, q0, (n,), L, eps)
        print(f"{w}: accepted {one['n_accept'].tolist()} of {n}")
        assert np.all(one["n_total"] == n), w
        assert one["n_accept"].sum() >= 1, w + ": no chain moved"
        check_state(one["q"], one["g"], one["logp"], data, what=w)
        parts = _hmc_state(prog, q0, SPLITS, L, eps)
        for k in one:
            assert one[k].tobytes() == parts[k].tobytes(), f"{w}: {k} differs over splits"
        for off, cnt in ((2, 1),):
            shard = _hmc_state(prog, q0, (n,), L, eps, chains=cnt, offset=off)
            for k in one:
                assert one[k][off:off + cnt].tobytes() == shard[k].tobytes(), \
                    f"{w}: {k} of chains {off}..{off + cnt - 1} differs in their shard"


def _hmc(name, slices, L):
    import mlx_mcmc_amd as m

    lp, init, _ = _model(name)
    s, _, info = m.hmc(lp, init, num_samples=3, num_warmup=3, step_size=MODELS[name][4],
                       num_leapfrog_steps=L, key=m.random.key(3), num_chains=C,
                       progress=False, return_info=True, return_trace=True, num_slices=slices)
    assert info.extra["kernel"] == "lanes", info.extra
    return s, info


@pytest.mark.parametrize("name", sorted(MODELS))
def test_matches_exchange_kernel(gpu, name):
    _program(name)      # (asserts that the automatic plan takes the dense route)
    _, init, data = _model(name)
    n = 6
    lu = [log_u(3, c, n) for c in range(C)]
    hs = float(_evaluate(data, perturbed_points(init, n=1)[0], None, np.float64, mags=True)[0])
    for L in STEPS:
        a, ia = _hmc(name, MODELS[name][3], L)      # explicit slices: the exchange kernel
        b, ib = _hmc(name, 0, L)                    # automatic: dense
        assert ia.trace["accepted"].any(), "the chains must move"
        full = 0
        for c in range(C):
            what = f"{name} L={L} chain {c}"
            r = {"accepted": ia.trace["accepted"][c], "ratio": ia.trace["accept_stat"][c],
                 "energy": ia.trace["energy"][c], "step_size": ia.trace["step_size"][c],
                 "log_u": lu[c]}
            g = {"accepted": ib.trace["accepted"][c], "ratio": ib.trace["accept_stat"][c],
                 "energy": ib.trace["energy"][c], "step_size": ib.trace["step_size"][c]}
            same = compare_trace(g, r, what, h_scale=hs)
            full += same == n
            ns = max(0, same - 3)       # draws of the agreeing prefix (3 warmup iterations)
            for k in a:
                np.testing.assert_allclose(b[k][c, :ns], a[k][c, :ns], rtol=1e-3, atol=1e-4,
                                           err_msg=f"{what} {k}")
        assert full >= C - 1, f"{name} L={L}: only {full} of {C} chains agree to the end"


def test_nuts_after_dense_hmc_runs_the_sliced_kernel(gpu):
    import torch

    from mlx_mcmc_amd import _engine

    prog = _program("g300")
    assert prog.num_slices == 4 and prog.nuts_kernel(3) == "sliced", \
        (prog.num_slices, prog.nuts_kernel(3))
    _, init, data = _model("g300")
    eps = MODELS["g300"][4]
    cs = _engine.ChainSet(prog, C, prog.layout.flatten(init), eps)
    cfg = dict(chain_offset=0, num_warmup=2, num_samples=2, sample_begin=0, sample_capacity=2,
               seed=5, step_size=eps, target_accept=0.8, adapt_step_size=True)
    cs.run_hmc(iter_begin=0, iter_count=4, num_leapfrog_steps=3, **cfg)
    cs.check_status()
    cs.run_nuts(iter_begin=0, iter_count=4, max_tree_depth=3, **cfg)
    torch.cuda.synchronize()
    cs.check_status()
    sc = cs.scalars()
    check_state(cs.positions().cpu().numpy(), cs.gradients().cpu().numpy(), sc["logp"].copy(),
                data, what="g300 after HMC then NUTS")
