"""nuts(nuts_kernel="glm"): the tree step k_glm_nuts_step (csrc/glm_nuts.h) on the
MFMA gradient kernel, against the oracle's NUTS (oracle/samplers.py, reference
nuts.py:137-319) under the near-tie rules of
test_gpu_nuts_trace.py::test_nuts_large_shape_against_oracle."""
import functools

import numpy as np
import pytest

import _glm
from oracle import samplers as S

pytestmark = pytest.mark.gpu

W_, S_, SEED = 20, 10, 3  # warmup, kept draws, seed of the oracle comparisons
CASES = {"bernoulli": (97, 5, 0.15), "normal": (97, 5, 0.04), "poisson": (97, 33, 0.05)}


def _run(family, slices, adapt, **kw):
    import mlx_mcmc_amd as m

    N, P, eps = CASES[family]
    lp_fn, init = _glm.model(_glm.ns_product(), _glm.data(family, N, P))
    _, _, info = m.nuts(lp_fn, init, num_samples=S_, num_warmup=W_, step_size=eps,
                        max_tree_depth=6, adapt_step_size=adapt, key=m.random.key(SEED),
                        num_chains=4, progress=False, return_info=True, return_trace=True,
                        keep_on_device=True, nuts_kernel="glm", num_slices=slices, **kw)
    assert info.extra["kernel"] == "glm" and info.extra["glm_slices"] == slices
    return info


@functools.lru_cache(maxsize=None)
def _oracle(family, chain, step_sizes=None):
    N, P, eps = CASES[family]
    olp, init = _glm.model(_glm.ns_torch(), _glm.data(family, N, P))
    return S.nuts(olp, init, num_samples=S_, num_warmup=W_, step_size=eps, max_tree_depth=6,
                  adapt_step_size=False, seed=SEED, chain=chain, step_sizes=step_sizes)


def _ulp(x):
    return float(np.spacing(np.float32(abs(x))))


def _compare(name, info, refs):
    """Per chain: trees equal to the oracle's up to the first difference, which
    its own margins must prove a near-tie; before it H0, alpha and the kept
    draws.  Returns the depths compared."""
    n, tr, D = W_ + S_, info.trace, info.device_samples.shape[-1]
    total, depths = 0, []
    for c, ref in enumerate(refs):
        rt = {k: np.asarray(v) for k, v in ref.trace.items()}
        gd, gl = tr["tree_depth"][c], tr["n_leapfrog"][c]
        same = next((i for i in range(n) if gd[i] != rt["depth"][i] or gl[i] != rt["leaves"][i]), n)
        h_drift = np.abs(tr["energy"][c][:n].astype(np.float64) - rt["energy"][:n])
        ties = np.array([8 * _ulp(abs(rt["energy"][i]) + D) + 4 * h_drift[i] for i in range(n)])
        print(f"{name} chain {c}: trees identical for {same} of {n}, depths "
              f"{rt['depth'][:same].tolist()}, H0 drift max {h_drift[:max(same, 1)].max():.3g}")
        if same < n:
            i = same
            tie_dot = 1e-5 + 4 * h_drift[i] / max(abs(rt["energy"][i]), 1.0)
            assert (rt["slice_gap"][i] <= ties[i] or rt["div_gap"][i] <= ties[i]
                    or rt["uturn_margin"][i] <= tie_dot), (
                f"{name} chain {c}: trees differ at {i} without a near-tie (gpu {gd[i]}/{gl[i]}, "
                f"oracle {rt['depth'][i]}/{rt['leaves'][i]}; margins {rt['slice_gap'][i]:.3g} "
                f"{rt['div_gap'][i]:.3g} {rt['uturn_margin'][i]:.3g}, tie {ties[i]:.3g})")
        assert np.all(h_drift[:same] <= 1e-5 * (np.abs(rt["energy"][:same]) + D)), h_drift
        ga, ra = tr["accept_stat"][c][:same].astype(np.float64), rt["alpha"][:same]
        assert np.all(np.abs(ga - ra) <= ra * np.expm1(ties[:same]) + 1e-5), (ga, ra)
        ns = max(0, same - W_)
        np.testing.assert_allclose(info.device_samples[c, :ns].cpu().numpy(), ref.samples[:ns],
                                   rtol=1e-4, atol=1e-5, err_msg=f"{name} chain {c}: draws")
        assert same >= 6, f"{name} chain {c}: compared only {same}"
        total += same
        depths += rt["depth"][:same].tolist()
    assert total >= 0.7 * len(refs) * n, f"{name}: only {total} chain-iterations compared"
    return depths


@pytest.mark.parametrize("slices", [1, 3])
@pytest.mark.parametrize("family", list(CASES))
def test_trees_match_oracle(gpu, family, slices):
    """Fixed step size: the first two cases give depths 2-5 that differ between
    the chains of the block (they sit in different iterations of a tick); the
    Poisson case reaches the depth cap 6, a second coefficient tile and the
    offset."""
    info = _run(family, slices, adapt=False)
    np.testing.assert_array_equal(info.trace["step_size"], CASES[family][2])
    depths = _compare(family, info, [_oracle(family, c) for c in range(4)])
    assert max(depths) >= (6 if family == "poisson" else 3)


def test_dual_averaging_replay(gpu):
    """Adaptation on: the GPU's step sizes are dual averaging of its own
    accept_stat, and the oracle replayed with them builds the same trees."""
    info = _run("bernoulli", 1, adapt=True)
    eps0, refs = CASES["bernoulli"][2], []
    for c in range(4):
        g_eps = info.trace["step_size"][c].astype(np.float64)
        da, eps_bar = S.dual_averaging_steps(info.trace["accept_stat"][c], eps0, W_)
        np.testing.assert_allclose(g_eps[:W_], da, rtol=1e-4, err_msg=f"chain {c}: dual averaging")
        np.testing.assert_allclose(g_eps[W_:], eps_bar, rtol=1e-4, err_msg=f"chain {c}: eps-bar")
        refs.append(_oracle("bernoulli", c, tuple(g_eps)))
    assert max(_compare("bernoulli/adapt", info, refs)) >= 3


def test_chains_do_not_depend_on_the_split(gpu):
    """40 chains in one call, as 33 + 7 through chain_offset, and cut into the
    launch windows [0, 7) and [7, 20): the same bytes per global chain (the
    asynchronous ticks, and what survives a window boundary)."""
    import torch

    import mlx_mcmc_amd as m
    from mlx_mcmc_amd import _engine, _trace

    lp_fn, init = _glm.model(_glm.ns_product(), _glm.data("poisson", 97, 33))
    kw = dict(num_samples=6, num_warmup=14, step_size=0.05, max_tree_depth=5,
              key=m.random.key(9), num_slices=3, nuts_kernel="glm")

    def run(C, off=0):
        s, _ = m.nuts(lp_fn, init, num_chains=C, chain_offset=off, progress=False, **kw)
        return np.concatenate([s["a"].reshape(C, 6, 1), s["beta"]], axis=2)

    whole = run(40)
    assert np.isfinite(whole).all() and np.ptp(whole[:, :, 1]) > 0
    assert whole.tobytes() == np.concatenate([run(33), run(7, off=33)]).tobytes()
    prog = _trace.compile_model(lp_fn, init, slices=3)
    chains = _engine.ChainSet(prog, 40, prog.layout.flatten(init), kw["step_size"])
    cut = torch.empty((40, 6, prog.D), dtype=torch.float32, device=chains.device)
    for a, n in ((0, 7), (7, 13)):
        chains.run_nuts_glm(samples=cut, iter_begin=a, iter_count=n, chain_offset=0, num_warmup=14,
                            num_samples=6, sample_begin=0, sample_capacity=6, seed=kw["key"].seed,
                            step_size=kw["step_size"], target_accept=0.65, adapt_step_size=True,
                            max_tree_depth=5)
    assert whole.tobytes() == cut.cpu().numpy().tobytes()


@pytest.mark.parametrize("maxj", [0, 1])
@pytest.mark.parametrize("N,P,C", [(1, 1, 1), (64, 256, 3)])
def test_edges(gpu, N, P, C, maxj):
    """The smallest program and the register cap at the two smallest depth
    caps.  nuts.h: the tree grows until s fails or the cap, so here it ends at
    the cap, and a tree that ends at depth j has built the subtrees of depths
    0 .. j - 1: 2^j - 1 leaves unless one stopped early, which a one-leaf
    subtree cannot."""
    import mlx_mcmc_amd as m

    lp_fn, init = _glm.model(_glm.ns_product(), _glm.data("bernoulli", N, P))
    s, _, info = m.nuts(lp_fn, init, num_samples=2, num_warmup=1, step_size=0.1,
                        max_tree_depth=maxj, key=m.random.key(1), num_chains=C, progress=False,
                        return_info=True, return_trace=True, nuts_kernel="glm")
    assert all(np.isfinite(np.asarray(v)).all() for v in s.values())
    depth, leaves = info.trace["tree_depth"], info.trace["n_leapfrog"]
    assert depth.shape == (C, 3) and np.all(depth == maxj)
    assert np.all(leaves == 2 ** depth - 1)
    assert np.array_equal(info.n_grad, 1 + leaves.sum(axis=1))
