"""glm_kernel="wide": the column-split MFMA gradient kernel k_glm_grad_wide
(csrc/glm_wide.h) against the float64 closed form, hmc() on it against the oracle
sampler, and the independence of a chain's draws from how the chains are split
under hmc() and nuts(nuts_kernel="glm")."""
import numpy as np
import pytest

import _glm
from _near_tie import compare_trace, log_u
from oracle import samplers as S

pytestmark = pytest.mark.gpu

# (N, P, C, S): the first column past the narrow cap (PTW 3, one exact row tile,
# three idle waves); all masked; ragged everywhere, the second wave's columns
# start inside the data; slices of three tiles, a partly filled round, a second
# chain block; the cap (coefficient chunks, a full round then a partial one: both
# r buffers); P rounded up to a PTW whose last tiles are all padding
SHAPES = [(32, 257, 32, 1), (1, 1, 1, 1), (33, 129, 5, 1), (161, 300, 33, 2),
          (161, 1024, 3, 1), (64, 640, 3, 2)]


@pytest.mark.parametrize("N,P,C,S", SHAPES)
@pytest.mark.parametrize("family", _glm.FAMILIES)
def test_logp_grad_matches_f64(gpu, family, N, P, C, S):
    """The gate of tests/test_gpu_glm.py: |lp - ref| <= 1e-5 max(1, |ref|),
    gradients rtol 2e-4, atol 2e-5 max(1, max |g|), two calls the same bytes.  The
    same closed form in float32 NumPy sits inside it at every shape here (worst
    lp 0.022 of the bound, worst gradient 0.005: checked on the CPU)."""
    from mlx_mcmc_amd import _engine, _trace

    d = _glm.data(family, N, P)
    lp_fn, init = _glm.model(_glm.ns_product(), d)
    prog = _trace.compile_model(lp_fn, init, slices=S, glm_kernel="wide")
    assert prog.slice_kernel == "glm" and prog.glm_slices(C) == S
    assert "k_glm_grad_wide" in prog.kernel_note
    q = np.random.default_rng(5).normal(size=(C, prog.D)).astype(np.float32)
    lp, g = _engine.logp_grad(prog, q)
    lp2, g2 = _engine.logp_grad(prog, q)
    lp, g = lp.cpu().numpy(), g.cpu().numpy()
    assert lp.tobytes() == lp2.cpu().numpy().tobytes() and g.tobytes() == g2.cpu().numpy().tobytes()
    rlp, rg = _glm.closed_form(d, q)
    err = np.abs(lp - rlp) / np.maximum(1.0, np.abs(rlp))
    print(f"{family} {N}x{P} C={C} S={S}: lp err {err.max():.2e}, "
          f"grad err {np.abs(g - rg).max():.2e} (max |g| {np.abs(rg).max():.2e})")
    assert np.all(err <= 1e-5)
    np.testing.assert_allclose(g, rg, rtol=2e-4, atol=2e-5 * max(1.0, np.abs(rg).max()))


@pytest.mark.parametrize("S_", [1, 3])
def test_hmc_matches_oracle(gpu, S_):
    """The scheme of test_gpu_glm.py::test_hmc_matches_oracle at (97, 260).  The
    step size 0.4 was chosen on the CPU from the oracle's chains alone: of their
    30 iterations they accept 23, 12, 17 and 19 (0.3 accepts nearly all, 0.5
    leaves one chain without an accept)."""
    import mlx_mcmc_amd as m

    seed, eps = 3, 0.4
    d = _glm.data("bernoulli", 97, 260)
    lp_fn, init = _glm.model(_glm.ns_product(), d)
    olp, _ = _glm.model(_glm.ns_torch(), d)
    kw = dict(num_samples=15, num_warmup=15, step_size=eps, num_leapfrog_steps=10)
    _, _, info = m.hmc(lp_fn, init, key=m.random.key(seed), num_chains=4, progress=False,
                       return_info=True, return_trace=True, num_slices=S_, glm_kernel="wide", **kw)
    assert info.extra["kernel"] == "glm" and info.extra["glm_slices"] == S_
    assert info.extra["glm_kernel"] == "wide"
    tr, n, total, acc = info.trace, 30, 0, []
    for c in range(4):
        ref = S.hmc(olp, init, seed=seed, chain=c, **kw)
        gpu_c = {"accepted": tr["accepted"][c][:n], "ratio": tr["accept_stat"][c][:n],
                 "step_size": tr["step_size"][c][:n], "energy": tr["energy"][c][:n]}
        ref_c = {k: np.asarray(ref.trace[k])[:n] for k in ("accepted", "ratio", "step_size",
                                                            "energy")}
        ref_c["log_u"] = log_u(seed, c, n)
        same = compare_trace(gpu_c, ref_c, f"chain {c}", verbose=True)
        assert same >= 5, f"chain {c}: compared only {same}"
        total += same
        acc += list(ref_c["accepted"])
    assert total >= 0.7 * 4 * n, f"only {total} of {4 * n} iterations compared"
    assert any(acc) and not all(acc)


@pytest.mark.parametrize("sampler", ["hmc", "nuts"])
def test_chains_do_not_depend_on_the_split(gpu, sampler):
    """40 chains in one call, as 33 + 7 through chain_offset, and cut into the
    launch windows [0, 7) and [7, 20): the same bytes per global chain."""
    import torch

    import mlx_mcmc_amd as m
    from mlx_mcmc_amd import _engine, _trace

    lp_fn, init = _glm.model(_glm.ns_product(), _glm.data("poisson", 97, 300))
    kw = dict(num_samples=6, num_warmup=14, step_size=0.05, key=m.random.key(9), num_slices=3,
              glm_kernel="wide")
    if sampler == "hmc":
        call, kw["num_leapfrog_steps"] = m.hmc, 4
        own = dict(num_leapfrog_steps=4, target_accept=0.8)
    else:
        call, kw["max_tree_depth"], kw["nuts_kernel"] = m.nuts, 3, "glm"
        own = dict(max_tree_depth=3, target_accept=0.65)

    def run(C, off=0):
        s, _ = call(lp_fn, init, num_chains=C, chain_offset=off, progress=False, **kw)
        return np.concatenate([s["a"].reshape(C, 6, 1), s["beta"]], axis=2)

    whole = run(40)
    assert np.isfinite(whole).all() and np.ptp(whole[:, :, 1]) > 0
    assert whole.tobytes() == np.concatenate([run(33), run(7, off=33)]).tobytes()
    prog = _trace.compile_model(lp_fn, init, slices=3, glm_kernel="wide")
    chains = _engine.ChainSet(prog, 40, prog.layout.flatten(init), kw["step_size"])
    cut = torch.empty((40, 6, prog.D), dtype=torch.float32, device=chains.device)
    launch = chains.run_hmc if sampler == "hmc" else chains.run_nuts_glm
    for a, n in ((0, 7), (7, 13)):
        launch(samples=cut, iter_begin=a, iter_count=n, chain_offset=0, num_warmup=14,
               num_samples=6, sample_begin=0, sample_capacity=6, seed=kw["key"].seed,
               step_size=kw["step_size"], adapt_step_size=True, **own)
    assert whole.tobytes() == cut.cpu().numpy().tobytes()
