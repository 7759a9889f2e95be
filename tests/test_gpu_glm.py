"""Design-matrix GLMs on the FP32 MFMA kernels (csrc/glm.h): the gradient
kernel against the float64 closed form, hmc() against the oracle sampler, and
the independence of a chain's draws from how the chains are split."""
import numpy as np
import pytest

import _glm
from _near_tie import compare_trace, log_u
from oracle import samplers as S

pytestmark = pytest.mark.gpu

# (N, P, C, S): one exact tile (pins the operand layouts); all-masked edges;
# ragged in every dimension; second p-tile, second chain block, slices with
# unequal tile counts; the register cap
SHAPES = [(32, 2, 32, 1), (1, 1, 1, 1), (33, 3, 5, 1), (97, 33, 33, 3), (64, 256, 3, 2)]


@pytest.mark.parametrize("N,P,C,S", SHAPES)
@pytest.mark.parametrize("family", _glm.FAMILIES)
def test_logp_grad_matches_f64(gpu, family, N, P, C, S):
    """The gate of the expression gradients (tests/test_gpu_expr.py): |lp - ref|
    <= 1e-5 max(1, |ref|), gradients rtol 2e-4, atol 2e-5 max(1, max |g|).  The
    same closed form in float32 NumPy sits inside it at every shape here (worst
    lp 0.027 of the bound, worst gradient 0.004: checked on the CPU)."""
    from mlx_mcmc_amd import _engine, _trace

    d = _glm.data(family, N, P)
    lp_fn, init = _glm.model(_glm.ns_product(), d)
    prog = _trace.compile_model(lp_fn, init, slices=S)
    assert prog.slice_kernel == "glm" and prog.glm_slices(C) == S
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
@pytest.mark.parametrize("family,eps,seed", [("bernoulli", 0.35, 3), ("normal", 0.07, 11)])
def test_hmc_matches_oracle(gpu, family, eps, seed, S_):
    """Decisions, ratios, energies and step sizes of every chain equal the
    oracle's HMC until a proven near-tie (tests/_near_tie.py)."""
    import mlx_mcmc_amd as m

    d = _glm.data(family, 97, 5)
    lp_fn, init = _glm.model(_glm.ns_product(), d)
    olp, _ = _glm.model(_glm.ns_torch(), d)
    kw = dict(num_samples=15, num_warmup=15, step_size=eps, num_leapfrog_steps=10)
    _, _, info = m.hmc(lp_fn, init, key=m.random.key(seed), num_chains=4, progress=False,
                       return_info=True, return_trace=True, num_slices=S_, **kw)
    assert info.extra["kernel"] == "glm" and info.extra["glm_slices"] == S_
    tr, n, total, acc = info.trace, 30, 0, []
    for c in range(4):
        ref = S.hmc(olp, init, seed=seed, chain=c, **kw)
        gpu_c = {"accepted": tr["accepted"][c][:n], "ratio": tr["accept_stat"][c][:n],
                 "step_size": tr["step_size"][c][:n], "energy": tr["energy"][c][:n]}
        ref_c = {k: np.asarray(ref.trace[k])[:n] for k in ("accepted", "ratio", "step_size",
                                                            "energy")}
        ref_c["log_u"] = log_u(seed, c, n)
        same = compare_trace(gpu_c, ref_c, f"{family} chain {c}", verbose=True)
        assert same >= 5, f"{family} chain {c}: compared only {same}"
        total += same
        acc += list(ref_c["accepted"])
    assert total >= 0.7 * 4 * n, f"{family}: only {total} of {4 * n} iterations compared"
    assert any(acc) and not all(acc)


def test_chains_do_not_depend_on_the_split(gpu):
    """40 chains in one call, as 33 + 7 through chain_offset, and with the run
    cut into two launches mid-warmup: the same bytes per global chain."""
    import torch

    import mlx_mcmc_amd as m
    from mlx_mcmc_amd import _engine, _trace

    d = _glm.data("poisson", 97, 33)
    lp_fn, init = _glm.model(_glm.ns_product(), d)
    kw = dict(num_samples=6, num_warmup=14, step_size=0.05, num_leapfrog_steps=4,
              key=m.random.key(9), num_slices=3)

    def run(C, off=0):
        s, _ = m.hmc(lp_fn, init, num_chains=C, chain_offset=off, progress=False, **kw)
        return np.concatenate([s["a"].reshape(C, 6, 1), s["beta"]], axis=2)

    whole = run(40)
    assert np.isfinite(whole).all() and np.ptp(whole[:, :, 1]) > 0
    split = np.concatenate([run(33), run(7, off=33)])
    assert whole.tobytes() == split.tobytes()
    # the same run as two launches, iterations [0, 7) and [7, 20)
    prog = _trace.compile_model(lp_fn, init, slices=3)
    chains = _engine.ChainSet(prog, 40, prog.layout.flatten(init), kw["step_size"])
    cut = torch.empty((40, 6, prog.D), dtype=torch.float32, device=chains.device)
    for a, n in ((0, 7), (7, 13)):
        chains.run_hmc(samples=cut, iter_begin=a, iter_count=n, chain_offset=0, num_warmup=14,
                       num_samples=6, sample_begin=0, sample_capacity=6, seed=kw["key"].seed,
                       step_size=kw["step_size"], target_accept=0.8, adapt_step_size=True,
                       num_leapfrog_steps=4)
    assert whole.tobytes() == cut.cpu().numpy().tobytes()
