"""Softmax regression on the class-packed MFMA gradient kernel
(csrc/glm_softmax.h): the gradient against the float64 closed form, hmc()
against the oracle sampler, and the independence of a chain's draws from how
the chains are split."""
import numpy as np
import pytest

import _glm_softmax as G
from _near_tie import compare_trace, log_u
from oracle import samplers as S

pytestmark = pytest.mark.gpu

# (N, P, K, C, S, q scale): one exact tile and a full block of Kp = 2 (pins the
# packing); all masked, one padded class; ragged, a second gradient block holding
# one chain; five gradient blocks feeding two step workgroups; PT = 2 and two
# slices; Kp = 32 with 15 padded classes; one chain per block (exchange distance
# 16); the cap, PT = 8; |eta| up to about 100 (a softmax without the max
# subtraction overflows f32 there)
SHAPES = [(32, 2, 2, 16, 1, 1.0), (1, 1, 3, 1, 1, 1.0), (33, 5, 3, 9, 1, 1.0),
          (33, 4, 4, 35, 1, 1.0), (161, 40, 8, 5, 2, 1.0), (40, 3, 17, 2, 1, 1.0),
          (97, 33, 32, 3, 1, 1.0), (64, 256, 5, 7, 2, 1.0), (33, 5, 3, 9, 1, 30.0)]


@pytest.mark.parametrize("intercept", [True, False])
@pytest.mark.parametrize("N,P,K,C,S_,scale", SHAPES)
def test_logp_grad_matches_f64(gpu, N, P, K, C, S_, scale, intercept):
    """The gate of tests/test_gpu_glm.py: |lp - ref| <= 1e-5 max(1, |ref|),
    gradients rtol 2e-4, atol 2e-5 max(1, max |g|).  The same closed form in
    float32 NumPy sits inside it at every shape here, with and without the
    intercepts (worst lp 0.012 of the bound, worst gradient 0.005: checked on the
    CPU), so no shape needs a wider bound."""
    from mlx_mcmc_amd import _engine, _trace

    d = G.data(N, P, K)
    lp_fn, init = G.model(G.ns_product(), d, intercept)
    prog = _trace.compile_model(lp_fn, init, slices=S_)
    assert prog.slice_kernel == "glm" and prog.glm_slices(C) == S_
    assert prog.D == P * K + (K if intercept else 0) and "k_glm_softmax_grad" in prog.kernel_note
    q = (scale * np.random.default_rng(5).normal(size=(C, prog.D))).astype(np.float32)
    lp, g = _engine.logp_grad(prog, q)
    lp2, g2 = _engine.logp_grad(prog, q)
    lp, g = lp.cpu().numpy(), g.cpu().numpy()
    assert lp.tobytes() == lp2.cpu().numpy().tobytes() and g.tobytes() == g2.cpu().numpy().tobytes()
    rlp, rg = G.closed_form(d, q, intercept)
    err = np.abs(lp - rlp) / np.maximum(1.0, np.abs(rlp))
    print(f"{N}x{P} K={K} C={C} S={S_} scale={scale}: lp err {err.max():.2e}, "
          f"grad err {np.abs(g - rg).max():.2e} (max |g| {np.abs(rg).max():.2e})")
    assert np.all(err <= 1e-5)
    np.testing.assert_allclose(g, rg, rtol=2e-4, atol=2e-5 * max(1.0, np.abs(rg).max()))


@pytest.mark.parametrize("S_", [1, 3])
def test_hmc_matches_oracle(gpu, S_):
    """Decisions, ratios, energies and step sizes of every chain equal the
    oracle's HMC until a proven near-tie (tests/_near_tie.py).  K = 3: a padded
    class.  The step size 0.25 comes from the oracle's chains alone: on the CPU
    they accept 27, 27, 25 and 27 of their 30 iterations with no log ratio below
    -2.1, so some reject and every trajectory is stable.  (0.15 accepts 116 of
    120; at 0.4 the oracle's own log ratios reach -163: leapfrog past its
    stability limit, where last-digit differences grow beyond the scheme's 8 ulp
    of H_init.)"""
    import mlx_mcmc_amd as m

    seed, eps, n = 3, 0.25, 30
    d = G.data(97, 5, 3)
    lp_fn, init = G.model(G.ns_product(), d)
    olp, _ = G.model(G.ns_torch(), d)
    kw = dict(num_samples=15, num_warmup=15, step_size=eps, num_leapfrog_steps=10)
    _, _, info = m.hmc(lp_fn, init, key=m.random.key(seed), num_chains=4, progress=False,
                       return_info=True, return_trace=True, num_slices=S_, **kw)
    assert info.extra["kernel"] == "glm" and info.extra["glm_slices"] == S_
    assert info.extra["glm_family"] == "categorical"
    tr, total, acc = info.trace, 0, []
    for c in range(4):
        ref = S.hmc(olp, init, seed=seed, chain=c, **kw)
        gpu_c = {"accepted": tr["accepted"][c][:n], "ratio": tr["accept_stat"][c][:n],
                 "step_size": tr["step_size"][c][:n], "energy": tr["energy"][c][:n]}
        ref_c = {k: np.asarray(ref.trace[k])[:n] for k in ("accepted", "ratio", "step_size",
                                                            "energy")}
        ref_c["log_u"] = log_u(seed, c, n)
        same = compare_trace(gpu_c, ref_c, f"softmax chain {c}", verbose=True)
        assert same >= 5, f"chain {c}: compared only {same}"
        total += same
        acc += list(ref_c["accepted"])
    assert total >= 0.7 * 4 * n, f"only {total} of {4 * n} iterations compared"
    assert any(acc) and not all(acc)


def test_chains_do_not_depend_on_the_split(gpu):
    """40 chains in one call, as 33 + 7 through chain_offset, and with the run
    cut into two launches mid-warmup: the same bytes per global chain.  K = 3
    packs CPB = 8 chains per gradient block: 33 is a multiple of neither 8 nor
    32."""
    import torch

    import mlx_mcmc_amd as m
    from mlx_mcmc_amd import _engine, _trace

    d = G.data(97, 33, 3)
    lp_fn, init = G.model(G.ns_product(), d)
    kw = dict(num_samples=6, num_warmup=14, step_size=0.05, num_leapfrog_steps=4,
              key=m.random.key(9), num_slices=3)

    def run(C, off=0):
        s, _ = m.hmc(lp_fn, init, num_chains=C, chain_offset=off, progress=False, **kw)
        return np.concatenate([s["B"].reshape(C, 6, -1), s["a"]], axis=2)

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
