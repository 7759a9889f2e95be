"""PSIS-LOO of design-matrix likelihoods on the MFMA select and gather kernels
(loo(loo_kernel="glm"), mc_glm_psis_loo, csrc/glm_psis.h).

Both comparisons are against the device's own ``pointwise_log_likelihood(
matrix=True)`` of the same likelihood and draws (held to float64 by
tests/test_gpu_glm_pointwise.py): the selection — tail, cutoff, minimum, tail
count — is bit-equal to ``np.sort`` of that matrix's column, and k-hat, sigma
and elpd_loo_i agree at rtol 1e-10 (the project's bar for f64 reductions) with
tests/_psis.psis_matrix of that matrix.

Shapes (observations x columns, C x S), the smallest across each boundary:
33 x 3, 2 x 9: one draw block, fewer than 17 draws so the upper half of a wave
is empty, Mt = 4 (no fit); 130 x 40, 4 x 150: two workgroups of rows, PT = 2,
two draw blocks of 320, a last tile of 24 draws, Mt = 74 (above a wave, sort
padded to 128); 33 x 129, 4 x 250: PT = 8, three blocks of 352, a last tile of
8 draws, Mt = 95.
"""
import numpy as np
import pytest

import _glm
import _glm_pointwise as GP
import _psis as PS
from test_gpu_psis import _check_selection, _same_bits

pytestmark = pytest.mark.gpu

SHAPES = {"small": (33, 3, 2, 9, 4), "two_blocks": (130, 40, 4, 150, 74),
          "wide": (33, 129, 4, 250, 95)}
# across the set: icpt="param", scale="exp", sliced=True, the Poisson offset (default)
OPTIONS = {("normal", "small"): dict(scale="exp"), ("normal", "two_blocks"): dict(icpt="param"),
           ("normal", "wide"): dict(sliced=True, scale="exp"),
           ("bernoulli", "small"): dict(icpt="param", sliced=True),
           ("bernoulli", "two_blocks"): dict(icpt="const"), ("bernoulli", "wide"): dict(),
           ("poisson", "small"): dict(), ("poisson", "two_blocks"): dict(sliced=True),
           ("poisson", "wide"): dict(icpt="param", offset=False)}


def _D():
    from mlx_mcmc_amd import diagnostics

    return diagnostics


def _loo(c, **kw):
    return _D().loo(c.log_likelihood, c.draws, GP.layout_of(c), group=False, loo_kernel="glm",
                    **kw)


def _own(c):
    got = _D().pointwise_log_likelihood(c.log_likelihood, c.draws, GP.layout_of(c), matrix=True,
                                        group=False)
    return PS.psis_matrix(got["matrix"].cpu().numpy().reshape(-1, c.N))


def _check_fit(got, own, ok=slice(None)):
    pw = got["pointwise"]
    for f, g in (("khat", pw["khat"]), ("sigma", got["sigma"]), ("elpd", pw["elpd_loo"])):
        np.testing.assert_allclose(g[ok], own[f][ok], rtol=1e-10, atol=0, err_msg=f)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("family", ["normal", "bernoulli", "poisson"])
def test_selection_and_fit_against_the_devices_own_matrix(gpu, family, shape):
    N, P, C, S, mt = SHAPES[shape]
    c = GP.case(family, N, P, C, S, **OPTIONS[family, shape])
    got, own = _loo(c, tail=True), _own(c)
    assert got["tail_len"] == mt == own["tail_len"]
    assert got["n_obs"] == N and got["n_draws"] == C * S and got["n_nonfinite"] == 0
    _check_selection(got, own)
    _check_fit(got, own)
    if shape == "small":   # at most four tail values: no fit, nothing is smoothed
        assert np.all(got["pointwise"]["khat"] == np.inf) and got["n_high_k"] == N
    else:
        assert np.all(np.isfinite(got["pointwise"]["khat"]))
    plain = _loo(c)        # the same bits, with or without the tail
    assert "tail" not in plain and "cutoff" not in plain
    for f in ("elpd_loo", "p_loo", "lppd", "khat"):
        assert _same_bits(got["pointwise"][f], plain["pointwise"][f]), f


def test_repeated_draws_tie_at_the_cutoff(gpu):
    N, P, C, S, mt = SHAPES["two_blocks"]
    c = GP.case("normal", N, P, C, S, icpt="param", seed=1)
    c.draws[:, 1::3] = c.draws[:, 0::3]   # every row three times, as rejected proposals leave
    c.draws[:, 2::3] = c.draws[:, 0::3]
    got, own = _loo(c, tail=True), _own(c)
    assert own["tail_len"] == mt and np.any(own["n"] < mt)   # ties at the cutoff dropped out
    _check_selection(got, own)
    _check_fit(got, own)


def test_a_non_integer_poisson_observation(gpu):
    N, P, C, S, _ = SHAPES["two_blocks"]
    c = GP.case("poisson", N, P, C, S)
    c.d.y[5] = 2.5                        # (the likelihood reads d.y when it is traced)
    got, own = _loo(c, tail=True), _own(c)
    pw, ok = got["pointwise"], np.arange(N) != 5
    assert got["n_nonfinite"] == C * S
    assert np.isnan(pw["elpd_loo"][5]) and np.isnan(pw["khat"][5]) and np.isnan(got["sigma"][5])
    _check_selection(got, own)
    _check_fit(got, own, ok)
    assert np.all(np.isfinite(pw["elpd_loo"][ok]))


def test_after_hmc(gpu):
    import mlx_mcmc_amd as m

    c = GP.case("bernoulli", 64, 3, 1, 1, icpt="param")
    ns = _glm.ns_product()

    def log_prob(p):
        return (c.log_likelihood(p) + ns.sum(ns.Normal(0.0, 2.0).log_prob(p["w"]))
                + ns.Normal(0.0, 5.0).log_prob(p["a"]))

    mc = m.MCMC(log_prob)
    mc.run({"w": np.zeros(3, np.float32), "a": np.float32(0.0)}, num_samples=40, num_warmup=20,
           method="hmc", step_size=0.1, num_leapfrog_steps=5, num_chains=2, random_seed=3,
           verbose=False, progress=False)
    got = mc.loo(c.log_likelihood, loo_kernel="glm")
    host = _D().loo(c.log_likelihood, mc.samples, group=False, loo_kernel="glm")
    assert got["n_obs"] == 64 and got["n_draws"] == 80 and got["tail_len"] == 16
    for f in ("elpd_loo", "p_loo", "lppd", "khat"):
        assert _same_bits(got["pointwise"][f], host["pointwise"][f]), f
