"""Pointwise log-likelihood and WAIC without a device: the host merge of
partials, the WAIC arithmetic, the observation order of a traced likelihood
and the facade's error before run()."""
import ctypes

import numpy as np
import pytest

import _pointwise as PW
from mlx_mcmc_amd import _lib, _trace, diagnostics as D


def _matrix(seed=3, R=53, M=9):
    """A float64 [R, M] matrix with a column holding one -inf and a column
    that is all -inf."""
    rng = np.random.default_rng(seed)
    x = rng.normal(-3.0, 2.0, (R, M))
    x[:, 1] += 40.0 * rng.uniform(size=R)          # a column whose maximum moves a lot
    x[17, 4] = -np.inf
    x[:, 6] = -np.inf
    return x


@pytest.mark.parametrize("cuts", [(20,), (5, 31), (1, 52)])
def test_merge_of_uneven_shards_equals_the_whole(cuts):
    x = _matrix()
    whole = PW.stats_of(x)
    parts = [PW.stats_of(s) for s in np.split(x, cuts, axis=0)]
    got = D.merge_pointwise(parts)
    for f in PW.FIELDS:
        np.testing.assert_allclose(got[f], whole[f], rtol=1e-12, atol=0, err_msg=f)
    # the -inf draw: its sum of exponentials is the others', mean -inf, M2 NaN
    assert np.isfinite(got["sumexp"][4]) and got["mean"][4] == -np.inf and np.isnan(got["m2"][4])
    assert got["nonfinite"][4] == 1
    # all -inf: MAX = -inf, SUMEXP = 0, no NaN in those two
    assert got["max"][6] == -np.inf and got["sumexp"][6] == 0.0
    assert got["nonfinite"][6] == x.shape[0]


def test_merge_order_of_nonfinite_classes():
    a = PW.stats_of(np.array([[1.0], [-np.inf]]))
    b = PW.stats_of(np.array([[np.inf], [2.0]]))
    c = PW.stats_of(np.array([[0.5], [1.5]]))
    assert D.merge_pointwise([a, c])["mean"][0] == -np.inf
    assert D.merge_pointwise([c, a])["mean"][0] == -np.inf
    assert np.isnan(D.merge_pointwise([a, b])["mean"][0])      # -inf + inf, as np.mean
    assert D.merge_pointwise([c, b])["max"][0] == np.inf
    with pytest.raises(ValueError):
        D.merge_pointwise([])


def test_waic_arithmetic_from_statistics():
    x = _matrix()[:, [0, 1, 2, 3, 5, 7, 8]]        # finite columns
    ref = PW.waic_of(x)
    got = D.waic_from_stats(PW.stats_of(x))
    for k in ("elpd_waic", "p_waic", "waic", "se", "lppd"):
        np.testing.assert_allclose(got[k], ref[k], rtol=1e-12, err_msg=k)
    np.testing.assert_allclose(got["pointwise"]["lppd"], ref["lppd_i"], rtol=1e-12)
    np.testing.assert_allclose(got["pointwise"]["p_waic"], ref["p_waic_i"], rtol=1e-12)
    np.testing.assert_allclose(got["pointwise"]["elpd_waic"], ref["elpd_i"], rtol=1e-12)
    assert got["waic"] == -2.0 * got["elpd_waic"]
    assert got["n_obs"] == x.shape[1] and got["n_draws"] == x.shape[0]
    assert got["n_high_p_waic"] == int(np.sum(ref["p_waic_i"] > 0.4)) > 0
    assert got["n_nonfinite"] == 0
    # one draw: p_waic is 0 / 0, as var(ddof=1) gives
    one = D.waic_from_stats(PW.stats_of(x[:1]))
    assert np.all(np.isnan(one["pointwise"]["p_waic"])) and one["n_draws"] == 1
    # an observation with a -inf draw is reported, not raised
    bad = D.waic_from_stats(PW.stats_of(_matrix()))
    assert bad["n_nonfinite"] == 1 + _matrix().shape[0]


def test_two_term_likelihood_counts_observations_in_trace_order():
    model = PW.two_terms_scalar()
    lay = PW.layout_of(model)
    init = {k: np.zeros(s, np.float32) for k, s in model.shapes.items()}
    traced = _trace.trace(model.log_likelihood, init, keep_order=True)
    assert [t.n for t in traced.terms] == list(model.sizes)
    assert traced.terms[0].dist == _lib.MC_DIST_GAMMA
    assert abs(traced.terms[0].weight - 1.0 / model.sizes[0]) < 1e-7
    # the library's count of a host-only program (no device)
    lib = _lib.load()
    lib.mc_debug_program_host_only(1)
    try:
        prog = _trace.Program(traced)
    finally:
        lib.mc_debug_program_host_only(0)
    assert prog.num_elements == sum(model.sizes) == model.M
    assert lib.mc_program_enable_pointwise(prog.handle) == _lib.MC_ERR_INVALID
    assert lib.mc_pointwise_workspace_bytes(prog.handle, 2, 3) == _lib.MC_ERR_INVALID
    assert lib.mc_program_num_elements(ctypes.c_void_p(0)) == _lib.MC_ERR_INVALID
    assert lay.size == 2


def test_folding_keeps_trace_order_for_a_likelihood():
    import mlx_mcmc_amd as m

    def ll(p):
        lp = m.Normal(p["mu"], 1.0).log_prob(0.1) + m.Normal(p["mu"], 1.0).log_prob(0.2)
        lp = lp + m.Normal(p["mu"], 3.0).log_prob(0.3)
        return lp + m.Normal(p["mu"], 1.0).log_prob(0.4)

    kept = _trace.trace(ll, {"mu": 0.0}, keep_order=True)
    assert [t.n for t in kept.terms] == [2, 1, 1]
    np.testing.assert_allclose(kept.terms[2].value.data, [0.4])
    folded = _trace.trace(ll, {"mu": 0.0})             # the samplers' folding is unchanged
    assert [t.n for t in folded.terms] == [3, 1]


def test_waic_before_run_raises():
    import mlx_mcmc_amd as m

    mc = m.MCMC(lambda p: m.Normal(0, 1).log_prob(p["x"]))
    with pytest.raises(ValueError, match="Must run sampling first"):
        mc.waic(lambda p: m.Normal(p["x"], 1).log_prob(0.5))
    with pytest.raises(ValueError, match="Must run sampling first"):
        mc.pointwise_log_likelihood(lambda p: m.Normal(p["x"], 1).log_prob(0.5))


def test_pointwise_needs_a_device():
    import torch

    if torch.cuda.is_available():
        return      # (the device path: tests/test_gpu_pointwise.py)
    model = PW.scalar_only()
    with pytest.raises(_lib.EngineUnavailable):
        D.pointwise_log_likelihood(model.log_likelihood, {"mu": model.draws[..., 0]})
