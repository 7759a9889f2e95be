"""Pointwise log-likelihood statistics and WAIC on the device
(mc_pointwise_stats, csrc/pointwise.h) against the float64 NumPy restatement
of tests/_pointwise.py, on synthetic draws.

Tolerances.  Matrix entries are f32 evaluations compared with float64 at the
project's bar for elementwise log_prob (rtol 2e-6, atol 2e-5).  A float32
NumPy restatement of these models stays within 0.27 of that bar on the matrix
and within 0.18 on every statistic (measured on the CPU: 0.129 / 0.031 / 0.011
/ 0.274 / 0.009 of the bar for the five models below).  The statistics are
f64 reductions of the device's own f32 values: against the same reduction in
NumPy of the device's matrix they agree at rtol 1e-10 (this isolates the
reduction); against the float64 model, at the matrix bar.

No staging case: the kernel stages nothing in LDS (a thread reads its <= 5
parameters of a draw from the sample buffer), so there are no chunk boundaries;
the boundaries that exist — the 256-observation tile, the 8-draw moment batch,
the draw blocks — are crossed by the shapes below (67 and 259 observations;
1 and 18 draws in one block, 111 draws in 3 blocks of 37, 200 in 6 of 34).
"""
import numpy as np
import pytest

import _pointwise as PW

pytestmark = pytest.mark.gpu


def _D():
    from mlx_mcmc_amd import diagnostics

    return diagnostics


_cache = {}


def _run(name, **kw):
    """(model, device result with matrix, float64 matrix), once per model."""
    key = (name, tuple(sorted(kw.items())))
    if key not in _cache:
        model = getattr(PW, name)(**kw)
        got = _D().pointwise_log_likelihood(model.log_likelihood, model.draws,
                                            PW.layout_of(model), matrix=True, group=False)
        _cache[key] = (model, got, model.ll(model.draws, np.float64))
    return _cache[key]


def _frac(got, ref):
    """Largest error as a fraction of the bar, over finite reference entries."""
    ok = np.isfinite(ref)
    if not ok.any():
        return 0.0
    return float(np.max(np.abs(got[ok] - ref[ok]) / (PW.ATOL + PW.RTOL * np.abs(ref[ok]))))


def _check(name, **kw):
    model, got, ref = _run(name, **kw)
    C, S, _ = model.draws.shape
    mat = got["matrix"].cpu().numpy()
    assert mat.shape == (C, S, model.M) and mat.dtype == np.float32
    print(f"{name}: matrix error {_frac(mat.astype(np.float64), ref):.3f} of the bar")
    np.testing.assert_array_equal(np.isfinite(mat), np.isfinite(ref))
    np.testing.assert_allclose(mat, ref, rtol=PW.RTOL, atol=PW.ATOL)
    own = PW.stats_of(mat)            # the same reduction of the device's own values
    model64 = PW.stats_of(ref)
    for f in PW.FIELDS:
        assert got[f].shape == (model.M,) and got[f].dtype == np.float64
        print(f"  {f}: {_frac(got[f], model64[f]):.3f} of the bar against the float64 model")
        np.testing.assert_allclose(got[f], own[f], rtol=1e-10, atol=0, err_msg=f)
        np.testing.assert_allclose(got[f], model64[f], rtol=PW.RTOL, atol=PW.ATOL, err_msg=f)
    return model, got, ref


def test_varying_intercept_unsorted_gather(gpu):
    _check("varying_intercept")


def test_two_terms_and_scalar_observation(gpu):
    model, got, ref = _check("two_terms_scalar")
    assert model.M == 13 + 259 + 1
    # term offsets: the Gamma term first (weight 1 / 13), the scalar last
    mat = got["matrix"].cpu().numpy()
    np.testing.assert_allclose(mat[..., -1], ref[..., -1], rtol=PW.RTOL, atol=PW.ATOL)


def test_scalar_observation_alone(gpu):
    model, got, _ = _check("scalar_only")
    assert model.M == 1 and got["n"][0] == 111


def test_logistic_regression_expression_term(gpu):
    _check("logistic")


def test_single_draw(gpu):
    model, got, ref = _check("varying_intercept", C=1, S=1)
    assert np.all(got["n"] == 1) and np.all(got["m2"] == 0) and np.all(got["sumexp"] == 1)
    w = _D().waic_from_stats(got)
    assert np.all(np.isnan(w["pointwise"]["p_waic"]))       # 0 / 0, as var(ddof=1)
    np.testing.assert_allclose(w["pointwise"]["lppd"], ref[0, 0], rtol=PW.RTOL, atol=PW.ATOL)


def test_out_of_support_draw(gpu):
    model, got, ref = _check("out_of_support")
    c, s, j = model.bad
    others = np.delete(ref.reshape(-1, model.M)[:, j], c * model.draws.shape[1] + s)
    assert got["nonfinite"][j] == 1 and got["nonfinite"].sum() == 1
    assert got["mean"][j] == -np.inf and np.isnan(got["m2"][j])
    np.testing.assert_allclose(got["sumexp"][j], np.sum(np.exp(others - others.max())),
                               rtol=PW.RTOL, atol=PW.ATOL)
    np.testing.assert_allclose(got["max"][j], others.max(), rtol=PW.RTOL, atol=PW.ATOL)
    w = _D().waic(model.log_likelihood, model.draws, PW.layout_of(model), group=False)
    assert w["n_nonfinite"] == 1 and w["n_obs"] == model.M and w["n_draws"] == 18
    assert np.isnan(w["elpd_waic"]) and np.isfinite(w["lppd"])


@pytest.mark.parametrize("name", ["two_terms_scalar", "logistic"])
def test_deterministic_with_and_without_matrix(gpu, name):
    model, got, _ = _run(name)
    lay = PW.layout_of(model)
    again = _D().pointwise_log_likelihood(model.log_likelihood, model.draws, lay, matrix=True,
                                          group=False)
    plain = _D().pointwise_log_likelihood(model.log_likelihood, model.draws, lay, group=False)
    assert "matrix" not in plain
    for f in PW.FIELDS:
        assert got[f].tobytes() == again[f].tobytes() == plain[f].tobytes(), f
    assert np.array_equal(got["matrix"].cpu().numpy(), again["matrix"].cpu().numpy(),
                          equal_nan=True)


def test_dict_samples_match_the_buffer(gpu):
    model, got, _ = _run("varying_intercept")
    q = model.draws
    as_dict = {"alpha": q[..., :5], "beta": q[..., 5], "log_sigma": q[..., 6]}
    d = _D().pointwise_log_likelihood(model.log_likelihood, as_dict, group=False)
    for f in PW.FIELDS:
        assert d[f].tobytes() == got[f].tobytes(), f


def test_end_to_end_waic_after_hmc(gpu):
    import mlx_mcmc_amd as m
    import mlx_mcmc_amd.core as mx
    import workloads as W

    lp_fn, _ = W.simple_normal(W.ns_product())
    data = W.simple_normal_data().astype(np.float32)

    def ll(p):
        return mx.sum(m.Normal(p["mu"], p["sigma"]).log_prob(mx.array(data)))

    mc = m.MCMC(lp_fn)
    mc.run({"mu": 4.5, "sigma": 2.0}, num_samples=50, num_warmup=50, method="hmc",
           step_size=0.1, num_leapfrog_steps=10, num_chains=4, random_seed=5, verbose=False,
           progress=False)
    assert mc.samples["mu"].shape == (4, 50)
    w = mc.waic(ll)                                        # the kept device buffer
    host = _D().waic(ll, mc.samples, group=False)          # the host-dict path
    for k in ("elpd_waic", "p_waic", "waic", "se", "lppd", "n_obs", "n_draws", "n_nonfinite"):
        assert w[k] == host[k], k
    mu = mc.samples["mu"].astype(np.float64)[..., None]
    sg = mc.samples["sigma"].astype(np.float64)[..., None]
    ref = PW.waic_of(PW.normal_lp(data.astype(np.float64), mu, sg, np.float64))
    assert w["n_obs"] == 100 and w["n_draws"] == 200 and w["n_nonfinite"] == 0
    np.testing.assert_allclose(w["pointwise"]["lppd"], ref["lppd_i"], rtol=PW.RTOL, atol=PW.ATOL)
    np.testing.assert_allclose(w["pointwise"]["p_waic"], ref["p_waic_i"], rtol=PW.RTOL,
                               atol=PW.ATOL)
    # sums over 100 observations: 100 times the per-observation slack
    np.testing.assert_allclose(w["elpd_waic"], ref["elpd_waic"], rtol=PW.RTOL, atol=100 * PW.ATOL)
    np.testing.assert_allclose(w["se"], ref["se"], rtol=1e-5)
    st = mc.pointwise_log_likelihood(ll, matrix=True)
    assert tuple(st["matrix"].shape) == (4, 50, 100)
