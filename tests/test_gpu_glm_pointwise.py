"""Pointwise log-likelihood and WAIC of design-matrix models on the device
(k_glm_pointwise, csrc/glm_pointwise.h) against a float64 NumPy evaluation of
the [C, S, N] matrix.

Matrix bound, per entry: ATOL + RTOL |ref| + 2 (P + 4) 2^-24 |r| A with A = |a|
+ |off_i| + sum_k |X_ik beta_k| and r = dl / d eta, both float64: the project's
elementwise f32 bar plus gamma_{P+2} A — a sequential f32 sum of P products
and two adds — carried to first order through l; the factor 2 covers the
products' own rounding and the second order.  The statistics are f64
reductions of the device's own f32 values: rtol 1e-10 against the same
reduction in NumPy.  WAIC against the float64 matrix: lppd_i, p_waic_i and
elpd_i each within ATOL + RTOL |want_i| + the largest third term of observation
i over the draws, and elpd_waic within the sum of its rows' bounds.
"""
import numpy as np
import pytest

import _glm
import _glm_pointwise as GP
import _pointwise as PW

pytestmark = pytest.mark.gpu

FAMILIES = _glm.FAMILIES
# (N, P, C, S), then what varies.  The last: R = 600 draws over NT = 5 row
# tiles (2 workgroups per draw block) split into B = 2 blocks of 320 and 280.
SHAPES = [
    ((32, 2, 1, 32), dict(icpt="none", scale="const", sliced=False, offset=True)),
    ((33, 3, 3, 37), dict(icpt="param", scale="exp", sliced=True, offset=True)),
    ((70, 33, 2, 40), dict(icpt="const", scale="const", sliced=True, offset=False)),
    ((40, 256, 1, 33), dict(icpt="param", scale="exp", sliced=False, offset=True)),
    ((150, 5, 2, 300), dict(icpt="param", scale="exp", sliced=True, offset=False)),
]
BIG = SHAPES[-1]


def _D():
    from mlx_mcmc_amd import diagnostics

    return diagnostics


def _pw(c, matrix=True, draws=None):
    got = _D().pointwise_log_likelihood(c.log_likelihood, c.draws if draws is None else draws,
                                        GP.layout_of(c), matrix=matrix, group=False)
    if matrix:
        got["matrix"] = got["matrix"].cpu().numpy()
    return got


def _check_waic(w, ref, third):
    """waic_from_stats' result w against the float64 matrix ref [R, N]; third
    [R, N] is the dot product's share of the entry bound."""
    want = PW.waic_of(ref)
    widen = third.max(axis=0)
    for key, wkey in (("lppd", "lppd_i"), ("p_waic", "p_waic_i"), ("elpd_waic", "elpd_i")):
        tol = PW.ATOL + PW.RTOL * np.abs(want[wkey]) + widen
        err = np.abs(w["pointwise"][key] - want[wkey])
        print(f"  {key}: worst error / bound {np.max(err / tol):.3f}")
        assert np.all(err <= tol), key
    assert abs(w["elpd_waic"] - want["elpd_waic"]) <= np.sum(tol)   # (tol: elpd_i's)


@pytest.mark.parametrize("shape,kw", SHAPES, ids=["x".join(map(str, s)) for s, _ in SHAPES])
@pytest.mark.parametrize("family", FAMILIES)
def test_matrix_and_statistics(gpu, family, shape, kw):
    c = GP.case(family, *shape, **kw)
    got = _pw(c)
    C, S, _ = c.draws.shape
    mat = got["matrix"]
    assert mat.shape == (C, S, c.N) and mat.dtype == np.float32
    ref, third = c.ref(c.draws)
    bound = GP.entry_bound(ref, third)
    err = np.abs(mat.astype(np.float64) - ref)
    print(f"{family} {shape}: worst matrix error / bound {np.max(err / bound):.3f}")
    assert np.all(np.isfinite(mat)) and np.all(err <= bound)
    own = PW.stats_of(mat)
    for f in PW.FIELDS:
        assert got[f].shape == (c.N,) and got[f].dtype == np.float64
        np.testing.assert_allclose(got[f], own[f], rtol=1e-10, atol=0, err_msg=f)
    assert np.all(got["n"] == C * S) and not got["nonfinite"].any()
    _check_waic(_D().waic_from_stats(got), ref.reshape(C * S, c.N), third.reshape(C * S, c.N))


def test_out_of_support_observation(gpu):
    c = GP.case("poisson", 33, 3, 3, 37, icpt="param", sliced=True)
    c.d.y[5] = 2.5                        # (the likelihood reads d.y when it is traced)
    got = _pw(c)
    R = 111
    assert got["max"][5] == -np.inf and got["sumexp"][5] == 0.0 and got["nonfinite"][5] == R
    assert got["nonfinite"].sum() == R and np.all(got["n"] == R)
    own = PW.stats_of(got["matrix"])
    for f in PW.FIELDS:
        np.testing.assert_allclose(got[f], own[f], rtol=1e-10, atol=0, err_msg=f)
    ref, third = c.ref(c.draws)
    keep = np.arange(33) != 5
    assert np.all(np.abs(got["matrix"][..., keep] - ref[..., keep])
                  <= GP.entry_bound(ref, third)[..., keep])


def test_nan_coefficient_draw(gpu):
    c = GP.case("bernoulli", 33, 3, 3, 37, icpt="param", sliced=True)
    draws = c.draws.copy()
    draws[1, 20, GP.LEAD + 1] = np.nan
    got = _pw(c, draws=draws)
    for f in ("max", "sumexp", "mean", "m2"):
        assert np.all(np.isnan(got[f])), f
    assert np.all(got["nonfinite"] == 1) and np.all(got["n"] == 111)
    mat = got["matrix"]
    assert np.all(np.isnan(mat[1, 20])) and np.isnan(mat).sum() == 33
    ref, third = c.ref(c.draws)           # the other draws' values are untouched
    ok = ~np.isnan(mat)
    assert np.all(np.abs(mat - ref)[ok] <= GP.entry_bound(ref, third)[ok])


def test_deterministic_with_and_without_matrix(gpu):
    c = GP.case("normal", *BIG[0], **BIG[1])
    first, again, plain = _pw(c), _pw(c), _pw(c, matrix=False)
    assert "matrix" not in plain
    assert first["matrix"].tobytes() == again["matrix"].tobytes()
    for f in PW.FIELDS:
        assert first[f].tobytes() == again[f].tobytes() == plain[f].tobytes(), f


def test_waic_after_hmc(gpu):
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
    assert mc.samples["w"].shape == (2, 40, 3)
    w = mc.waic(c.log_likelihood)                                     # the kept device buffer
    host = _D().waic(c.log_likelihood, mc.samples, group=False)       # the host-dict path
    for k in ("elpd_waic", "p_waic", "waic", "se", "lppd", "n_obs", "n_draws", "n_nonfinite"):
        assert w[k] == host[k], k
    assert w["n_obs"] == 64 and w["n_draws"] == 80 and w["n_nonfinite"] == 0
    q = np.concatenate([mc.samples["w"], mc.samples["a"][..., None]], axis=2)
    ref, third = c.ref(q)
    _check_waic(w, ref.reshape(80, 64), third.reshape(80, 64))


def test_refusals_before_any_launch(gpu):
    from mlx_mcmc_amd import _lib, _trace

    c = GP.case("poisson", 33, 3, 2, 9)
    lay = GP.layout_of(c)
    ns = _glm.ns_product()
    with pytest.raises(ValueError, match="LOO"):
        _D().loo(c.log_likelihood, c.draws, lay, group=False)
    with pytest.raises(ValueError, match="predictive"):
        _D().posterior_predictive(c.log_likelihood, c.draws, lay, group=False)
    with pytest.raises(ValueError, match=r"exactly one mx\.sum\(Family\(X @ beta"):
        _D().waic(lambda p: c.log_likelihood(p) + ns.sum(ns.Normal(0.0, 2.0).log_prob(p["w"])),
                  c.draws, lay, group=False)
    prog = _trace.pointwise_program(c.log_likelihood, lay)
    assert prog.num_elements == 33
    lib = _lib.load()
    assert lib.mc_psis_workspace_bytes(prog.handle, 2, 9, 1.0) == _lib.MC_ERR_UNSUPPORTED
    assert b"design-matrix" in lib.mc_last_error()
    assert lib.mc_predictive_workspace_bytes(prog.handle, 2, 9, 1) == _lib.MC_ERR_UNSUPPORTED
