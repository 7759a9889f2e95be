"""PSIS-LOO without a device: the tail-length rule, the float64 restatement's
own sanity (it recovers a generalized Pareto shape), the library's host fit
(mc_psis_fit_host: the code the fit kernel runs) against the restatement, and
the Python layer's refusals."""
import ctypes

import numpy as np
import pytest

import _psis as PS
from mlx_mcmc_amd import _lib, diagnostics as D


def _host_fit(tail_desc, cutoff, lmin, want_lw=True):
    lib = _lib.load()
    t = np.ascontiguousarray(tail_desc, np.float32)
    kh, sg = ctypes.c_double(), ctypes.c_double()
    lw = np.full(t.size, np.nan)
    rc = lib.mc_psis_fit_host(t.ctypes.data_as(ctypes.c_void_p), t.size, float(cutoff),
                              float(lmin), ctypes.byref(kh), ctypes.byref(sg),
                              lw.ctypes.data_as(ctypes.c_void_p) if want_lw else None)
    assert rc == _lib.MC_OK, lib.mc_last_error()
    return kh.value, sg.value, lw


def test_tail_lengths():
    lib = _lib.load()
    for N, mt in PS.TAIL_LENS.items():
        assert lib.mc_psis_tail_len(N, 1.0) == mt == PS.tail_len(N), N
    assert lib.mc_psis_tail_len(7400, 0.25) == PS.tail_len(7400, 0.25) == 517
    assert lib.mc_psis_tail_len(0, 1.0) == _lib.MC_ERR_INVALID
    assert lib.mc_psis_tail_len(10, 0.0) == _lib.MC_ERR_INVALID
    assert lib.mc_psis_tail_len(10, float("nan")) == _lib.MC_ERR_INVALID


@pytest.mark.parametrize("n", [100, 1518])
@pytest.mark.parametrize("k", [-0.3, 0.2, 0.7, 1.2])
def test_restatement_recovers_a_generalized_pareto_shape(n, k):
    """A condition on the reference, not on the code under test: the restated
    fit of n inverse-CDF draws from GPD(k, sigma = 1) lands within
    4 (1 + |k|) / sqrt(n) of k, for twenty seeds."""
    worst = 0.0
    for seed in range(20):
        u = np.random.default_rng(100 + seed).uniform(size=n)
        y = np.sort(np.expm1(-k * np.log1p(-u)) / k)
        khat, sigma = PS.gpd_fit(y)
        worst = max(worst, abs(khat - k) / ((1 + abs(k)) / np.sqrt(n)))
        assert sigma > 0
    print(f"n = {n}, k = {k}: worst |khat - k| = {worst:.2f} (1 + |k|) / sqrt(n)")
    assert worst <= 4.0


def _model_tails():
    """(label, column) pairs: float32 NumPy columns of the models' matrices
    whose tails have n = 5, 22, 23, 40, 76, 259 values, and a synthetic 1518."""
    out = []
    for label, model, obs in [
            ("n5", PS.varying_intercept(C=1, S=25), (0, 33, 66)),
            ("n22", PS.tied(), (0, 33, 66)),
            ("n23", PS.varying_intercept(), (0, 33, 66)),
            ("n40", PS.two_terms_scalar(C=4, S=50), (0, 12, 13, 271, 272)),
            ("n76", PS.varying_intercept(C=4, S=160), (0, 66)),
            ("n259", PS.logistic(C=8, S=925), (0, 66))]:
        mat = model.ll(model.draws, np.float32).reshape(-1, model.M)
        out += [(f"{label}/{o}", mat[:, o]) for o in obs]
    rng = np.random.default_rng(1518)
    out.append(("n1518", (-0.5 * rng.standard_normal(256000) ** 2 - 1.0).astype(np.float32)))
    return out


def test_host_fit_against_the_restatement():
    """k-hat, sigma and every log weight of the library's host fit against the
    float64 restatement at rtol 1e-10 (the project's bar for f64 reductions);
    the restatement's two summation orders are printed beside it."""
    seen = set()
    for label, col in _model_tails():
        ref = PS.psis_column(col)
        rev = PS.psis_column(col, reverse=True)
        seen.add(ref["n"])
        kh, sg, lw = _host_fit(ref["tail"][::-1], ref["cutoff"], ref["min"])
        with np.errstate(all="ignore"):
            order = max(abs(rev["khat"] - ref["khat"]) / abs(ref["khat"]),
                        float(np.nanmax(np.abs(rev["lw"] - ref["lw"]) / np.abs(ref["lw"]))))
        print(f"{label}: n = {ref['n']}, khat = {kh:.6f}, sigma = {sg:.6g}; "
              f"host - restatement {abs(kh - ref['khat']) / abs(ref['khat']):.2e}, "
              f"restatement's two orders {order:.2e}")
        assert np.isfinite(kh) and sg > 0
        np.testing.assert_allclose(kh, ref["khat"], rtol=1e-10, atol=0, err_msg=label)
        np.testing.assert_allclose(sg, ref["sigma"], rtol=1e-10, atol=0, err_msg=label)
        np.testing.assert_allclose(lw, ref["lw"], rtol=1e-10, atol=0, err_msg=label)
        assert np.all(lw <= 0) and np.all(np.diff(lw) >= 0)
    assert seen == {5, 22, 23, 40, 76, 259, 1518}, seen


def test_four_values_are_not_fitted():
    t = np.array([-1.0, -1.5, -2.0, -4.0], np.float32)
    kh, sg, lw = _host_fit(t, -0.5, -4.0)
    assert kh == np.inf and np.isnan(sg)
    np.testing.assert_array_equal(lw, -4.0 - t.astype(np.float64))      # the raw rule
    kh, sg, lw = _host_fit(t[:0], -0.5, -4.0)
    assert kh == np.inf and lw.size == 0
    kh, sg, _ = _host_fit(t, -0.5, -4.0, want_lw=False)
    assert kh == np.inf
    lib = _lib.load()
    assert lib.mc_psis_fit_host(None, 3, 0.0, 0.0, None, None, None) == _lib.MC_ERR_INVALID


@pytest.mark.parametrize("n", [8, 110, 1000])
def test_all_exceedances_equal(n):
    """A tail of one repeated value (reachable through the host call alone: a
    device tail of equal values still has its smallest apart).  The rule is
    IEEE arithmetic all the way: the result is what the restatement's same
    formulas give — finite, or NaN should a grid point land on b = 0 (0 / 0) —
    and a NaN k-hat smooths nothing."""
    t = np.full(n, -3.0, np.float32)
    kh, sg, lw = _host_fit(t, -1.0, -3.5)
    y = np.full(n, np.exp(-3.5 + 3.0) - np.exp(-3.5 + 1.0))
    rk, rs = PS.gpd_fit(y)
    print(f"n = {n}: khat = {kh}, sigma = {sg} (restatement {rk}, {rs})")
    assert np.isnan(kh) == np.isnan(rk) and np.isnan(sg) == np.isnan(rs)
    if np.isnan(kh):
        np.testing.assert_array_equal(lw, -3.5 + 3.0)
    else:
        np.testing.assert_allclose([kh, sg], [rk, rs], rtol=1e-8)
        assert np.all(np.isfinite(lw)) and np.all(lw <= 0)


def _fake(elpd_i, key="elpd_loo"):
    return {"pointwise": {key: np.asarray(elpd_i, np.float64)}, "n_obs": len(elpd_i)}


def test_compare():
    rng = np.random.default_rng(4)
    a, b = rng.normal(-1, 0.3, 50), rng.normal(-1.1, 0.3, 50)
    c = D.compare(_fake(a), _fake(b))
    np.testing.assert_allclose(c["elpd_diff"], np.sum(a - b), rtol=1e-13)
    np.testing.assert_allclose(c["se_diff"], np.sqrt(50 * np.var(a - b)), rtol=1e-13)
    assert D.compare(_fake(a), _fake(a)) == {"elpd_diff": 0.0, "se_diff": 0.0, "n_obs": 50}
    w = D.compare(_fake(a, "elpd_waic"), _fake(b, "elpd_waic"))
    assert w["elpd_diff"] == c["elpd_diff"]
    with pytest.raises(ValueError, match="50 and 49"):
        D.compare(_fake(a), _fake(b[:49]))
    with pytest.raises(ValueError, match="two loo results or two waic"):
        D.compare(_fake(a), _fake(b, "elpd_waic"))


def test_loo_before_run_raises():
    import mlx_mcmc_amd as m

    mc = m.MCMC(lambda p: m.Normal(0, 1).log_prob(p["x"]))
    with pytest.raises(ValueError, match="Must run sampling first"):
        mc.loo(lambda p: m.Normal(p["x"], 1).log_prob(0.5))


def test_loo_refuses_shards_of_draws(monkeypatch):
    import torch.distributed as dist

    monkeypatch.setattr(dist, "is_available", lambda: True)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    model = PS.scalar_only()
    with pytest.raises(ValueError, match="not mergeable over shards of draws"):
        D.loo(model.log_likelihood, {"mu": model.draws[..., 0]})
    with pytest.raises(ValueError, match="r_eff"):
        D.loo(model.log_likelihood, {"mu": model.draws[..., 0]}, r_eff=0.0, group=False)
