"""Posterior predictive replicates on the device (mc_predictive,
csrc/predictive.h) against the library's scalar host definition
(mc_predictive_draw) and the NumPy restatement of tests/_predictive.py, on
synthetic draws.

Shapes: C = 3, S = 37 is a ragged batch of 8 draws and B = 3 draw blocks
(111 / 32); 259 observations cross the 256-element tile; the single draw
C = S = 1 is one block.

Tolerances.  Replicates of raw operands equal the host definition bit for bit
(IEEE operations only on both sides); Gamma / Beta shapes below 1 go through
one double exp rounded to f32 (mc_expf_ref) and are held to 2 ulp(f32).
Through an exp-transformed scale the device's f32 exp is within 4 ulp of the
float64 transform: rtol 1e-6 where the scale is the whole replicate; with an
affine loc beside it the bound is 1e-6 of the scale's effect |scale * z0| plus
the final sum's rounding, 2^-24 |y|.  The statistics are f64 reductions of the
device's own f32 replicates: rtol 1e-10 against NumPy's (the bar of the
pointwise statistics).
"""
import numpy as np
import pytest

import _pointwise as PW
import _predictive as PP

pytestmark = pytest.mark.gpu

SEED = 0x5EED0123456789


def _D():
    from mlx_mcmc_amd import diagnostics

    return diagnostics


_cache = {}


def _run(name, **kw):
    """(model, device result with replicates, observations [C, S, M]), once per model."""
    key = (name, tuple(sorted(kw.items())))
    if key not in _cache:
        model = getattr(PP, name)(**kw)
        got = _D().posterior_predictive(model.log_likelihood, model.draws, PP.layout_of(model),
                                        seed=SEED, replicates=True, group=False)
        _cache[key] = (model, got, model.operands(model.draws)[1])
    return _cache[key]


def _check_stats(got, rep, value):
    own = PP.stats_of(rep, value)
    for f in PP.FIELDS:
        assert got[f].shape == (rep.shape[-1],) and got[f].dtype == np.float64
        np.testing.assert_allclose(got[f], own[f], rtol=1e-10, atol=0, err_msg=f)
    nfin = own["n"] - own["nonfinite"]
    with np.errstate(all="ignore"):
        np.testing.assert_allclose(got["var"], own["m2"] / (nfin - 1.0), rtol=1e-10)
        np.testing.assert_allclose(got["pit"], own["below"] / nfin, rtol=1e-10)


def _check_bits(name, **kw):
    model, got, value = _run(name, **kw)
    C, S, _ = model.draws.shape
    rep = got["replicates"].cpu().numpy()
    assert rep.shape == (C, S, model.M) and rep.dtype == np.float32
    host = PP.model_host_replicates(model, SEED)
    assert np.all(np.isfinite(host))
    assert rep.tobytes() == host.tobytes()
    _check_stats(got, rep, value)
    return model, got, rep


def test_normal_gathered_loc_two_tiles(gpu):
    model, got, rep = _check_bits("normal_gather")
    assert np.all(got["n"] == 111) and np.all(got["nonfinite"] == 0)
    # the NumPy oracle's float32 statement of the same draws
    q = model.draws
    _, _, m, s = model.operands(q)
    C, S, M = m.shape
    ref = PP.normal_draw(m, s, SEED, np.arange(C)[:, None, None], np.arange(S)[None, :, None],
                         np.arange(M)[None, None, :])
    assert rep.tobytes() == ref.tobytes()


def test_gamma_exponential_beta_halfnormal_shapes_from_one(gpu):
    model, got, rep = _check_bits("mixed")
    assert model.M == 13 + 1 + 5 + 7
    assert np.all(rep[..., :14] > 0) and np.all((rep[..., 14:19] > 0) & (rep[..., 14:19] < 1))
    assert np.all(rep[..., 19:] >= 0)


def test_gamma_beta_shapes_below_one(gpu):
    model, got, value = _run("mixed", lo=0.2, hi=0.95)
    rep = got["replicates"].cpu().numpy()
    host = PP.model_host_replicates(model, SEED)
    ulp = np.spacing(np.abs(host))
    worst = float(np.max(np.abs(rep.astype(np.float64) - host) / ulp))
    print(f"shapes below 1: worst difference {worst:.2f} ulp")
    assert worst <= 2.0
    # the terms without a boosted Gamma stay bit-identical
    assert rep[..., 13].tobytes() == host[..., 13].tobytes()
    assert rep[..., 19:].tobytes() == host[..., 19:].tobytes()
    _check_stats(got, rep, value)


def test_affine_loc(gpu):
    _check_bits("affine")


def test_single_draw(gpu):
    model, got, rep = _check_bits("normal_gather", C=1, S=1)
    assert np.all(got["n"] == 1) and np.all(got["m2"] == 0)
    assert np.array_equal(got["mean"], rep[0, 0].astype(np.float64))
    assert np.all(np.isnan(got["var"]))                     # 0 / 0, as var(ddof=1)


def _z0(model):
    C, S, _ = model.draws.shape
    return PP._z0(SEED, np.arange(C)[:, None, None], np.arange(S)[None, :, None],
                  np.arange(model.M)[None, None, :]).astype(np.float64)


def test_transformed_scale(gpu):
    model, got, value = _run("exp_scale")
    rep = got["replicates"].cpu().numpy()
    _, _, _, s = model.operands(model.draws)               # float64 exp of the f32 parameter
    C, S, _ = model.draws.shape
    c, i = np.arange(C)[:, None, None], np.arange(S)[None, :, None]
    ref = np.concatenate([
        np.abs(s[..., :7] * _z0(model)[..., :7]),
        PP.exponential_draw(1.0, SEED, c, i, np.array([7])[None, None, :]).astype(np.float64)
        / s[..., 7:]], axis=2)
    np.testing.assert_allclose(rep, ref, rtol=1e-6, atol=0)
    _check_stats(got, rep, value)


def test_transformed_scale_beside_an_affine_loc(gpu):
    model, got, value = _run("affine", transformed=True)
    rep = got["replicates"].cpu().numpy().astype(np.float64)
    _, _, m, s = model.operands(model.draws)
    eff = s * _z0(model)
    ref = m.astype(np.float64) + eff
    bound = 1e-6 * np.abs(eff) + 2.0 ** -24 * np.abs(ref)
    print(f"worst error {float(np.max(np.abs(rep - ref) / bound)):.3f} of the bound")
    assert np.all(np.abs(rep - ref) <= bound)
    _check_stats(got, got["replicates"].cpu().numpy(), value)


@pytest.mark.parametrize("name", ["normal_gather", "mixed"])
def test_deterministic_with_and_without_replicates(gpu, name):
    model, got, _ = _run(name)
    lay = PP.layout_of(model)
    again = _D().posterior_predictive(model.log_likelihood, model.draws, lay, seed=SEED,
                                      replicates=True, group=False)
    plain = _D().posterior_predictive(model.log_likelihood, model.draws, lay, seed=SEED,
                                      group=False)
    assert "replicates" not in plain
    for f in PP.FIELDS + ("var", "pit"):
        assert got[f].tobytes() == again[f].tobytes() == plain[f].tobytes(), f
    assert got["replicates"].cpu().numpy().tobytes() == again["replicates"].cpu().numpy().tobytes()
    other = _D().posterior_predictive(model.log_likelihood, model.draws, lay, seed=SEED + 1,
                                      group=False)
    assert other["mean"].tobytes() != got["mean"].tobytes()


@pytest.mark.parametrize("name", ["normal_gather", "mixed"])
def test_chain_split_reproduces_the_rows(gpu, name):
    model, got, _ = _run(name)
    lay, q = PP.layout_of(model), model.draws
    full = got["replicates"].cpu().numpy()
    a = _D().posterior_predictive(model.log_likelihood, q[0:2], lay, seed=SEED, replicates=True,
                                  chain_offset=0, group=False)
    b = _D().posterior_predictive(model.log_likelihood, q[2:3], lay, seed=SEED, replicates=True,
                                  chain_offset=2, group=False)
    assert a["replicates"].cpu().numpy().tobytes() == full[0:2].tobytes()
    assert b["replicates"].cpu().numpy().tobytes() == full[2:3].tobytes()
    merged = _D().merge_predictive([a, b])
    for f in PP.FIELDS:
        np.testing.assert_allclose(merged[f], got[f], rtol=1e-12, atol=0, err_msg=f)


@pytest.mark.parametrize("name", ["normal_gather", "mixed"])
def test_thin_reproduces_every_third_row(gpu, name):
    model, got, value = _run(name)
    full = got["replicates"].cpu().numpy()
    t = _D().posterior_predictive(model.log_likelihood, model.draws, PP.layout_of(model),
                                  seed=SEED, thin=3, replicates=True, group=False)
    rep = t["replicates"].cpu().numpy()
    assert rep.shape == (3, 13, model.M)                   # ceil(37 / 3)
    assert rep.tobytes() == np.ascontiguousarray(full[:, ::3]).tobytes()
    assert np.all(t["n"] == 39)
    _check_stats(t, rep, value[:, ::3])


@pytest.mark.parametrize("name", ["normal_gather", "mixed"])
def test_iteration_split_reproduces_the_rows(gpu, name):
    model, got, _ = _run(name)
    lay, q = PP.layout_of(model), model.draws
    full = got["replicates"].cpu().numpy()
    a = _D().posterior_predictive(model.log_likelihood, q[:, :20], lay, seed=SEED,
                                  replicates=True, group=False)
    b = _D().posterior_predictive(model.log_likelihood, q[:, 20:], lay, seed=SEED,
                                  replicates=True, iter_offset=20, group=False)
    assert a["replicates"].cpu().numpy().tobytes() == np.ascontiguousarray(full[:, :20]).tobytes()
    assert b["replicates"].cpu().numpy().tobytes() == np.ascontiguousarray(full[:, 20:]).tobytes()
    merged = _D().merge_predictive([a, b])
    for f in PP.FIELDS:
        np.testing.assert_allclose(merged[f], got[f], rtol=1e-12, atol=0, err_msg=f)


def test_non_positive_scale_gives_counted_nan(gpu):
    bad = ((1, 4, -0.3), (2, 36, 0.0))
    model, got, value = _run("normal_gather", bad=bad)
    rep = got["replicates"].cpu().numpy()
    for c, s, _ in bad:
        assert np.all(np.isnan(rep[c, s]))
    assert np.isnan(rep).sum() == 2 * model.M
    assert np.all(got["nonfinite"] == 2) and np.all(got["n"] == 111)
    # the finite moments are those of the other 109 draws
    keep = np.ones((3, 37), bool)
    for c, s, _ in bad:
        keep[c, s] = False
    others = rep[keep].astype(np.float64)
    np.testing.assert_allclose(got["mean"], others.mean(axis=0), rtol=1e-10)
    np.testing.assert_allclose(got["var"], others.var(axis=0, ddof=1), rtol=1e-10)
    np.testing.assert_allclose(got["pit"], (others < value[keep]).mean(axis=0), rtol=1e-10)
    _check_stats(got, rep, value)
    # and the other draws' replicates are those of the clean model
    clean = _run("normal_gather")[1]["replicates"].cpu().numpy()
    assert rep[keep].tobytes() == clean[keep].tobytes()


def test_expression_likelihood_is_refused_before_any_launch(gpu):
    from mlx_mcmc_amd import _lib

    model = PW.logistic()
    with pytest.raises(_lib.EngineError, match="term 0.*expression") as e:
        _D().posterior_predictive(model.log_likelihood, model.draws, PW.layout_of(model),
                                  group=False)
    assert e.value.code == _lib.MC_ERR_UNSUPPORTED


def test_end_to_end_after_hmc(gpu):
    import mlx_mcmc_amd as m
    import mlx_mcmc_amd.core as mx

    rng = np.random.default_rng(31)
    n = 200
    y = (0.7 + rng.standard_normal(n)).astype(np.float32)

    def lp(p):                                   # flat prior: theta | y ~ N(ybar, 1 / n)
        return mx.sum(m.Normal(p["theta"], 1.0).log_prob(y))

    mc = m.MCMC(lp)
    # 10 steps of 0.011: a quarter period of the posterior's oscillator
    # (omega = sqrt(n)), nearly independent draws; no step-size adaptation
    mc.run({"theta": 0.5}, num_samples=500, num_warmup=100, method="hmc", step_size=0.011,
           num_leapfrog_steps=10, adapt_step_size=False, num_chains=4, random_seed=9,
           verbose=False, progress=False)
    assert mc.samples["theta"].shape == (4, 500)
    pp = mc.posterior_predictive(lp)
    again = mc.posterior_predictive(lp, seed=9)            # the run's seed is the default
    assert pp["mean"].tobytes() == again["mean"].tobytes()
    post_mean, post_var = float(np.mean(y.astype(np.float64))), 1.0 / n
    pred_var = 1.0 + post_var
    assert np.all(pp["n"] == 2000) and np.all(pp["nonfinite"] == 0)
    se = np.sqrt(pred_var / 2000)
    print(f"worst mean deviation {float(np.max(np.abs(pp['mean'] - post_mean)) / se):.2f} se, "
          f"var in [{pp['var'].min():.3f}, {pp['var'].max():.3f}], "
          f"mean pit {pp['pit'].mean():.3f}")
    assert np.all(np.abs(pp["mean"] - post_mean) < 5 * se)
    assert np.all(np.abs(pp["var"] / pred_var - 1.0) < 0.15)
    assert abs(pp["pit"].mean() - 0.5) < 0.1
    rep = mc.posterior_predictive(lp, thin=10, replicates=True)["replicates"]
    assert tuple(rep.shape) == (4, 50, n)
