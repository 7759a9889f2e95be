"""Posterior predictive sampling without a device: the scalar definition
(mc_predictive_draw, csrc/predictive.h) against the NumPy oracle and
scipy.stats, the host merge of partials, the facade's error before run() and
the ABI."""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy import stats as sps

import _predictive as PP
from mlx_mcmc_amd import _lib, diagnostics as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Kolmogorov-Smirnov cap on D sqrt(n): the asymptotic p ~ 1e-4
# (2 exp(-2 * 2.23^2) = 9.6e-5), so that a correct sampler fails one of the
# eleven cases below with probability ~ 1e-3.
KS_CAP = 2.23
KS_N = 20000
GAMMA_CASES = [(a, b) for a in (0.3, 1.0, 2.5, 40.0) for b in (0.5, 3.0)]
BETA_CASES = [(0.5, 0.5), (2.0, 5.0), (30.0, 1.2)]


def _triples(n=300, seed=5):
    """(chain, iter, obs) with chain > 0, iter > 0 and obs >= 2^24 among them."""
    rng = np.random.default_rng(seed)
    chain = rng.integers(0, 1000, n)
    it = rng.integers(0, 100000, n)
    obs = rng.integers(0, 5000, n)
    obs[n // 2:] = rng.integers(2 ** 24, 2 ** 32, n - n // 2)
    chain[0] = it[0] = obs[0] = 0
    obs[-1] = 2 ** 32 - 1
    return chain, it, obs


def test_closed_form_samplers_equal_the_oracle_bit_for_bit():
    chain, it, obs = _triples()
    rng = np.random.default_rng(6)
    loc = rng.standard_normal(chain.size).astype(np.float32) * np.float32(10.0)
    sc = rng.uniform(0.01, 30.0, chain.size).astype(np.float32)
    seed = 0x1234567890ABCDEF
    got = PP.host_draws(PP.NORMAL, loc, sc, seed, chain, it, obs)
    assert got.tobytes() == PP.normal_draw(loc, sc, seed, chain, it, obs).tobytes()
    got = PP.host_draws(PP.HALFNORMAL, loc, sc, seed, chain, it, obs)     # (loc is ignored)
    assert got.tobytes() == PP.halfnormal_draw(sc, seed, chain, it, obs).tobytes()
    assert np.all(got >= 0)
    got = PP.host_draws(PP.EXPONENTIAL, loc, sc, seed, chain, it, obs)
    assert got.tobytes() == PP.exponential_draw(sc, seed, chain, it, obs).tobytes()
    assert np.all(got >= 0) and np.all(np.isfinite(got))


def _ks(x, cdf):
    d = sps.kstest(np.asarray(x, np.float64), cdf).statistic
    return float(d * np.sqrt(len(x)))


def _grid(case):
    """20 000 distinct (iter, obs) pairs; the seed is fixed per case."""
    it, obs = np.divmod(np.arange(KS_N), 200)
    return 1000 + case, it, obs


@pytest.mark.parametrize("case", range(len(GAMMA_CASES)))
def test_gamma_kolmogorov_smirnov(case):
    a, b = GAMMA_CASES[case]
    seed, it, obs = _grid(case)
    x = PP.host_draws(PP.GAMMA, a, b, seed, 3, it, obs)
    assert np.all(np.isfinite(x)) and np.all(x >= 0)
    ref = sps.gamma(a, scale=1.0 / b)
    k = _ks(x, ref.cdf)
    own = _ks(ref.rvs(KS_N, random_state=np.random.default_rng(seed)), ref.cdf)
    print(f"Gamma({a}, {b}): D sqrt(n) = {k:.3f} (scipy's own rvs: {own:.3f})")
    assert own < KS_CAP
    assert k < KS_CAP


@pytest.mark.parametrize("case", range(len(BETA_CASES)))
def test_beta_kolmogorov_smirnov(case):
    a, b = BETA_CASES[case]
    seed, it, obs = _grid(100 + case)
    x = PP.host_draws(PP.BETA, a, b, seed, 0, it, obs)
    assert np.all(np.isfinite(x)) and np.all((x >= 0) & (x <= 1))
    ref = sps.beta(a, b)
    k = _ks(x, ref.cdf)
    own = _ks(ref.rvs(KS_N, random_state=np.random.default_rng(seed)), ref.cdf)
    print(f"Beta({a}, {b}): D sqrt(n) = {k:.3f} (scipy's own rvs: {own:.3f})")
    assert own < KS_CAP
    assert k < KS_CAP


def test_invalid_parameters_give_nan():
    nan = float("nan")
    for dist in (PP.NORMAL, PP.HALFNORMAL, PP.EXPONENTIAL, PP.GAMMA, PP.BETA):
        for s in (0.0, -1.0, nan):
            assert np.isnan(PP.host_draw(dist, 1.5, s, 7, 1, 2, 3)), (dist, s)
    for dist in (PP.GAMMA, PP.BETA):
        for a in (0.0, -1.0, nan):                       # alpha = 0 among them
            assert np.isnan(PP.host_draw(dist, a, 2.0, 7, 1, 2, 3)), (dist, a)
    assert np.isnan(PP.host_draw(PP.NORMAL, nan, 1.0, 7, 1, 2, 3))      # a NaN loc
    assert np.isfinite(PP.host_draw(PP.NORMAL, 0.0, 1.0, 7, 1, 2, 3))
    # shapes no attempt accepts (an infinite shape: every test compares NaN)
    # run out of attempts: NaN, promptly
    assert np.isnan(PP.host_draw(PP.GAMMA, float("inf"), 1.0, 7, 1, 2, 3))
    # distributions without a sampling distribution
    out = ctypes.c_float()
    lib = _lib.load()
    for dist in (_lib.MC_DIST_IDENTITY, _lib.MC_DIST_EXPR, 17, -1):
        assert lib.mc_predictive_draw(dist, 0.0, 1.0, 0, 0, 0, 0,
                                      ctypes.byref(out)) == _lib.MC_ERR_UNSUPPORTED
    assert lib.mc_predictive_draw(0, 0.0, 1.0, 0, 0, 0, 0, None) == _lib.MC_ERR_INVALID


@pytest.mark.parametrize("dist,m,s", [(PP.NORMAL, 0.5, 2.0), (PP.EXPONENTIAL, 0.0, 1.5),
                                      (PP.GAMMA, 0.7, 2.0), (PP.BETA, 2.0, 3.0)])
def test_every_counter_field_changes_the_draw(dist, m, s):
    base = dict(seed=11, chain=2, it=5, obs=9)
    x0 = PP.host_draw(dist, m, s, **base)
    for k, v in (("seed", 12), ("seed", 11 + 2 ** 32), ("chain", 3), ("it", 6), ("obs", 10)):
        assert PP.host_draw(dist, m, s, **dict(base, **{k: v})) != x0, k
    assert PP.host_draw(dist, m, s, **base) == x0


def _matrix(seed=3, Rn=53, M=9):
    """[R, M] float32 replicates with a column holding one NaN and a column
    that is all NaN, and their observations."""
    rng = np.random.default_rng(seed)
    x = rng.normal(2.0, 3.0, (Rn, M)).astype(np.float32)
    x[17, 4] = np.nan
    x[:, 6] = np.nan
    return x, rng.normal(2.0, 3.0, M)


@pytest.mark.parametrize("cuts", [(20,), (5, 31), (1, 52)])
def test_merge_of_uneven_shards_equals_the_whole(cuts):
    x, v = _matrix()
    whole = PP.stats_of(x, v)
    parts = [PP.stats_of(s, v) for s in np.split(x, cuts, axis=0)]
    got = D.merge_predictive(parts)
    assert sorted(got) == sorted(PP.FIELDS)
    for f in PP.FIELDS:
        np.testing.assert_allclose(got[f], whole[f], rtol=1e-12, atol=0, err_msg=f)
    # one NaN replicate: counted, the moments are the other 52 draws'
    others = np.delete(x[:, 4].astype(np.float64), 17)
    assert got["nonfinite"][4] == 1 and got["n"][4] == 53
    np.testing.assert_allclose(got["mean"][4], others.mean(), rtol=1e-12)
    np.testing.assert_allclose(got["m2"][4], others.var() * 52, rtol=1e-12)
    # all NaN: no moments, nothing below
    assert got["nonfinite"][6] == 53 and got["below"][6] == 0
    assert np.isnan(got["mean"][6]) and np.isnan(got["m2"][6])
    # an all-NaN shard in front of, behind and between finite shards
    col = x[:, :1].copy()
    col[:5] = np.nan
    for c in [(5,), (2, 5), (5, 30)]:
        m = D.merge_predictive([PP.stats_of(s, v[:1]) for s in np.split(col, c, axis=0)])
        w = PP.stats_of(col, v[:1])
        for f in PP.FIELDS:
            np.testing.assert_allclose(m[f], w[f], rtol=1e-12, atol=0, err_msg=f)
    rev = D.merge_predictive([PP.stats_of(col[5:], v[:1]), PP.stats_of(col[:5], v[:1])])
    np.testing.assert_allclose(rev["mean"], PP.stats_of(col, v[:1])["mean"], rtol=1e-12)


def test_merge_of_nothing_raises():
    with pytest.raises(ValueError):
        D.merge_predictive([])


def test_posterior_predictive_before_run_raises():
    import mlx_mcmc_amd as m

    mc = m.MCMC(lambda p: m.Normal(0, 1).log_prob(p["x"]))
    with pytest.raises(ValueError, match="Must run sampling first"):
        mc.posterior_predictive(lambda p: m.Normal(p["x"], 1).log_prob(0.5))


def test_header_declares_and_library_exports_the_symbols():
    text = open(os.path.join(ROOT, "include", "mcmc355.h")).read()
    assert re.search(r"#define\s+MC_RNG_TAG_PREDICT\s+7\b", text)
    assert _lib.MC_RNG_TAG_PREDICT == PP.TAG_PREDICT == 7
    for k, f in enumerate(("N", "MEAN", "M2", "BELOW", "NONFINITE", "COUNT")):
        assert re.search(rf"#define\s+MC_PP_{f}\s+{k}\b", text), f
        assert getattr(_lib, f"MC_PP_{f}") == k
    assert D.PP_FIELDS == PP.FIELDS and len(D.PP_FIELDS) == _lib.MC_PP_COUNT
    lib = _lib.load()
    bound = {name: (res, args) for name, res, args in _lib.SIGNATURES}
    for name in ("mc_predictive_draw", "mc_predictive_workspace_bytes", "mc_predictive"):
        assert re.search(rf"\b{name}\(", text), name
        fn = getattr(lib, name)                          # exported
        assert fn.restype is bound[name][0] and list(fn.argtypes) == bound[name][1]
    assert len(bound["mc_predictive"][1]) == 13
    assert lib.mc_predictive_workspace_bytes(ctypes.c_void_p(0), 1, 1, 1) == _lib.MC_ERR_INVALID


def test_host_only_program_has_no_view_to_sample_on():
    from mlx_mcmc_amd import _trace

    model = PP.mixed()
    init = {k: np.ones(s, np.float32) for k, s in model.shapes.items()}
    traced = _trace.trace(model.log_likelihood, init, keep_order=True)
    assert [t.n for t in traced.terms] == list(model.sizes)
    assert [t.dist for t in traced.terms] == [_lib.MC_DIST_GAMMA, _lib.MC_DIST_EXPONENTIAL,
                                              _lib.MC_DIST_BETA, _lib.MC_DIST_HALFNORMAL]
    lib = _lib.load()
    lib.mc_debug_program_host_only(1)
    try:
        prog = _trace.Program(traced)
    finally:
        lib.mc_debug_program_host_only(0)
    assert prog.num_elements == model.M
    assert lib.mc_predictive_workspace_bytes(prog.handle, 2, 3, 1) == _lib.MC_ERR_INVALID
