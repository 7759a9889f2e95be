"""Posterior predictive replicates of design-matrix likelihoods on the device
(k_glm_predictive, csrc/glm_predictive.h; posterior_predictive(...,
predictive_kernel="glm")) against the definition at a float64 eta.

A replicate is the library's scalar sampler at the f32 eta the kernel forms;
that eta is within third = 2 (P + 4) 2^-24 A of the float64 one
(_glm_predictive.eta64).  Normal: |rep - (eta64 + s z0)| within
_glm_pointwise.entry_bound(ref, third), z0 the bit-exact f32 normal of the
entry's counter (a wrong index misses by O(1)).  Bernoulli / Poisson: the host
sampler at f32(eta64), f32(eta64 - third) and f32(eta64 + third); where the
three agree (an insensitive entry) the device must give exactly that value, and
at most 2 % of a case's entries may be sensitive (checked on the host alone
when the inputs were chosen: the shares are below 0.1 %).  The statistics are
f64 reductions of the device's own replicates: rtol 1e-10, counts exact.
"""
import functools

import numpy as np
import pytest

import _discrete as DS
import _glm
import _glm_pointwise as GP
import _glm_predictive as GPP
import _predictive as PP
from test_gpu_glm_pointwise import SHAPES

pytestmark = pytest.mark.gpu

SEED, CH0, IT0 = 11, 3, 7
RAGGED = 1                      # (33, 3, 3, 37)
# (family, shape index, what is added to the Poisson offset: rates past 10 run PTRS)
CASES = [(f, k, 0.0) for f in _glm.FAMILIES for k in range(len(SHAPES))] + [("poisson", RAGGED, 3.0)]


def _D():
    from mlx_mcmc_amd import diagnostics

    return diagnostics


def _case(family, k, boost=0.0):
    c = GP.case(family, *SHAPES[k][0], **SHAPES[k][1])
    if boost:
        c.d.off = c.d.off + np.float32(boost)   # (the likelihood reads d.off when it is traced)
    return c


def _pp(c, draws=None, replicates=True, chain_offset=CH0, iter_offset=IT0, **kw):
    got = _D().posterior_predictive(c.log_likelihood, c.draws if draws is None else draws,
                                    GP.layout_of(c), seed=SEED, replicates=replicates,
                                    chain_offset=chain_offset, iter_offset=iter_offset,
                                    group=False, predictive_kernel="glm", **kw)
    if replicates:
        got["replicates"] = got["replicates"].cpu().numpy()
    return got


@functools.lru_cache(maxsize=None)
def _ragged(family):
    """The (33, 3, 3, 37) case and its full run, shared and left unchanged."""
    c = _case(family, RAGGED)
    return c, _pp(c)


def _same(a, b, keys):
    return all(a[f].tobytes() == b[f].tobytes() for f in keys)


def _keys(family):
    return PP.FIELDS + (() if family == "normal" else ("equal",))


@pytest.mark.parametrize("family,k,boost", CASES,
                         ids=[f"{f}-{'x'.join(map(str, SHAPES[k][0]))}" + ("-ptrs" if b else "")
                              for f, k, b in CASES])
def test_replicates_and_statistics(gpu, family, k, boost):
    from mlx_mcmc_amd import _lib

    c = _case(family, k, boost)
    got = _pp(c)
    C, S, _ = c.draws.shape
    rep = got["replicates"]
    assert rep.shape == (C, S, c.N) and rep.dtype == np.float32 and np.all(np.isfinite(rep))
    eta, third, s = GPP.eta64(c, c.draws, **SHAPES[k][1])
    ids = (np.arange(C)[:, None, None] + CH0, np.arange(S)[None, :, None] + IT0,
           np.arange(c.N)[None, None, :])
    if family == "normal":
        ref = eta + s * PP._z0(SEED, *ids).astype(np.float64)
        err, bound = np.abs(rep - ref), GP.entry_bound(ref, third)
        print(f"{family} {SHAPES[k][0]}: worst error / bound {np.max(err / bound):.3f}")
        assert np.all(err <= bound)
    else:
        kind = (_lib.MC_DISCRETE_BERNOULLI if family == "bernoulli" else _lib.MC_DISCRETE_POISSON)
        mid, lo, hi = (DS.host_draws(kind, 0.0, (eta + d).astype(np.float32), SEED, *ids)
                       for d in (0.0, -third, third))
        calm = (mid == lo) & (mid == hi)
        print(f"{family} {SHAPES[k][0]}: sensitive share {1.0 - calm.mean():.5f}, "
              f"largest replicate {rep.max():.0f}")
        assert 1.0 - calm.mean() <= 0.02
        assert np.array_equal(rep[calm], mid[calm])
        if boost:
            assert (np.exp(eta) > 10.5).mean() > 0.5    # (most entries take the PTRS branch)
    own = DS.stats_of(rep, c.d.y)
    for f in PP.FIELDS:
        assert got[f].shape == (c.N,) and got[f].dtype == np.float64
        np.testing.assert_allclose(got[f], own[f], rtol=1e-10, atol=0, err_msg=f)
    assert np.array_equal(got["below"], own["below"])
    assert np.all(got["n"] == C * S) and not got["nonfinite"].any()
    if family == "normal":
        assert "equal" not in got and "pit_mid" not in got
    else:
        assert np.array_equal(got["equal"], own["equal"])
        assert np.all((got["pit_mid"] >= 0) & (got["pit_mid"] <= 1))


@pytest.mark.parametrize("family", _glm.FAMILIES)
def test_reproducible_over_calls_thin_and_shards(gpu, family):
    c, full = _ragged(family)
    keys, rep = _keys(family), full["replicates"]
    assert _same(full, _pp(c), keys + ("replicates",))
    assert _same(full, _pp(c, replicates=False), keys)
    assert _pp(c, thin=3)["replicates"].tobytes() == rep[:, ::3].tobytes()
    tail = _pp(c, draws=c.draws[1:], chain_offset=CH0 + 1)
    assert tail["replicates"].tobytes() == rep[1:].tobytes()
    late = _pp(c, draws=c.draws[:, 10:], iter_offset=IT0 + 10)
    assert late["replicates"].tobytes() == rep[:, 10:].tobytes()


@pytest.mark.parametrize("family", _glm.FAMILIES)
def test_nan_coefficient_draw(gpu, family):
    c, full = _ragged(family)
    draws = c.draws.copy()
    draws[1, 20, GP.LEAD + 1] = np.nan
    got = _pp(c, draws=draws)
    rep = got["replicates"]
    assert np.all(np.isnan(rep[1, 20])) and np.isnan(rep).sum() == 33
    ok = ~np.isnan(rep)
    assert np.array_equal(rep[ok], full["replicates"][ok])
    assert np.all(got["nonfinite"] == 1) and np.all(got["n"] == 111)
    np.testing.assert_allclose(got["mean"], DS.stats_of(rep, c.d.y)["mean"], rtol=1e-10)


def test_zero_scale_draw(gpu):
    c, full = _ragged("normal")
    draws = c.draws.copy()
    draws[2, 5, -1] = -np.inf               # log_sigma: the scale exp(-inf) = 0 is not > 0
    got = _pp(c, draws=draws)
    rep = got["replicates"]
    assert np.all(np.isnan(rep[2, 5])) and np.isnan(rep).sum() == 33
    assert np.all(got["nonfinite"] == 1) and np.all(got["n"] == 111)
    ok = ~np.isnan(rep)
    assert np.array_equal(rep[ok], full["replicates"][ok])


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
    got = mc.posterior_predictive(c.log_likelihood, predictive_kernel="glm")
    assert got["pit_mid"].shape == (64,) and np.all(got["n"] == 80)
    assert np.all((got["pit_mid"] >= 0) & (got["pit_mid"] <= 1))
    host = _D().posterior_predictive(c.log_likelihood, mc.samples, seed=3, group=False,
                                     predictive_kernel="glm")
    assert _same(got, host, _keys("bernoulli") + ("pit_mid",))


def test_refusals_before_any_launch(gpu):
    from mlx_mcmc_amd import _lib, _trace

    c = GP.case("poisson", 33, 3, 2, 9)
    ns = _glm.ns_product()
    with pytest.raises(ValueError, match=r"exactly one mx\.sum\(Family\(X @ beta"):
        _D().posterior_predictive(
            lambda p: c.log_likelihood(p) + ns.sum(ns.Normal(0.0, 2.0).log_prob(p["w"])),
            c.draws, GP.layout_of(c), group=False, predictive_kernel="glm")
    plain = PP.normal_gather()
    with pytest.raises(ValueError, match="predictive_kernel='glm' takes a design-matrix"):
        _D().posterior_predictive(plain.log_likelihood, plain.draws, PP.layout_of(plain),
                                  group=False, predictive_kernel="glm")
    lib = _lib.load()
    prog = _trace.pointwise_program(plain.log_likelihood, PP.layout_of(plain))
    assert lib.mc_glm_predictive_workspace_bytes(prog.handle, 2, 9, 1) == _lib.MC_ERR_UNSUPPORTED
    assert b"not a design-matrix" in lib.mc_last_error()
    prog = _trace.pointwise_program(c.log_likelihood, GP.layout_of(c))
    assert lib.mc_glm_predictive_workspace_bytes(prog.handle, 2, 9, 0) == _lib.MC_ERR_INVALID
    assert b"thin" in lib.mc_last_error()
    assert lib.mc_glm_predictive_workspace_bytes(prog.handle, 2, 9, 1) == 0
