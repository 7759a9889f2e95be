"""PSIS-LOO on the device (mc_psis_loo, csrc/psis.h) against the float64 NumPy
restatement of tests/_psis.py, on synthetic draws.

Three comparisons per model, with ``tail=True``:
* the selection — every observation's tail, cutoff, minimum and tail count —
  is bit-equal to ``np.sort`` of the device's own ``matrix=True`` column;
* k-hat, sigma and elpd_loo_i agree at rtol 1e-10 (the project's bar for f64
  reductions) with the restatement applied to that matrix: this isolates the
  fit and the sums from the f32 evaluation;
* against the float64 model, elpd_loo_i and k-hat stay within the project's
  elementwise bar (rtol 2e-6, atol 2e-5; a float32 NumPy restatement of these
  five shapes stays within 0.36 of it on elpd_loo_i, k-hat within 7e-6).

The shapes cross every boundary there is: the 256-observation tile (273
observations), the draw blocks (3 of 37, 6 of 34), a 64-lane wave in the tail
(76), the sort's padding (23 -> 32, 40 -> 64, 76 -> 128, 259 -> 512), a tail
above 256, ties at the cutoff, and the degenerate tails (n = 0, n <= 4, Mt = 0).
"""
import numpy as np
import pytest

import _psis as PS

pytestmark = pytest.mark.gpu

FIELDS = ("elpd_loo", "p_loo", "looic", "se", "lppd", "n_obs", "n_draws", "tail_len", "n_high_k",
          "n_nonfinite")


def _D():
    from mlx_mcmc_amd import diagnostics

    return diagnostics


_cache = {}


def _loo(model, **kw):
    return _D().loo(model.log_likelihood, model.draws, PS.layout_of(model), group=False, **kw)


def _matrix(model):
    got = _D().pointwise_log_likelihood(model.log_likelihood, model.draws, PS.layout_of(model),
                                        matrix=True, group=False)
    return got["matrix"].cpu().numpy().reshape(-1, model.M)


def _run(name, **kw):
    """(model, device loo with tails, the restatement on the device's own
    matrix, the restatement on the float64 model), once per model."""
    key = (name, tuple(sorted(kw.items())))
    if key not in _cache:
        model = getattr(PS, name)(**kw)
        _cache[key] = (model, _loo(model, tail=True), PS.psis_matrix(_matrix(model)),
                       PS.psis_matrix(model.ll(model.draws, np.float64)))
    return _cache[key]


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _check_selection(got, own):
    tail = got["tail"].cpu().numpy()
    assert tail.dtype == np.float32 and tail.shape == own["tail"].shape
    assert np.array_equal(np.isnan(tail), np.isnan(own["tail"]))
    assert _same_bits(np.nan_to_num(tail, nan=0.0), np.nan_to_num(own["tail"], nan=0.0))
    assert _same_bits(got["cutoff"], own["cutoff"])
    assert _same_bits(got["min"], own["min"])
    np.testing.assert_array_equal(got["tail_n"], own["n"])


def _check(name, mt, **kw):
    model, got, own, ref = _run(name, **kw)
    assert got["tail_len"] == mt == own["tail_len"] and got["n_obs"] == model.M
    assert got["n_draws"] == model.draws.shape[0] * model.draws.shape[1]
    _check_selection(got, own)
    pw = got["pointwise"]
    for f, g in (("khat", pw["khat"]), ("sigma", got["sigma"]), ("elpd", pw["elpd_loo"])):
        with np.errstate(all="ignore"):
            dev = np.nanmax(np.abs(g - own[f]) / np.abs(own[f]))
        print(f"{name}: {f} deviates {dev:.2e} from the restatement on the device's matrix")
        np.testing.assert_allclose(g, own[f], rtol=1e-10, atol=0, err_msg=f)
    print(f"{name}: against the float64 model elpd_loo_i {PS.frac(pw['elpd_loo'], ref['elpd']):.3f}"
          f" of the bar, khat {PS.frac(pw['khat'], ref['khat']):.3f} of the bar "
          f"({np.max(np.abs(pw['khat'] - ref['khat'])):.2e} absolute); "
          f"khat in [{pw['khat'].min():.3f}, {pw['khat'].max():.3f}]")
    np.testing.assert_allclose(pw["elpd_loo"], ref["elpd"], rtol=PS.RTOL, atol=PS.ATOL)
    np.testing.assert_allclose(pw["khat"], ref["khat"], rtol=PS.RTOL, atol=PS.ATOL)
    # the summary fields follow from the pointwise terms
    assert got["elpd_loo"] == float(np.sum(pw["elpd_loo"]))
    assert got["p_loo"] == got["lppd"] - got["elpd_loo"] and got["looic"] == -2 * got["elpd_loo"]
    np.testing.assert_array_equal(pw["p_loo"], pw["lppd"] - pw["elpd_loo"])
    np.testing.assert_allclose(got["se"], np.sqrt(model.M * np.var(pw["elpd_loo"])), rtol=1e-13)
    assert got["n_high_k"] == int(np.sum(pw["khat"] > 0.7)) and got["n_nonfinite"] == 0
    return model, got, own, ref


def test_varying_intercept_three_blocks(gpu):
    _check("varying_intercept", 23)


def test_two_terms_two_tiles_and_a_scalar(gpu):
    model, got, _, _ = _check("two_terms_scalar", 40, C=4, S=50)
    assert model.M == 273


def test_tail_longer_than_a_wave(gpu):
    _check("varying_intercept", 76, C=4, S=160)


def test_expression_term_and_a_tail_above_256(gpu):
    _check("logistic", 259, C=8, S=925)


def test_scalar_observation_alone(gpu):
    model, _, _, _ = _check("scalar_only", 23)
    assert model.M == 1


def test_ties_at_the_cutoff_drop_out(gpu):
    model = PS.tied()
    got, own = _loo(model, tail=True), PS.psis_matrix(_matrix(model))
    assert got["tail_len"] == 23
    assert np.all(got["tail_n"] == 22) and np.all(np.isfinite(got["pointwise"]["khat"]))
    _check_selection(got, own)
    np.testing.assert_allclose(got["pointwise"]["khat"], own["khat"], rtol=1e-10, atol=0)
    np.testing.assert_allclose(got["pointwise"]["elpd_loo"], own["elpd"], rtol=1e-10, atol=0)


def test_identical_draws_have_no_tail(gpu):
    model = PS.varying_intercept()
    model.draws[:] = model.draws[0, 0]
    got, mat = _loo(model, tail=True), _matrix(model)
    assert np.all(got["tail_n"] == 0) and np.all(got["pointwise"]["khat"] == np.inf)
    assert np.all(np.isnan(got["tail"].cpu().numpy()))
    np.testing.assert_array_equal(got["pointwise"]["elpd_loo"], mat[0].astype(np.float64))
    assert got["n_high_k"] == model.M


def test_small_run_with_an_out_of_support_draw(gpu):
    model = PS.out_of_support()
    got, own = _loo(model, tail=True), PS.psis_matrix(_matrix(model))
    j = model.bad[2]
    ok = np.arange(model.M) != j
    pw = got["pointwise"]
    assert got["n_draws"] == 18 and got["tail_len"] == 4 and got["n_nonfinite"] == 1
    # at most four tail values: no fit, plain importance sampling
    assert np.all(pw["khat"][ok] == np.inf) and np.all(got["tail_n"][ok] <= 4)
    np.testing.assert_allclose(pw["elpd_loo"][ok], own["elpd"][ok], rtol=1e-10, atol=0)
    x = _matrix(model)[:, ok].astype(np.float64)
    np.testing.assert_allclose(pw["elpd_loo"][ok], -np.log(np.mean(np.exp(-x), axis=0)),
                               rtol=1e-10)
    assert np.isnan(pw["elpd_loo"][j]) and np.isnan(pw["khat"][j])
    assert np.isnan(got["elpd_loo"]) and got["n_high_k"] == model.M - 1


def test_single_draw(gpu):
    model = PS.varying_intercept(C=1, S=1)
    got = _loo(model, tail=True)
    assert got["tail_len"] == 0 and tuple(got["tail"].shape) == (model.M, 0)
    assert np.all(got["tail_n"] == 0) and np.all(got["pointwise"]["khat"] == np.inf)
    np.testing.assert_array_equal(got["pointwise"]["elpd_loo"],
                                  _matrix(model)[0].astype(np.float64))


@pytest.mark.parametrize("name,kw", [("two_terms_scalar", {"C": 4, "S": 50}),
                                     ("logistic", {"C": 8, "S": 925})])
def test_deterministic_with_and_without_the_tail(gpu, name, kw):
    model, got, _, _ = _run(name, **kw)
    again, plain = _loo(model, tail=True), _loo(model)
    assert "tail" not in plain and "cutoff" not in plain
    for f in ("elpd_loo", "p_loo", "lppd", "khat"):
        assert _same_bits(got["pointwise"][f], again["pointwise"][f]), f
        assert _same_bits(got["pointwise"][f], plain["pointwise"][f]), f
    for f in FIELDS:
        assert got[f] == again[f] == plain[f], f
    for f in ("cutoff", "min", "sigma", "tail_n"):
        assert _same_bits(got[f], again[f]), f
    assert _same_bits(got["tail"].cpu().numpy(), again["tail"].cpu().numpy())


def test_a_tail_beyond_the_capacity_is_refused_before_any_launch(gpu):
    from mlx_mcmc_amd import _lib, _trace

    model = PS.scalar_only()
    prog = _trace.pointwise_program(model.log_likelihood, PS.layout_of(model))
    lib = _lib.load()
    rc = lib.mc_psis_workspace_bytes(prog.handle, 1 << 15, 1 << 15, 1.0)
    assert rc == _lib.MC_ERR_UNSUPPORTED and b"kPsisMaxTail" in lib.mc_last_error()
    assert lib.mc_psis_tail_len(1 << 30, 1.0) == 98304
    # the largest tail that fits
    assert lib.mc_psis_workspace_bytes(prog.handle, 1, 466000, 1.0) > 2048 * 4


def test_end_to_end_loo_after_hmc(gpu):
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
    res = mc.loo(ll)                                       # the kept device buffer
    host = _D().loo(ll, mc.samples, group=False)           # the host-dict path
    for k in FIELDS:
        assert res[k] == host[k], k
    for k in ("elpd_loo", "p_loo", "lppd", "khat"):
        assert _same_bits(res["pointwise"][k], host["pointwise"][k]), k
    assert res["n_obs"] == 100 and res["n_draws"] == 200 and res["tail_len"] == 40
    assert res["n_nonfinite"] == 0 and res["p_loo"] == res["lppd"] - res["elpd_loo"]
    st = mc.pointwise_log_likelihood(ll, matrix=True)
    own = PS.psis_matrix(st["matrix"].cpu().numpy())
    pw = res["pointwise"]
    print(f"end to end: khat in [{pw['khat'].min():.3f}, {pw['khat'].max():.3f}], "
          f"tail counts in [{own['n'].min():.0f}, {own['n'].max():.0f}], "
          f"elpd_loo {res['elpd_loo']:.4f}, p_loo {res['p_loo']:.4f}")
    np.testing.assert_allclose(pw["khat"], own["khat"], rtol=1e-10, atol=0)
    np.testing.assert_allclose(pw["elpd_loo"], own["elpd"], rtol=1e-10, atol=0)
    assert _D().compare(res, mc.loo(ll)) == {"elpd_diff": 0.0, "se_diff": 0.0, "n_obs": 100}

