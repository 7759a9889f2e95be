"""Pointwise log-likelihood and WAIC of softmax regression on the device
(k_glm_softmax_pointwise, csrc/glm_softmax_pointwise.h; pointwise_kernel="glm")
against a float64 NumPy log-softmax of the [C, S, N] matrix.

Matrix bound, per entry: tests/test_gpu_glm_pointwise.py's, carried through the
softmax to first order: ATOL + RTOL |ref| + 2 (P + 4) 2^-24 sum_k |[k = y_i] -
p_ik| A_ik with A_ik = |a_k| + sum_p |X_ip B_pk| — class k's logit carries
gamma_{P+2} A_ik and enters l with weight dl / d eta_k = [k = y] - p_k.  The same
matrix evaluated in float32 NumPy on the CPU sits inside it at every shape here:
worst error / bound 0.011, 0.026, 0.011, 0.003 and 0.021 in the order of SHAPES
(0.026 the worst), so no shape needs a wider bound.  Statistics and WAIC: as in that file."""
import numpy as np
import pytest

import _glm_softmax as G
import _pointwise as PW

pytestmark = pytest.mark.gpu

# (N, P, K, C, S, intercept): one tile, KP = 2, 16 draws per MFMA tile; a padded
# class, ragged rows, R = 111 a multiple of neither 32 nor DPT; PT = 2, KP = 8, an
# idle wave; PT = 8, KP = 32, one draw per tile; K = 17 in KP = 32, R = 600 over
# NT = 5: two draw blocks and k_pw_merge
SHAPES = [(32, 2, 2, 1, 32, False), (33, 3, 3, 3, 37, True), (70, 33, 5, 2, 40, True),
          (40, 256, 32, 1, 33, True), (150, 5, 17, 2, 300, False)]
KW = dict(group=False, pointwise_kernel="glm")


def like_of(d, intercept):
    import mlx_mcmc_amd as m
    import mlx_mcmc_amd.core as mx

    def like(p):
        eta = mx.array(d.X) @ p["B"]
        return mx.sum(m.Categorical(logits=eta + p["a"] if intercept else eta).log_prob(d.y))
    return like


def case(N, P, K, C, S, intercept):
    """(data, likelihood, draws [C, S, D] = (B row-major, a), layout)"""
    from mlx_mcmc_amd import _trace

    d = G.data(N, P, K)
    shapes = {"B": np.zeros((P, K), np.float32)}
    if intercept:
        shapes["a"] = np.zeros(K, np.float32)
    draws = np.random.default_rng(N + P + K).normal(size=(C, S, P * K + K * intercept))
    return d, like_of(d, intercept), draws.astype(np.float32), _trace.layout_of(shapes)


def ref_of(d, q, dt=np.float64):
    """The [C, S, N] matrix in dt and the third term of its bound (float64)."""
    PK = d.P * d.K
    B = q[..., :PK].reshape(q.shape[:2] + (d.P, d.K))
    a = q[..., None, PK:] if q.shape[-1] > PK else np.zeros(d.K, np.float32)
    eta = d.X.astype(dt) @ B.astype(dt) + a.astype(dt)
    ls = eta - eta.max(-1, keepdims=True)
    ls = ls - np.log(np.exp(ls).sum(-1, keepdims=True))
    hot = d.y[:, None] == np.arange(d.K)
    A = np.abs(d.X).astype(np.float64) @ np.abs(B).astype(np.float64) + np.abs(a)
    third = 2 * (d.P + 4) * 2.0 ** -24 * (np.abs(hot - np.exp(ls.astype(np.float64))) * A).sum(-1)
    return ls[..., hot].reshape(ls.shape[:3]), third


def bound_of(ref, third):
    return PW.ATOL + PW.RTOL * np.abs(ref) + third


def pointwise(like, draws, lay, matrix=True):
    from mlx_mcmc_amd import diagnostics

    got = diagnostics.pointwise_log_likelihood(like, draws, lay, matrix=matrix, **KW)
    if matrix:
        got["matrix"] = got["matrix"].cpu().numpy()
    return got


def check_waic(w, ref, third):
    """waic_from_stats' result against the float64 matrix [R, N], each row's bound
    widened by its observation's largest third term over the draws."""
    want = PW.waic_of(ref)
    for key, wkey in (("lppd", "lppd_i"), ("p_waic", "p_waic_i"), ("elpd_waic", "elpd_i")):
        tol = PW.ATOL + PW.RTOL * np.abs(want[wkey]) + third.max(axis=0)
        assert np.all(np.abs(w["pointwise"][key] - want[wkey]) <= tol), key
    assert abs(w["elpd_waic"] - want["elpd_waic"]) <= np.sum(tol)   # (tol: elpd_i's)


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_matrix_statistics_and_waic(gpu, shape):
    from mlx_mcmc_amd import diagnostics

    d, like, draws, lay = case(*shape)
    C, S = draws.shape[:2]
    got = pointwise(like, draws, lay)
    mat = got["matrix"]
    assert mat.shape == (C, S, d.N) and mat.dtype == np.float32
    ref, third = ref_of(d, draws)
    err = np.abs(mat.astype(np.float64) - ref)
    print(f"{shape}: worst matrix error / bound {np.max(err / bound_of(ref, third)):.3f}")
    assert np.all(np.isfinite(mat)) and np.all(err <= bound_of(ref, third))
    own = PW.stats_of(mat)
    for f in PW.FIELDS:
        assert got[f].shape == (d.N,) and got[f].dtype == np.float64
        np.testing.assert_allclose(got[f], own[f], rtol=1e-10, atol=0, err_msg=f)
    assert np.all(got["n"] == C * S) and not got["nonfinite"].any()
    check_waic(diagnostics.waic_from_stats(got), ref.reshape(C * S, d.N),
               third.reshape(C * S, d.N))


def test_nan_coefficient_draw(gpu):
    d, like, draws, lay = case(*SHAPES[1])
    ref, third = ref_of(d, draws)          # the other draws' values are untouched
    bad = draws.copy()
    bad[1, 20, 4] = np.nan                 # B[1, 1] of one draw
    got = pointwise(like, bad, lay)
    for f in ("max", "sumexp", "mean", "m2"):
        assert np.all(np.isnan(got[f])), f
    assert np.all(got["nonfinite"] == 1) and np.all(got["n"] == 111)
    mat = got["matrix"]
    assert np.all(np.isnan(mat[1, 20])) and np.isnan(mat).sum() == 33
    ok = ~np.isnan(mat)
    assert np.all(np.abs(mat - ref)[ok] <= bound_of(ref, third)[ok])


def test_deterministic_with_and_without_matrix(gpu):
    _, like, draws, lay = case(*SHAPES[4])
    first, again = pointwise(like, draws, lay), pointwise(like, draws, lay)
    plain = pointwise(like, draws, lay, matrix=False)
    assert "matrix" not in plain
    assert first["matrix"].tobytes() == again["matrix"].tobytes()
    for f in PW.FIELDS:
        assert first[f].tobytes() == again[f].tobytes() == plain[f].tobytes(), f


def test_waic_after_hmc(gpu):
    import mlx_mcmc_amd as m
    from mlx_mcmc_amd import diagnostics

    d = G.data(64, 3, 3)
    like = like_of(d, True)
    log_prob, init = G.model(G.ns_product(), d)
    mc = m.MCMC(log_prob)
    mc.run(init, num_samples=40, num_warmup=20, method="hmc", step_size=0.1,
           num_leapfrog_steps=5, num_chains=2, random_seed=3, verbose=False, progress=False)
    w = mc.waic(like, pointwise_kernel="glm")                       # the kept device buffer
    host = diagnostics.waic(like, mc.samples, **KW)                 # the host-dict path
    for k in ("elpd_waic", "p_waic", "waic", "se", "lppd", "n_obs", "n_draws", "n_nonfinite"):
        assert w[k] == host[k], k
    assert w["n_obs"] == 64 and w["n_draws"] == 80 and w["n_nonfinite"] == 0
    q = np.concatenate([mc.samples["B"].reshape(2, 40, 9), mc.samples["a"]], axis=2)
    ref, third = ref_of(d, np.asarray(q, np.float32))
    check_waic(w, ref.reshape(80, 64), third.reshape(80, 64))
