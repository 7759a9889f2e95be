"""Float64 NumPy restatement of the pointwise log-likelihood statistics and
WAIC (diagnostics.pointwise_log_likelihood / waic), shared by
tests/test_pointwise_host.py and tests/test_gpu_pointwise.py.

Each model gives the product's ``log_likelihood(params)`` (traced), the
parameter shapes, seeded synthetic draws [C, S, D] and ``ll(draws, dtype)``:
the [C, S, M] matrix of per-observation values in the user's observation
order, evaluated in ``dtype`` (float64: the reference; float32: what the
tolerance of an f32 evaluation is measured with).  ``stats_of`` / ``waic_of``
reduce a matrix with plain NumPy: log(sum(exp(x - max))) after a max shift,
mean, var(ddof=1).
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np

FIELDS = ("max", "sumexp", "n", "mean", "m2", "nonfinite")
# the project's bar for elementwise f32 log_prob against float64
# (tests/test_gpu_dists_ext.py)
RTOL, ATOL = 2e-6, 2e-5

_gammaln = np.vectorize(math.lgamma, otypes=[np.float64])


def _mx():
    import mlx_mcmc_amd as m
    import mlx_mcmc_amd.core as mx

    return m, mx


# ---- log densities in a NumPy dtype ------------------------------------------
def normal_lp(v, m, s, dt):
    c = dt(-0.5) * np.log(dt(2.0) * dt(np.pi))
    d = v - m
    return (c - np.log(s)) - (dt(0.5) * d * d) / (s * s)


def halfnormal_lp(v, s, dt):
    with np.errstate(all="ignore"):
        lp = np.log(dt(2.0)) + normal_lp(v, dt(0.0), s, dt)
    return np.where(v >= 0, lp, -np.inf).astype(dt)


def gamma_lp(v, a, b, dt):
    lg = _gammaln(np.asarray(a, np.float64)).astype(dt)
    return ((a * np.log(b) - lg) + (a - dt(1.0)) * np.log(v)) - b * v


# ---- statistics and WAIC from a matrix ---------------------------------------
def stats_of(ll):
    """The six statistics of a [C, S, M] (or [R, M]) matrix, float64."""
    x = np.asarray(ll, np.float64).reshape(-1, ll.shape[-1])
    with np.errstate(all="ignore"):
        mx = np.max(x, axis=0)
        e = np.exp(x - mx)
        e[np.isneginf(x)] = 0.0          # a -inf draw adds nothing (also when max = -inf)
        mean = np.mean(x, axis=0)
        m2 = np.var(x, axis=0) * x.shape[0]
    return {"max": mx, "sumexp": np.sum(e, axis=0), "n": np.full(x.shape[1], float(x.shape[0])),
            "mean": mean, "m2": m2,
            "nonfinite": np.sum(~np.isfinite(x), axis=0).astype(np.float64)}


def waic_of(ll):
    """WAIC from the matrix (Vehtari, Gelman and Gabry 2017)."""
    x = np.asarray(ll, np.float64).reshape(-1, ll.shape[-1])
    R, M = x.shape
    with np.errstate(all="ignore"):
        mx = np.max(x, axis=0)
        lppd_i = np.log(np.sum(np.exp(x - mx), axis=0)) + mx - np.log(R)
        p_i = np.var(x, axis=0, ddof=1) if R > 1 else np.full(M, np.nan)
        elpd_i = lppd_i - p_i
    return {"elpd_waic": float(np.sum(elpd_i)), "p_waic": float(np.sum(p_i)),
            "waic": float(-2.0 * np.sum(elpd_i)), "se": float(np.sqrt(M * np.var(elpd_i))),
            "lppd": float(np.sum(lppd_i)), "lppd_i": lppd_i, "p_waic_i": p_i, "elpd_i": elpd_i}


# ---- models ------------------------------------------------------------------
def _draws(rng, C, S, cols):
    """[C, S, D] float32 draws: N(0, 1), or uniform in [lo, hi] for (lo, hi) columns."""
    out = []
    for kind, width in cols:
        if kind == "n":
            out.append(rng.standard_normal((C, S, width)))
        else:
            out.append(rng.uniform(kind[0], kind[1], (C, S, width)))
    return np.concatenate(out, axis=2).astype(np.float32)


def varying_intercept(C=3, S=37, G=5, N=67, seed=11):
    """Normal(alpha[g] + beta * x, exp(log_sigma)).log_prob(y): g unsorted and
    non-injective; 67 = one wave and a ragged tail; 111 draws."""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, G, N).astype(np.int32)
    g[:G] = np.arange(G)[::-1]            # every group used, unsorted from the start
    x = rng.standard_normal(N).astype(np.float32)
    y = rng.standard_normal(N).astype(np.float32)

    def log_likelihood(p):
        m, mx = _mx()
        return mx.sum(m.Normal(p["alpha"][g] + p["beta"] * x, mx.exp(p["log_sigma"])).log_prob(y))

    def ll(q, dt):
        q = q.astype(dt)
        loc = q[..., :G][..., g] + q[..., G:G + 1] * x.astype(dt)
        return normal_lp(y.astype(dt), loc, np.exp(q[..., G + 1:G + 2]), dt)

    shapes = {"alpha": (G,), "beta": (), "log_sigma": ()}
    draws = _draws(rng, C, S, [("n", G + 1), ((-0.5, 0.5), 1)])
    return SimpleNamespace(log_likelihood=log_likelihood, shapes=shapes, draws=draws, ll=ll, M=N)


def two_terms_scalar(C=3, S=37, n_gamma=13, n_normal=259, seed=12):
    """mean of a Gamma term with a per-element (data) shape (weight 1 / 13), a
    Normal term of two tiles (259 = 256 + 3), and one scalar observation."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(1.0, 4.0, n_gamma).astype(np.float32)
    t = rng.uniform(0.2, 3.0, n_gamma).astype(np.float32)
    y = rng.standard_normal(n_normal).astype(np.float32)
    y0 = 0.75

    def log_likelihood(p):
        m, mx = _mx()
        return (mx.mean(m.Gamma(a, mx.exp(p["log_rate"])).log_prob(t))
                + mx.sum(m.Normal(p["mu"], 1.5).log_prob(y))
                + m.Normal(p["mu"], 2.0).log_prob(y0))

    def ll(q, dt):
        q = q.astype(dt)
        mu, rate = q[..., 0:1], np.exp(q[..., 1:2])
        w = dt(np.float32(1.0) / np.float32(n_gamma))      # mx.mean: the f32 reciprocal
        return np.concatenate([
            w * gamma_lp(t.astype(dt), a.astype(dt), rate, dt),
            normal_lp(y.astype(dt), mu, dt(1.5), dt),
            normal_lp(dt(y0), mu, dt(2.0), dt)], axis=-1)

    shapes = {"mu": (), "log_rate": ()}
    draws = _draws(rng, C, S, [("n", 1), ((-0.5, 0.5), 1)])
    return SimpleNamespace(log_likelihood=log_likelihood, shapes=shapes, draws=draws, ll=ll,
                           M=n_gamma + n_normal + 1, sizes=(n_gamma, n_normal, 1))


def scalar_only(C=3, S=37, seed=13):
    """One scalar observation: M = 1 as its own program."""
    rng = np.random.default_rng(seed)
    y0 = -0.4

    def log_likelihood(p):
        m, _ = _mx()
        return m.Normal(p["mu"], 2.0).log_prob(y0)

    def ll(q, dt):
        return normal_lp(dt(y0), q.astype(dt)[..., 0:1], dt(2.0), dt)

    return SimpleNamespace(log_likelihood=log_likelihood, shapes={"mu": ()},
                           draws=_draws(rng, C, S, [("n", 1)]), ll=ll, M=1)


def logistic(C=3, S=37, N=67, seed=14):
    """sum(where(Y, log(p), log1p(-p))), p = sigmoid(b0 + b1 * x): an expression term."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(N).astype(np.float32)
    Y = (rng.uniform(size=N) < 0.5).astype(np.float32)

    def log_likelihood(p):
        _, mx = _mx()
        pr = mx.sigmoid(p["b0"] + p["b1"] * x)
        return mx.sum(mx.where(Y, mx.log(pr), mx.log1p(-pr)))

    def ll(q, dt):
        q = q.astype(dt)
        pr = dt(1.0) / (dt(1.0) + np.exp(-(q[..., 0:1] + q[..., 1:2] * x.astype(dt))))
        return np.where(Y != 0, np.log(pr), np.log1p(-pr)).astype(dt)

    return SimpleNamespace(log_likelihood=log_likelihood, shapes={"b0": (), "b1": ()},
                           draws=_draws(rng, C, S, [("n", 2)]), ll=ll, M=N)


def out_of_support(C=2, S=9, n=5, seed=15):
    """HalfNormal(2).log_prob(z) over a latent vector z: one draw puts z[2]
    below 0, outside the support."""
    rng = np.random.default_rng(seed)

    def log_likelihood(p):
        m, mx = _mx()
        return mx.sum(m.HalfNormal(2.0).log_prob(p["z"]))

    def ll(q, dt):
        return halfnormal_lp(q.astype(dt), dt(2.0), dt)

    draws = np.abs(_draws(rng, C, S, [("n", n)])) + np.float32(0.1)
    draws[1, 4, 2] = -0.3
    return SimpleNamespace(log_likelihood=log_likelihood, shapes={"z": (n,)}, draws=draws, ll=ll,
                           M=n, bad=(1, 4, 2))


def layout_of(model):
    from mlx_mcmc_amd import _trace

    return _trace.layout_of({k: np.zeros(s, np.float32) for k, s in model.shapes.items()})
