"""NumPy restatement of the posterior predictive definition (include/mcmc355.h,
csrc/predictive.h) and the models of tests/test_predictive_host.py and
tests/test_gpu_predictive.py.

``normal_draw`` / ``halfnormal_draw`` / ``exponential_draw`` restate the three
closed-form samplers in float32 through oracle/philox.py (bit for bit);
``host_draws`` applies the library's own scalar definition
(``mc_predictive_draw``) to arrays of operands; ``stats_of`` reduces a matrix
of replicates in float64.  Each model gives the product's
``log_likelihood(params)``, the parameter shapes, seeded synthetic draws
[C, S, D] and ``operands(q)``: per observation and draw the distribution code
and the float32 (value, loc / alpha, scale / rate / beta) the kernel forms.
"""
from __future__ import annotations

import ctypes
from types import SimpleNamespace

import numpy as np

from oracle import philox as R

TAG_PREDICT = 7
FIELDS = ("n", "mean", "m2", "below", "nonfinite")
NORMAL, HALFNORMAL, EXPONENTIAL, GAMMA, BETA = range(5)
F32 = np.float32


def _mx():
    import mlx_mcmc_amd as m
    import mlx_mcmc_amd.core as mx

    return m, mx


# ---- the closed-form samplers in float32 ---------------------------------------
def _z0(seed, chain, it, obs):
    w = R.draw(seed, chain, it, TAG_PREDICT, 0, obs)
    return R.box_muller(w[..., 0], w[..., 1])[0]


def normal_draw(loc, scale, seed, chain, it, obs):
    return (F32(loc) + F32(scale) * _z0(seed, chain, it, obs)).astype(F32)


def halfnormal_draw(scale, seed, chain, it, obs):
    return np.abs(F32(scale) * _z0(seed, chain, it, obs)).astype(F32)


def exponential_draw(rate, seed, chain, it, obs):
    w = R.draw(seed, chain, it, TAG_PREDICT, 0, obs)
    return (-R.logf_unit(R.u01_boxf(w[..., 0])) / F32(rate)).astype(F32)


# ---- the library's scalar definition over arrays ---------------------------------
def host_draw(dist, m, s, seed, chain, it, obs):
    from mlx_mcmc_amd import _lib

    out = ctypes.c_float()
    rc = _lib.load().mc_predictive_draw(int(dist), float(m), float(s), int(seed), int(chain),
                                        int(it), int(obs), ctypes.byref(out))
    assert rc == 0, rc
    return F32(out.value)


def host_draws(dist, m, s, seed, chain, it, obs):
    """mc_predictive_draw over broadcast arrays (float32 out)."""
    from mlx_mcmc_amd import _lib

    fn = _lib.load().mc_predictive_draw
    args = np.broadcast_arrays(np.asarray(dist), np.asarray(m, F32), np.asarray(s, F32),
                               np.asarray(chain), np.asarray(it), np.asarray(obs))
    res = np.empty(args[0].shape, F32)
    out = ctypes.c_float()
    ref = ctypes.byref(out)
    flat = res.reshape(-1)
    seed = int(seed)
    for k, (d, a, b, c, i, o) in enumerate(zip(*(x.reshape(-1).tolist() for x in args))):
        assert fn(d, a, b, seed, c, i, o, ref) == 0
        flat[k] = out.value
    return res


def model_host_replicates(model, seed, chain_offset=0, iter_offset=0, q=None):
    """[C, S, M] float32: the host definition at the model's operand values."""
    dist, _, m, s = model.operands(model.draws if q is None else q)
    C, S, M = m.shape
    return host_draws(dist, m, s, seed, np.arange(C)[:, None, None] + chain_offset,
                      np.arange(S)[None, :, None] + iter_offset, np.arange(M)[None, None, :])


# ---- statistics of a matrix of replicates ---------------------------------------
def stats_of(rep, value):
    """The five statistics of [.., M] replicates against [.., M] observations
    (float64; the moments over the finite replicates, NaN when there is none)."""
    x = np.asarray(rep, np.float64).reshape(-1, rep.shape[-1])
    v = np.broadcast_to(np.asarray(value, np.float64), rep.shape).reshape(x.shape)
    fin = np.isfinite(x)
    nfin = fin.sum(axis=0).astype(np.float64)
    with np.errstate(all="ignore"):
        mean = np.where(fin, x, 0.0).sum(axis=0) / nfin
        m2 = np.where(fin, (x - mean) ** 2, 0.0).sum(axis=0)
        m2 = np.where(nfin > 0, m2, np.nan)
    return {"n": np.full(x.shape[1], float(x.shape[0])), "mean": mean, "m2": m2,
            "below": (fin & (x < v)).sum(axis=0).astype(np.float64),
            "nonfinite": (~fin).sum(axis=0).astype(np.float64)}


# ---- models --------------------------------------------------------------------
def _cols(rng, C, S, cols):
    """[C, S, D] float32 draws: N(0, 1) for "n", uniform in [lo, hi] for (lo, hi)."""
    out = []
    for kind, width in cols:
        if kind == "n":
            out.append(rng.standard_normal((C, S, width)))
        else:
            out.append(rng.uniform(kind[0], kind[1], (C, S, width)))
    return np.concatenate(out, axis=2).astype(F32)


def _bc(x, shape):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(x, F32), shape))


def _stack(C, S, terms):
    """Concatenate per-term (dist, value, m, s) to [C, S, M] arrays."""
    ds, vs, ms, ss = [], [], [], []
    for dist, n, v, m, s in terms:
        shp = (C, S, n)
        ds.append(np.full(shp, dist, np.int64))
        vs.append(_bc(v, shp))
        ms.append(_bc(m, shp))
        ss.append(_bc(s, shp))
    return tuple(np.concatenate(a, axis=2) for a in (ds, vs, ms, ss))


def normal_gather(C=3, S=37, G=5, N=259, seed=21, bad=()):
    """Normal(alpha[g], sigma).log_prob(y): 259 = 256 + 3 elements (two tiles),
    g unsorted and non-injective, a raw scalar scale.  ``bad``: (c, s, value)
    triples that overwrite sigma (a non-positive scale)."""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, G, N).astype(np.int32)
    g[:G] = np.arange(G)[::-1]
    y = rng.standard_normal(N).astype(F32)

    def log_likelihood(p):
        m, mx = _mx()
        return mx.sum(m.Normal(p["alpha"][g], p["sigma"]).log_prob(y))

    def operands(q):
        C_, S_ = q.shape[:2]
        return _stack(C_, S_, [(NORMAL, N, y, q[..., :G][..., g], q[..., G:G + 1])])

    draws = _cols(rng, C, S, [("n", G), ((0.5, 2.0), 1)])
    for c, s, val in bad:
        draws[c, s, G] = val
    return SimpleNamespace(log_likelihood=log_likelihood, shapes={"alpha": (G,), "sigma": ()},
                           draws=draws, operands=operands, M=N)


def mixed(C=3, S=37, lo=1.0, hi=4.0, seed=22):
    """A Gamma term of 13 elements whose shape follows the draw (mean: weight
    1 / 13, ignored by a replicate), a scalar Exponential observation, a Beta
    term of 5 elements with both shapes following the draw and a HalfNormal
    term of 7.  Shapes uniform in [lo, hi]: >= 1 (bit equality with the host)
    or < 1 (the boosted Gamma)."""
    rng = np.random.default_rng(seed)
    t = rng.uniform(0.2, 3.0, 13).astype(F32)
    b = rng.uniform(0.05, 0.95, 5).astype(F32)
    h = np.abs(rng.standard_normal(7)).astype(F32)
    y0 = 0.75

    def log_likelihood(p):
        m, mx = _mx()
        return (mx.mean(m.Gamma(p["a"], 1.5).log_prob(t))
                + m.Exponential(p["rate"]).log_prob(y0)
                + mx.sum(m.Beta(p["ba"], p["bb"]).log_prob(b))
                + mx.sum(m.HalfNormal(p["hs"]).log_prob(h)))

    def operands(q):
        C_, S_ = q.shape[:2]
        return _stack(C_, S_, [(GAMMA, 13, t, q[..., 0:1], 1.5),
                               (EXPONENTIAL, 1, y0, 0.0, q[..., 1:2]),
                               (BETA, 5, b, q[..., 2:3], q[..., 3:4]),
                               (HALFNORMAL, 7, h, 0.0, q[..., 4:5])])

    shapes = {"a": (), "rate": (), "ba": (), "bb": (), "hs": ()}
    draws = _cols(rng, C, S, [((lo, hi), 1), ((0.3, 3.0), 1), ((lo, hi), 2), ((0.5, 2.0), 1)])
    return SimpleNamespace(log_likelihood=log_likelihood, shapes=shapes, draws=draws,
                           operands=operands, M=26, sizes=(13, 1, 5, 7))


def affine(C=3, S=37, G=5, N=67, seed=23, transformed=False):
    """Normal(alpha[g] + beta * x, sigma).log_prob(y), 67 elements: the affine
    loc's two roundings.  ``transformed``: sigma = mx.exp(log_sigma); operands
    then carry the transform in float64 (compared at rtol 1e-6)."""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, G, N).astype(np.int32)
    g[:G] = np.arange(G)[::-1]
    x = rng.standard_normal(N).astype(F32)
    y = rng.standard_normal(N).astype(F32)

    def log_likelihood(p):
        m, mx = _mx()
        sc = mx.exp(p["log_sigma"]) if transformed else p["sigma"]
        return mx.sum(m.Normal(p["alpha"][g] + p["beta"] * x, sc).log_prob(y))

    def operands(q):
        C_, S_ = q.shape[:2]
        loc = (q[..., :G][..., g] + (q[..., G:G + 1] * x).astype(F32)).astype(F32)
        sc = q[..., G + 1:G + 2]
        if transformed:
            sc = np.exp(sc.astype(np.float64))      # (float64: not rounded to f32)
            d, v, m, _ = _stack(C_, S_, [(NORMAL, N, y, loc, 1.0)])
            return d, v, m, np.broadcast_to(sc, m.shape)
        return _stack(C_, S_, [(NORMAL, N, y, loc, sc)])

    name = "log_sigma" if transformed else "sigma"
    rng_s = (-0.5, 0.5) if transformed else (0.5, 2.0)
    draws = _cols(rng, C, S, [("n", G + 1), (rng_s, 1)])
    return SimpleNamespace(log_likelihood=log_likelihood,
                           shapes={"alpha": (G,), "beta": (), name: ()}, draws=draws,
                           operands=operands, M=N)


def exp_scale(C=3, S=37, seed=24):
    """HalfNormal(exp(log_s)) of 7 elements and a scalar Exponential(exp(log_r)):
    the transformed operand is the whole of the replicate's scale (no loc to
    cancel against), operands in float64."""
    rng = np.random.default_rng(seed)
    h = np.abs(rng.standard_normal(7)).astype(F32)
    y0 = 0.4

    def log_likelihood(p):
        m, mx = _mx()
        return (mx.sum(m.HalfNormal(mx.exp(p["log_s"])).log_prob(h))
                + m.Exponential(mx.exp(p["log_r"])).log_prob(y0))

    def operands(q):
        C_, S_ = q.shape[:2]
        d, v, m, _ = _stack(C_, S_, [(HALFNORMAL, 7, h, 0.0, 1.0), (EXPONENTIAL, 1, y0, 0.0, 1.0)])
        e = np.exp(q.astype(np.float64))
        s = np.concatenate([np.broadcast_to(e[..., 0:1], (C_, S_, 7)), e[..., 1:2]], axis=2)
        return d, v, m, s

    draws = _cols(rng, C, S, [((-0.5, 0.5), 2)])
    return SimpleNamespace(log_likelihood=log_likelihood, shapes={"log_s": (), "log_r": ()},
                           draws=draws, operands=operands, M=8)


def layout_of(model):
    from mlx_mcmc_amd import _trace

    return _trace.layout_of({k: np.zeros(s, F32) for k, s in model.shapes.items()})
