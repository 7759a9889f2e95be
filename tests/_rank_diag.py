"""Float64 restatement of the rank-normalised diagnostics (Vehtari, Gelman,
Simpson, Carpenter and Buerkner 2021) as include/mcmc355.h states them for
mc_rank_diag, with scipy's rankdata / ndtri and direct autocovariance sums; a
generator of AR(1) chains; and the sequence rule with its decision margin."""
import numpy as np
from scipy.special import ndtri
from scipy.stats import rankdata

PHIS = (0.0, 0.5, 0.95, -0.5)


def ar1_chains(seed, C, S, D):
    """[C, S, D] float32: element d is AR(1) with phi = PHIS[d % 4], unit
    marginal variance; the phi = 0.5 elements are rounded to quarters (many
    ties)."""
    rng = np.random.default_rng(seed)
    x = np.empty((C, S, D))
    for d in range(D):
        phi = PHIS[d % 4]
        e = rng.standard_normal((C, S))
        x[:, 0, d] = e[:, 0]
        for s in range(1, S):
            x[:, s, d] = phi * x[:, s - 1, d] + np.sqrt(1 - phi * phi) * e[:, s]
        if phi == 0.5:
            x[:, :, d] = np.round(x[:, :, d] * 4) / 4
    return x.astype(np.float32)


def split(x):
    """[C, S] -> [2C, n]: draws [0, h) and [S - h, S) of every chain, h = S // 2."""
    C, S = x.shape
    h = S // 2
    return np.stack([x[:, :h], x[:, S - h:]], axis=1).reshape(2 * C, h)


def zscores(y):
    """Normal scores of the average ranks of y [m, n] among all its values."""
    r = rankdata(np.asarray(y).ravel(), method="average")
    return ndtri((r - 0.375) / (r.size + 0.25)).reshape(np.shape(y))


def rhat(y):
    y = np.asarray(y, np.float64)
    m, n = y.shape
    W = np.mean(np.var(y, axis=1, ddof=1))
    Bn = np.var(np.mean(y, axis=1), ddof=1)
    if not W > 0:
        return np.nan
    return np.sqrt(((n - 1) / n * W + Bn) / W)


def geyer(rho, n, N):
    """The sequence rule on rho[0 .. n-1] (rho[0] = 1): (ESS, margin), margin
    the smallest |even + odd| over the pairs the loop tested and the final
    |even|."""
    r = np.zeros(n + 2)
    even, odd = 1.0, float(rho[1])
    r[0], r[1] = even, odd
    t = 1
    margin = np.inf
    while t < n - 3:
        margin = min(margin, abs(even + odd))
        if not even + odd > 0:
            break
        even, odd = float(rho[t + 1]), float(rho[t + 2])
        if even + odd >= 0:
            r[t + 1], r[t + 2] = even, odd
        t += 2
    if t > 1:   # the last pair read: whether the first loop wrote it
        margin = min(margin, abs(even + odd))
    max_t = t - 2
    margin = min(margin, abs(even))
    if even > 0:
        r[max_t + 1] = even
    t = 1
    while t <= max_t - 2:
        if r[t + 1] + r[t + 2] > r[t - 1] + r[t]:
            r[t + 1] = r[t + 2] = (r[t - 1] + r[t]) / 2
        t += 2
    tau = -1 + 2 * np.sum(r[:max_t + 1]) + r[max_t + 1]
    tau = max(tau, 1 / np.log10(N))
    return N / tau, margin


def rhos(y):
    """(rho[0 .. n-1], W) of y [m, n] by direct autocovariance sums; W = 0: (None, 0)."""
    y = np.asarray(y, np.float64)
    m, n = y.shape
    v = y - y.mean(axis=1, keepdims=True)
    a = np.array([np.mean(np.sum(v[:, :n - t] * v[:, t:], axis=1) / n) for t in range(n)])
    W = a[0] * n / (n - 1)
    if not W > 0:
        return None, 0.0
    vp = (n - 1) / n * W + np.var(y.mean(axis=1), ddof=1)
    rho = 1 - (W - a) / vp
    rho[0] = 1.0
    return rho, W


def ess(y):
    """(ESS, margin) of y [m, n]; (NaN, inf) where W = 0."""
    rho, W = rhos(y)
    if rho is None:
        return np.nan, np.inf
    m, n = np.shape(y)
    return geyer(rho, n, m * n)


FIELDS = ("rhat_bulk", "rhat_folded", "rhat_rank", "ess_bulk", "ess_tail")


def element(x):
    """The five outputs of one element x [C, S] float32, its bulk z-scores
    [2C, n], whether it is constant, and the smallest decision margin of its
    three ESS computations."""
    x = np.asarray(x, np.float32)
    y = split(x)
    m, n = y.shape
    nan = {f: np.nan for f in FIELDS}
    if n < 4:
        return nan, np.full((m, n), np.nan), False, np.inf
    if np.isnan(y).any():
        return nan, None, False, np.inf
    with np.errstate(all="ignore"):
        med = np.median(y.ravel())
        # (scalar percentiles: numpy then forms the virtual index in float32)
        q05, q95 = np.percentile(y.ravel(), 5.0), np.percentile(y.ravel(), 95.0)
        assert med.dtype == q05.dtype == q95.dtype == np.float32
        z = zscores(y)
        zf = zscores(np.abs(y - med))
        eb, m0 = ess(z)
        e05, m1 = ess((y <= q05).astype(np.float64))
        e95, m2 = ess((y <= q95).astype(np.float64))
        rb, rf = rhat(z), rhat(zf)
    out = {"rhat_bulk": rb, "rhat_folded": rf, "rhat_rank": np.maximum(rb, rf),
           "ess_bulk": eb, "ess_tail": np.minimum(e05, e95)}
    return out, z, bool(np.all(y == y.ravel()[0])), min(m0, m1, m2)


def buffer(x):
    """element() over a [C, S, D] buffer: ({field: [D]}, z [D, 2C, n] (NaN rows
    for NaN elements), n_constant, margin)."""
    x = np.asarray(x, np.float32)
    C, S, D = x.shape
    res = [element(x[:, :, d]) for d in range(D)]
    out = {f: np.array([r[0][f] for r in res]) for f in FIELDS}
    z = np.stack([r[1] if r[1] is not None else np.full((2 * C, S // 2), np.nan) for r in res])
    return out, z, sum(r[2] for r in res), min(r[3] for r in res)


def classic_split_rhat(x):
    """BDA3 split R-hat of one element x [C, S]."""
    return rhat(split(np.asarray(x, np.float64)))
