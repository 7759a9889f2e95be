"""Float64 NumPy restatement of PSIS-LOO as the project defines it
(include/mcmc355.h, "PSIS-LOO over kept draws", steps 1-8), shared by
tests/test_psis_host.py and tests/test_gpu_psis.py.  The models are those of
tests/_pointwise.py.

``psis_matrix`` takes a [R, M] (or [C, S, M]) matrix of pointwise values: the
selection (sort, cutoff, strict tail) happens in the matrix's own dtype, all
arithmetic after it in float64.  ``reverse=True`` sums every sum over the tail
in the opposite order: the spread between the two orders is what a change of
summation order can cost.
"""
from __future__ import annotations

import math

import numpy as np

from _pointwise import (ATOL, RTOL, layout_of, logistic, out_of_support,  # noqa: F401
                        scalar_only, two_terms_scalar, varying_intercept)

FIELDS = ("elpd", "khat", "sigma", "cutoff", "min", "n")
TAIL_LENS = {1: 0, 2: 1, 5: 1, 20: 4, 21: 5, 111: 23, 200: 40, 640: 76, 7400: 259,
             256000: 1518}


def tail_len(N, r_eff=1.0):
    return min(int(math.ceil(min(N / 5.0, 3.0 * math.sqrt(N / r_eff)))), N - 1)


def _sum(a, reverse, axis=-1):
    return np.sum(np.flip(a, axis=axis) if reverse else a, axis=axis)


def gpd_fit(y, reverse=False):
    """(khat, sigma) of ascending float64 exceedances y (step 5)."""
    y = np.asarray(y, np.float64)
    n = y.size
    if n <= 4:
        return np.inf, np.nan
    with np.errstate(all="ignore"):
        m = 30 + int(math.floor(math.sqrt(n)))
        i = np.arange(1, m + 1, dtype=np.float64)
        yq = y[int(math.floor(n / 4.0 + 0.5)) - 1]
        b = (1.0 - np.sqrt(m / (i - 0.5))) / (3.0 * yq) + 1.0 / y[-1]
        kap = _sum(np.log1p(-b[:, None] * y[None, :]), reverse) / n
        ll = n * (np.log(-b / kap) - kap - 1.0)
        w = 1.0 / np.sum(np.exp(ll[None, :] - ll[:, None]), axis=1)
        w = w / np.sum(w)
        bbar = np.sum(w * b)
        kbar = _sum(np.log1p(-bbar * y), reverse) / n
        return (n * kbar + 5.0) / (n + 10.0), -kbar / bbar


def log_weights(t, khat, sigma, lmin, ec):
    """The tail's log weights in rank order (step 6); t is the tail in
    decreasing order, float64."""
    n = t.size
    if not (np.isfinite(khat) and sigma > 0):
        return lmin - t
    with np.errstate(all="ignore"):
        l1 = np.log1p(-(np.arange(1, n + 1) - 0.5) / n)
        q = -sigma * l1 if abs(khat) < np.finfo(np.float64).eps \
            else sigma * np.expm1(-khat * l1) / khat
        return np.minimum(np.log(q + ec), 0.0)


def psis_column(col, r_eff=1.0, reverse=False):
    """Steps 1-8 for one observation's values over the draws."""
    x = np.asarray(col).ravel() + 0.0            # (-0 taken as +0)
    N = x.size
    mt = tail_len(N, r_eff)
    s = np.sort(x)
    L, lmin = s[mt], s[0]
    tail = s[s < L]
    n = tail.size
    out = {"cutoff": float(L), "min": float(lmin), "n": n, "tail": tail, "tail_len": mt}
    if not np.all(np.isfinite(x)):
        out.update(elpd=np.nan, khat=np.nan, sigma=np.nan, lw=np.full(n, np.nan))
        return out
    with np.errstate(all="ignore"):
        L, lmin = np.float64(L), np.float64(lmin)
        t = tail[::-1].astype(np.float64)
        ec = np.exp(lmin - L)
        khat, sigma = gpd_fit(np.exp(lmin - t) - ec, reverse)
        lw = log_weights(t, khat, sigma, lmin, ec)
        rest = x[x >= L].astype(np.float64)
        num = (N - n) + _sum(np.exp(t + lw - lmin), reverse)
        den = _sum(np.exp(lw), reverse) + np.sum(np.exp(lmin - rest))
        out.update(elpd=float((np.log(num) - np.log(den)) + lmin), khat=float(khat),
                   sigma=float(sigma), lw=lw)
    return out


def psis_matrix(mat, r_eff=1.0, reverse=False):
    """Per-observation arrays of the fields, and the [M, Mt] tails (ascending,
    NaN past each length) as the device lays them out."""
    x = np.asarray(mat)
    x = x.reshape(-1, x.shape[-1])
    cols = [psis_column(x[:, o], r_eff, reverse) for o in range(x.shape[1])]
    mt = cols[0]["tail_len"]
    tails = np.full((x.shape[1], mt), np.nan, x.dtype)
    for o, c in enumerate(cols):
        tails[o, :c["n"]] = c["tail"]
    out = {f: np.array([c[f] for c in cols], np.float64) for f in FIELDS}
    out.update(tail=tails, tail_len=mt, cols=cols)
    return out


def frac(got, ref):
    """Largest error as a fraction of the elementwise bar, over finite reference entries."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    ok = np.isfinite(ref)
    if not ok.any():
        return 0.0
    return float(np.max(np.abs(got[ok] - ref[ok]) / (ATOL + RTOL * np.abs(ref[ok]))))


def tied(model_fn=varying_intercept):
    """varying_intercept's draws extended to S = 38 with every odd draw a copy
    of the even one before it (rejected proposals repeat draws)."""
    model = model_fn(S=38)
    model.draws[:, 1::2] = model.draws[:, 0::2]
    return model
