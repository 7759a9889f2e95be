"""k_hmc_lf's first moment from per-run constants (test helper).

lanes_fast.h no longer sums M1 = sum_e (x_e - theta) in the sweep: once per
launch a lane forms, for its run of n observations,
    c = (float) (sum_e x_e / n),    R = (float) sum_e (x_e - c)
(both sums in double, in element order) and every step takes
    M1 = fma(n, c - theta, R)                          (float32, lf_m1).
Here: the model of tests/_ragged.py over observations shifted by a constant
(an uncentred sum x - n theta loses the shift's magnitude in float32), the
run patterns, and numpy emulations of the old serial form and of the new form
with their derived bounds.
"""
import numpy as np

from _lf_ends import ENDS
from _lf_rounds import ROUNDS
from _ragged import U, _gamma, ragged_data

# every run under 16 elements (no 16-element round), an empty and a single one
SHORT = [0, 1] + [3 + i for i in range(10)]

PATTERNS = {n: p[0] for n, p in ENDS.items()}
PATTERNS.update({n: p[0] for n, p in ROUNDS.items()})
PATTERNS["short"] = SHORT
SHIFTS = (0.0, 1e3, 1e5)


def shifted_hier(ns, lengths, order="sorted", shift=0.0):
    """(log_prob, init, data) as _ragged.ragged_hier, the observations moved
    by `shift` (rounded to float32: they are the data then)."""
    data = ragged_data(lengths, order)
    y = (data["y"] + np.float32(shift)).astype(np.float32)
    data = {"y": y, "group": data["group"], "G": data["G"]}
    group, G = data["group"], data["G"]

    def log_prob(params):
        mu, tau, sigma, theta = params["mu"], params["tau"], params["sigma"], params["theta"]
        lp = ns.Normal(0, 10).log_prob(mu)
        lp = lp + ns.HalfNormal(5).log_prob(tau)
        lp = lp + ns.HalfNormal(5).log_prob(sigma)
        lp = lp + ns.sum(ns.Normal(mu, tau).log_prob(theta))
        lp = lp + ns.sum(ns.Normal(theta[group], sigma).log_prob(ns.array(y)))
        return lp

    sums = np.bincount(group, weights=y.astype(np.float64), minlength=G)
    counts = np.bincount(group, minlength=G)
    gm = np.where(counts > 0, sums / np.maximum(counts, 1), y.mean()).astype(np.float32)
    init = {"mu": np.float32(gm.mean()), "tau": np.float32(max(gm.std(), 0.5)),
            "sigma": np.float32(1.0), "theta": gm}
    return log_prob, init, data


def runs_of(data):
    """Per group, its observations in data order (a lane's run at one lane
    per parameter)."""
    return [data["y"][data["group"] == g] for g in range(data["G"])]


def fma32(a, b, c):
    """fma(a, b, c) of float32 values, correctly rounded: the product is
    exact in float64, the sum is rounded to odd there (the error of TwoSum
    sets the sticky bit), and 53 bits are more than 24 + 2."""
    p = np.float64(a) * np.float64(b)
    c = np.float64(c)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    if err != 0.0 and not (s.view(np.int64) & 1):
        s = np.nextafter(s, np.inf if err > 0 else -np.inf)
    return np.float32(s)


def run_consts(x):
    """(c, R) of a run, as lanes_fast.h lf_run_consts forms them."""
    n = len(x)
    if n == 0:
        return np.float32(0.0), np.float32(0.0)
    s = np.float64(0.0)
    for v in x:
        s = s + np.float64(v)
    c = np.float32(s / np.float64(n))
    t = np.float64(0.0)
    for v in x:
        t = t + (np.float64(v) - np.float64(c))
    return c, np.float32(t)


def m1_new(x, theta):
    """fma(n, c - theta, R) in float32; an empty run's is 0."""
    if len(x) == 0:
        return np.float32(0.0)
    c, R = run_consts(x)
    return fma32(np.float32(len(x)), np.float32(c - np.float32(theta)), R)


def m1_uncentred(x, theta):
    """The form the shifted cases exist to fail: (float) sum x - n theta."""
    s = np.float32(np.sum(x.astype(np.float64)))
    return fma32(-np.float32(len(x)), np.float32(theta), s)


def m1_serial(x, theta):
    """The sweep's old sum: d = x - theta added to the even / odd
    accumulators in element order, then the two joined (float32)."""
    a = [np.float32(0.0), np.float32(0.0)]
    for e, v in enumerate(x):
        a[e & 1] = np.float32(a[e & 1] + np.float32(np.float32(v) - np.float32(theta)))
    return np.float32(a[0] + a[1])


def m1_f64(x, theta):
    return float(np.sum(x.astype(np.float64) - np.float64(theta)))


def bound_new(x, theta):
    """2^-23 (n |c - theta| + |R|): one rounding each (U = 2^-24) for
    c - theta (carried n times), the fma (|M1| <= n |c - theta| + |R|) and R."""
    if len(x) == 0:
        return 0.0
    c, R = run_consts(x)
    return 2.0 * U * (len(x) * abs(float(c) - float(np.float32(theta))) + abs(float(R)))


def bound_serial(x, theta):
    """The serial sum's share of _ragged.bounds: n terms, each d = x - theta
    with one rounding of its own: gamma(n + 1) sum |x - theta|."""
    return _gamma(len(x) + 1) * float(np.sum(np.abs(x.astype(np.float64) - np.float64(theta))))
