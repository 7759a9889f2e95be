"""k_hmc_lf's second moment from per-run constants (test helper).

lanes_fast.h lf_moments sums nothing per step: about the run's centre
c = (float) mean(x) (tests/_lf_first_moment.py run_consts) the planner keeps
    R = (float) sum_e (x_e - c),    Q = (float) sum_e (x_e - c)^2
(sums in double, in element order) and, with d = c - theta in float32,
    M2 = sum_e (x_e - theta)^2 = Q + 2 d R + n d^2 = fma(fma(n, d, 2 R), d, Q).
The identity is exact about any centre, so c's own rounding is no error.

Bound (U = 2^-24, one rounding each):
  d        relative U: n d^2 moves by 2 U n d^2, 2 d R by U 2 |d R|;
  inner    fma(n, d, 2 R), then times d: U (n d^2 + 2 |R d|);
  outer    U |M2| <= U (Q + n d^2 + 2 |R d|);
  Q        U Q;           R: U 2 |R d|;
together at most U (2 Q + 4 n d^2 + 4 * 2 |R d|) <= 2^-22 (Q + n d^2 + 2 |R d|).
"""
import numpy as np

from _lf_first_moment import fma32, run_consts

OFFSETS = (-1.5, -0.5, 0.5, 1.5)   # theta - mean(x)


def q_const(x, c):
    """Q of a run about its centre c, in float64 (the planner rounds it once)."""
    t = np.float64(0.0)
    for v in x:
        d = np.float64(v) - np.float64(c)
        t = t + d * d
    return t


def m2_new(x, theta, r_factor=2.0):
    """fma(fma(n, d, 2 R), d, Q) in float32 (r_factor: the mutants' 0 / -2)."""
    if len(x) == 0:
        return np.float32(0.0)
    c, R = run_consts(x)
    Q = np.float32(q_const(x, c))
    d = np.float32(c - np.float32(theta))
    inner = fma32(np.float32(len(x)), d, np.float32(np.float32(r_factor) * R))
    return fma32(inner, d, Q)


def m2_f64(x, theta):
    return float(np.sum((x.astype(np.float64) - np.float64(np.float32(theta))) ** 2))


def bound_m2(x, theta):
    if len(x) == 0:
        return 0.0
    c, R = run_consts(x)
    d = float(c) - float(np.float32(theta))
    return 2.0 ** -22 * (float(q_const(x, c)) + len(x) * d * d + 2.0 * abs(float(R) * d))
