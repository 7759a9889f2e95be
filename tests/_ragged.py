"""Ragged and empty group runs (test helper): the hierarchical Normal model of
workloads.hierarchical over explicit per-group observation counts, its closed
form in numpy float64, and derived float32 error bounds.

workloads.hierarchical_data deals N observations evenly (runs of 100..143),
so a per-lane run there is always two software-pipelined rounds or more, a
remainder fixed by the shape and a masked tail of 0 or 1 element.  PATTERNS
names run lengths that reach the other regimes of every sweep routine
(lanes_fast.h lf_moments, lanes.h lr_moments, nuts_sliced.h nsl_moments,
mh_sliced.h msl_sumsq, sliced.h run_moments2, the tape's segment tiles) and
of the lane planner (plan_lanes.hip plan_lanes: rs slots, rep lane groups).

The model (mu, tau, sigma scalars; theta[G]):
    mu ~ N(0, 10), tau ~ HalfNormal(5), sigma ~ HalfNormal(5),
    theta_g ~ N(mu, tau), y_i ~ N(theta[group_i], sigma)
extra="scalar_mix" adds a scalar parameter z with z ~ N(mu, sigma) and a
second prior tau ~ Gamma(3, 1) (tests/test_gpu_sliced.py model_scalar_mix's
terms): scalar terms that are no own prior, so the lane kernels run their
generic scalar path (k_hmc_lr, not k_hmc_lf).

Parameter order (the flat layout): mu, tau, sigma, [z,] theta.
"""
import numpy as np

U = 2.0 ** -24          # float32 unit roundoff


def _cyc(n, f):
    return [int(f(i)) for i in range(n)]


# name -> observations per group.  With 33..64 groups on one slice the planner
# takes rs = 1 and rep = 1: a lane's run is one group, lmin4 = min(nonzero) // 4.
# N runs up to 2424 (rem3): the log p bound there, ~0.5, is still below one
# observation's contribution, log(2 pi) / 2 + log sigma = 0.92 at sigma = 1
# (asserted for every group of every pattern in test_ragged_reference.py).
PATTERNS = {
    "tiny": _cyc(48, lambda i: i % 8),              # lmin4 = 0, empty groups, 16 idle lanes
    "ones": [1] * 40,                               # lmin4 = 0, lmax = 1
    "exact32": [32] * 40,                           # no tail at all
    "round1": _cyc(48, lambda i: 16 + i % 8),       # lmin4 = 4: one round, clamped prefetch
    "rem0": _cyc(48, lambda i: 32 + i % 8),         # lmin4 = 8 .. 11: remainders 0 .. 3,
    "rem1": _cyc(48, lambda i: 37 + i % 8),         #   the 2-group unrolls at odd and even
    "rem2": _cyc(48, lambda i: 42 + i % 8),         #   counts, a tail of 0 .. 7
    "rem3": _cyc(48, lambda i: 47 + i % 8),
    "skew": [301, 64] + [1, 2, 3] * 14,             # lmin4 = 0, lmax = 301
    "slots2": _cyc(100, lambda i: (7 * i) % 41),    # rs = 2, slot 1 part-filled, zeros
    "slots4": _cyc(150, lambda i: (5 * i) % 23),    # rs = 3 -> 4, slot 2 part-filled
    "rep8": [0, 1, 5, 9, 100],                      # rep = 8, runs shorter than the group
    "rep16": [3, 16, 17],                           # rep = 16
    "rep2": _cyc(20, lambda i: (3 * i) % 11),       # rep = 2
    "few_long": [1, 700, 5],                        # the tape's virtual-segment split
}

# (register slots, lanes per private parameter) plan_lanes gives each pattern
# on one slice: rs = ceil(G / 64), 3 -> 4; rep = min(16, 64 / next power of two
# >= G) when rs = 1.  test_gpu_ragged.py asserts them (Program.lane_slots /
# lane_rep), and rep = 1 under MC_LANES_REP=1.  The tape's virtual-segment
# split of few_long has no query: that case rests on the run of 700 being
# longer than a segment tile, and is held only by its f64 check.
PLAN = {"tiny": (1, 1), "ones": (1, 1), "exact32": (1, 1), "round1": (1, 1), "rem0": (1, 1),
        "rem1": (1, 1), "rem2": (1, 1), "rem3": (1, 1), "skew": (1, 1), "slots2": (2, 1),
        "slots4": (4, 1), "rep8": (1, 8), "rep16": (1, 16), "rep2": (1, 2), "few_long": (1, 16)}

SEED = 0    # the data seed the mutation tests of test_ragged_reference.py were checked at


def ragged_data(lengths, order="sorted", seed=SEED):
    lengths = np.asarray(lengths, np.int64)
    G = len(lengths)
    rng = np.random.default_rng(seed)
    group = np.repeat(np.arange(G, dtype=np.int64), lengths)
    theta_true = rng.normal(1.0, 2.0, G)
    y = rng.normal(theta_true[group], 1.0).astype(np.float32)
    if order == "shuffled":
        perm = np.random.default_rng(seed + 1000).permutation(len(y))
        y, group = y[perm], group[perm]
    elif order != "sorted":
        raise ValueError(order)
    return {"y": y, "group": group.astype(np.int32), "G": G}


def ragged_hier(ns, lengths, order="sorted", extra=None, seed=SEED):
    """(log_prob, init, data) of the model over `lengths` observations per
    group, for W.ns_product() and W.ns_oracle() alike."""
    if extra not in (None, "scalar_mix"):
        raise ValueError(extra)
    data = ragged_data(lengths, order, seed)
    y, group, G = data["y"], data["group"], data["G"]

    def log_prob(params):
        mu, tau, sigma, theta = params["mu"], params["tau"], params["sigma"], params["theta"]
        lp = ns.Normal(0, 10).log_prob(mu)
        lp = lp + ns.HalfNormal(5).log_prob(tau)
        lp = lp + ns.HalfNormal(5).log_prob(sigma)
        if extra == "scalar_mix":
            lp = lp + ns.Gamma(3.0, 1.0).log_prob(tau)
            lp = lp + ns.Normal(mu, sigma).log_prob(params["z"])
        lp = lp + ns.sum(ns.Normal(mu, tau).log_prob(theta))
        lp = lp + ns.sum(ns.Normal(theta[group], sigma).log_prob(ns.array(y)))
        return lp

    sums = np.bincount(group, weights=y, minlength=G)
    counts = np.bincount(group, minlength=G)
    gm = np.where(counts > 0, sums / np.maximum(counts, 1), y.mean()).astype(np.float32)
    init = {"mu": np.float32(gm.mean()), "tau": np.float32(max(gm.std(), 0.5)),
            "sigma": np.float32(1.0)}
    if extra == "scalar_mix":
        init["z"] = np.float32(gm.mean() + 0.3)
    init["theta"] = gm
    return log_prob, init, data


def perturbed_points(init, n=4, seed=7):
    """[n, D] float32 points around `init` in layout order, scales kept
    positive (row 0 is `init` itself)."""
    rng = np.random.default_rng(seed)
    q0 = np.concatenate([np.atleast_1d(np.asarray(v, np.float32)).ravel() for v in init.values()])
    pts = np.tile(q0, (n, 1))
    names = list(init)
    for k in range(1, n):
        pts[k] += rng.normal(0.0, 0.3, q0.size).astype(np.float32)
        for nm in ("tau", "sigma"):
            j = names.index(nm)
            pts[k, j] = np.float32(q0[j] * np.exp(rng.normal(0.0, 0.3)))
    return pts.astype(np.float32)


# --------------------------------------------------------------------------
# the closed form, in any dtype
# --------------------------------------------------------------------------
HALF_LOG_2PI = 0.91893853320467274178
LOG2 = 0.69314718055994530942


def _split(q, G, extra):
    nsc = 4 if extra == "scalar_mix" else 3
    z = q[3] if nsc == 4 else None
    return q[0], q[1], q[2], z, q[nsc:nsc + G], nsc


def _evaluate(data, q, extra, dt, weights=None, mags=False):
    """log p and gradient in dtype `dt` (np.float64: the reference;
    np.float32: a float32 evaluation by per-group moment sums).  weights: a
    per-observation multiplicity (the mutation tests).  mags: return instead
    the sums of the sub-terms' magnitudes, per quantity (for bounds())."""
    y = data["y"].astype(dt)
    group, G = data["group"], data["G"]
    q = np.asarray(q).astype(dt)
    mu, tau, sigma, z, theta, nsc = _split(q, G, extra)
    w = np.ones(len(y), dt) if weights is None else np.asarray(weights).astype(dt)
    c0 = dt(HALF_LOG_2PI)
    half, one = dt(0.5), dt(1.0)
    A = np.abs if mags else (lambda x: x)

    order = np.argsort(group, kind="stable")
    counts = np.bincount(group, minlength=G)
    full = np.nonzero(counts)[0]
    starts = (np.cumsum(counts) - counts)[full]

    def seg(v):          # per-group sums, in the working dtype
        out = np.zeros(G, dt)
        if len(full):
            out[full] = np.add.reduceat(v[order], starts, dtype=dt)
        return out

    d = y - theta[group]
    iv = one / (sigma * sigma)
    cnt = seg(w)
    s1, s2 = seg(w * A(d)), seg(w * d * d)
    dth = theta - mu
    it = one / (tau * tau)
    n_obs = np.sum(cnt, dtype=dt)
    Gf = dt(G)
    if not mags:
        lp = -(half * np.sum(s2, dtype=dt)) * iv - n_obs * (np.log(sigma) + c0)
        lp = lp - (half * np.sum(dth * dth, dtype=dt)) * it - Gf * (np.log(tau) + c0)
        lp = lp - half * mu * mu / dt(100.0) - (dt(np.log(10.0)) + c0)
        lp = lp - half * tau * tau / dt(25.0) + (dt(LOG2) - c0 - dt(np.log(5.0)))
        lp = lp - half * sigma * sigma / dt(25.0) + (dt(LOG2) - c0 - dt(np.log(5.0)))
        g_theta = s1 * iv - dth * it
        g_mu = np.sum(dth, dtype=dt) * it - mu / dt(100.0)
        g_tau = np.sum(dth * dth, dtype=dt) * it / tau - Gf / tau - tau / dt(25.0)
        g_sigma = np.sum(s2, dtype=dt) * iv / sigma - n_obs / sigma - sigma / dt(25.0)
        g_z = None
        if extra == "scalar_mix":
            dz = z - mu
            lp = lp - half * dz * dz * iv - (np.log(sigma) + c0)
            lp = lp + (dt(2.0) * np.log(tau) - tau - dt(LOG2))      # Gamma(3, 1): -lgamma(3)
            g_z = -dz * iv
            g_mu = g_mu + dz * iv
            g_sigma = g_sigma + dz * dz * iv / sigma - one / sigma
            g_tau = g_tau + dt(2.0) / tau - one
    else:
        lp = (half * np.sum(s2, dtype=dt)) * iv + n_obs * (abs(np.log(sigma)) + c0)
        lp = lp + (half * np.sum(dth * dth, dtype=dt)) * it + Gf * (abs(np.log(tau)) + c0)
        lp = lp + half * mu * mu / dt(100.0) + (dt(np.log(10.0)) + c0)
        lp = lp + half * tau * tau / dt(25.0) + (dt(LOG2) + c0 + dt(np.log(5.0)))
        lp = lp + half * sigma * sigma / dt(25.0) + (dt(LOG2) + c0 + dt(np.log(5.0)))
        g_theta = s1 * iv + np.abs(dth) * it
        g_mu = np.sum(np.abs(dth), dtype=dt) * it + abs(mu) / dt(100.0)
        g_tau = np.sum(dth * dth, dtype=dt) * it / tau + Gf / tau + tau / dt(25.0)
        g_sigma = np.sum(s2, dtype=dt) * iv / sigma + n_obs / sigma + sigma / dt(25.0)
        g_z = None
        if extra == "scalar_mix":
            dz = abs(z - mu)
            lp = lp + half * dz * dz * iv + (abs(np.log(sigma)) + c0)
            lp = lp + (dt(2.0) * abs(np.log(tau)) + tau + dt(LOG2))
            g_z = dz * iv
            g_mu = g_mu + dz * iv
            g_sigma = g_sigma + dz * dz * iv / sigma + one / sigma
            g_tau = g_tau + dt(2.0) / tau + one
    g = np.empty(nsc + G, dt)
    g[0], g[1], g[2] = g_mu, g_tau, g_sigma
    if g_z is not None:
        g[3] = g_z
    g[nsc:] = g_theta
    return dt(lp), g


def ref_logp_grad(data, q, extra=None):
    """The closed-form log density and gradient in numpy float64 (no
    autograd), at the float32 point `q` ([D]) cast up."""
    return _evaluate(data, np.asarray(q, np.float32), extra, np.float64)


def f32_logp_grad(data, q, extra=None, weights=None):
    """The same formulas evaluated in float32 (per-group moment sums, as the
    lane kernels form them); `weights` counts each observation 0, 1 or 2
    times (the mutants of test_ragged_reference.py)."""
    return _evaluate(data, np.asarray(q, np.float32), extra, np.float32, weights=weights)


# roundings of one term beyond the additions of the sum it enters, in units of
# U = 2^-24 (a <= 1 ulp unit counts 2).  The longest chain any kernel has:
#   d = y - theta (or theta - mu)                         1   (2 where squared)
#   d * d                                                 1
#   1/s: v_rcp_f32, <= 1 ulp                              2
#   1/s^2 = (1/s)(1/s): 2 * 2 + 1                         5
#   the product with 1/s^2                                1
#   the weight                                            1
#   log s: v_log_f32 <= 1 ulp (2), ln 2 rounded (1), the product (1)      4
#   c0 = -log(2 pi)/2 rounded (1), c0 - log s (1), the count's product (1)  3
#   joining a term's parts (the subtraction)              1
C_GRAD_LOC = 1 + 5 + 1 + 1              # d / s^2 terms: theta_g, mu, z           = 8
C_GRAD_SCALE = 3 + 5 + 1 + 1 + 3 + 1    # (d^2 / s^2 - 1) / s terms: tau, sigma   = 14
C_LOGP = 3 + 5 + 1 + 1 + 1              # d^2 / (2 s^2) + log s + c0 terms        = 11
                                        # (the log s chain, 4 + 3 + 1 + 1 = 9, is shorter)


def _gamma(k):
    return k * U / (1.0 - k * U)


def bounds(data, q, extra=None):
    """Absolute error bounds (lp_bound, g_bound[D]) of a float32 evaluation at
    `q`, derived (not measured): a float32 sum of n terms in any order, each
    term carrying c roundings of its own, is within
        gamma(n + c) * sum_i |term_i|,   gamma(k) = k U / (1 - k U),
    of the exact sum (Higham, Accuracy and Stability, eq. 4.4 with the
    terms' own (1 + delta)^c), where a term that is itself a difference
    (z^2 / s - 1 / s, c0 - log s ...) counts by the magnitudes of its parts.
    c per quantity: C_GRAD_LOC, C_GRAD_SCALE, C_LOGP above, each rounding
    written out there.  n: for theta_g the run length plus 1 (its prior);
    for mu, tau, sigma, z and log p every term of the model: N + G plus the
    scalar terms."""
    q = np.asarray(q, np.float32)
    G = data["G"]
    N = len(data["y"])
    nsc = 4 if extra == "scalar_mix" else 3
    n_scalar = 5 if extra == "scalar_mix" else 3
    n_all = N + G + n_scalar
    mlp, mg = _evaluate(data, q, extra, np.float64, mags=True)
    counts = np.bincount(data["group"], minlength=G)
    gb = np.empty(nsc + G)
    gb[0] = _gamma(n_all + C_GRAD_LOC) * mg[0]
    gb[1] = _gamma(n_all + C_GRAD_SCALE) * mg[1]
    gb[2] = _gamma(n_all + C_GRAD_SCALE) * mg[2]
    if nsc == 4:
        gb[3] = _gamma(n_all + C_GRAD_LOC) * mg[3]
    gb[nsc:] = np.array([_gamma(int(c) + 1 + C_GRAD_LOC) for c in counts]) * mg[nsc:]
    return _gamma(n_all + C_LOGP) * float(mlp), gb


def check_state(q, g, logp, data, extra=None, what=""):
    """Every chain's gradient g[c] and log density logp[c] at q[c] against the
    float64 reference, within bounds() (g=None: log p alone, a sampler that
    keeps no gradient).  Prints the worst ratio error / bound before it
    asserts."""
    q = np.atleast_2d(np.asarray(q, np.float32))
    no_g = g is None
    g = np.zeros(q.shape) if no_g else np.atleast_2d(np.asarray(g))
    assert np.all(np.isfinite(g)) and np.all(np.isfinite(logp)), f"{what}: not finite"
    logp = np.atleast_1d(np.asarray(logp))
    assert q.shape == g.shape and logp.shape == (q.shape[0],), (q.shape, g.shape, logp.shape)
    worst_g = worst_lp = 0.0
    fails = []
    for c in range(q.shape[0]):
        rl, rg = ref_logp_grad(data, q[c], extra)
        bl, bg = bounds(data, q[c], extra)
        eg = np.zeros_like(rg) if no_g else np.abs(g[c].astype(np.float64) - rg)
        el = abs(float(logp[c]) - float(rl))
        worst_g = max(worst_g, float(np.max(eg / np.maximum(bg, 1e-300))))
        worst_lp = max(worst_lp, el / bl)
        bad = np.nonzero(~(eg <= bg))[0]
        if bad.size:
            j = int(bad[np.argmax(eg[bad])])
            fails.append(f"chain {c}: g[{j}] = {g[c][j]!r}, f64 {rg[j]!r}, |err| {eg[j]:.3e} > "
                         f"bound {bg[j]:.3e} ({bad.size} components out)")
        if not el <= bl:
            fails.append(f"chain {c}: log p = {logp[c]!r}, f64 {rl!r}, |err| {el:.3e} > "
                         f"bound {bl:.3e}")
    print(f"{what}: worst |err| / bound: gradient {worst_g:.3f}, log p {worst_lp:.3f}")
    assert not fails, f"{what}: " + "; ".join(fails[:6])
