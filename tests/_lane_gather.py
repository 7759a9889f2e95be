"""Models and helpers of the gathered-parameter lane tests
(tests/test_expr_lane_gather_host.py, tests/test_lane_gather_reference.py on
the CPU, tests/test_gpu_expr_lane_gather.py on the GPU)."""
import ctypes

import numpy as np

import workloads as W

# group sizes of the ragged varying-slopes data set, cycled over the groups:
# every run-length class of the lane sweep (empty, below one 4-element trip,
# a ragged tail, several trips)
SIZES = (0, 1, 2, 3, 5, 8, 13, 34, 55, 89, 144, 3)


def ragged_slopes_data(G, seed=11):
    """(x, y, group): group g holds SIZES[g % 12] observations, the index
    shuffled (unsorted), y = alpha_g + beta_g x + noise."""
    rng = np.random.default_rng(seed)
    sizes = np.array([SIZES[g % len(SIZES)] for g in range(G)])
    group = np.repeat(np.arange(G), sizes)
    rng.shuffle(group)
    n = group.size
    alpha = rng.normal(1.0, 1.0, G)
    beta = rng.normal(-0.5, 0.7, G)
    x = rng.normal(0.0, 1.0, n).astype(np.float32)
    y = (alpha[group] + beta[group] * x + rng.normal(0.0, 0.5, n)).astype(np.float32)
    return x, y, group.astype(np.int32)


def ragged_slopes_truth(G, seed=11):
    """The generating (alpha, beta) of ragged_slopes_data: a start inside the
    posterior's bulk (from a far start every early proposal is rejected)."""
    rng = np.random.default_rng(seed)
    sizes = np.array([SIZES[g % len(SIZES)] for g in range(G)])
    rng.shuffle(np.repeat(np.arange(G), sizes))
    alpha = rng.normal(1.0, 1.0, G)
    beta = rng.normal(-0.5, 0.7, G)
    return alpha.astype(np.float32), beta.astype(np.float32)


def ragged_slopes(ns, G, seed=11):
    """workloads.varying_slopes over the ragged data set, started at the
    generating coefficients."""
    x, y, group = ragged_slopes_data(G, seed)
    alpha0, beta0 = ragged_slopes_truth(G, seed)

    def log_prob(params):
        mu_a, mu_b, sigma = params["mu_a"], params["mu_b"], params["sigma"]
        alpha, beta = params["alpha"], params["beta"]
        lp = ns.Normal(0, 5).log_prob(mu_a) + ns.Normal(0, 5).log_prob(mu_b)
        lp = lp + ns.HalfNormal(2).log_prob(sigma)
        lp = lp + ns.sum(ns.Normal(mu_a, 2.0).log_prob(alpha))
        lp = lp + ns.sum(ns.Normal(mu_b, 2.0).log_prob(beta))
        mean = alpha[group] + beta[group] * ns.array(x)
        return lp + ns.sum(ns.Normal(mean, sigma).log_prob(ns.array(y)))

    return log_prob, {"mu_a": np.float32(1.0), "mu_b": np.float32(-0.5),
                      "sigma": np.float32(0.5), "alpha": alpha0, "beta": beta0}


def poly_slopes(ns, G, N, nvec=3, extra=0, seed=12):
    """y ~ N(sum_k c_k[g] x^k, sigma) over nvec gathered coefficient vectors
    (nvec = 3: alpha[g] + beta[g] x + gamma[g] x^2), c_k ~ N(0, 2); `extra`
    more vectors d_m gathered the same way enter the mean as 0.1 d_m[g]."""
    rng = np.random.default_rng(seed)
    group = rng.integers(0, G, N).astype(np.int32)
    coef = rng.normal(0.3, 0.6, (nvec, G))
    x = rng.normal(0.0, 0.8, N).astype(np.float32)
    mean = sum(coef[k][group] * x.astype(np.float64) ** k for k in range(nvec))
    y = (mean + rng.normal(0.0, 0.5, N)).astype(np.float32)
    names = ["c%d" % k for k in range(nvec)] + ["d%d" % m for m in range(extra)]

    def log_prob(params):
        sigma = params["sigma"]
        lp = ns.HalfNormal(2).log_prob(sigma)
        for nm in names:
            lp = lp + ns.sum(ns.Normal(0.0, 2.0).log_prob(params[nm]))
        xa = ns.array(x)
        m = params["c0"][group]
        xp = xa
        for k in range(1, nvec):
            m = m + params["c%d" % k][group] * xp
            xp = xp * xa
        for e in range(extra):
            m = m + 0.1 * params["d%d" % e][group]
        return lp + ns.sum(ns.Normal(m, sigma).log_prob(ns.array(y)))

    init = {"sigma": np.float32(0.5)}     # (started at the generating coefficients)
    for k, nm in enumerate(names):
        init[nm] = coef[k].astype(np.float32) if k < nvec else np.full(G, 0.1, np.float32)
    return log_prob, init


def weighted_start(G, n):
    """workloads.weighted_indexed's init with alpha at the groups' weighted
    mean residuals (a start inside the posterior's bulk)."""
    group, z, w, y = W.weighted_indexed_data(G, n)
    _, init = W.weighted_indexed(W.ns_oracle(), G, n)
    r = y - 0.5 * z[group]
    num = np.bincount(group, weights=w * r, minlength=G)
    den = np.bincount(group, weights=w, minlength=G)
    start = dict(init)
    start["alpha"] = (num / np.maximum(den, 1e-9)).astype(np.float32)
    return start


def lane_source(h):
    from mlx_mcmc_amd import _lib

    lib = _lib.load()
    n = lib.mc_debug_expr_jit_lane_source(h, None, 0)
    buf = ctypes.create_string_buffer(n + 1)
    lib.mc_debug_expr_jit_lane_source(h, buf, n + 1)
    return buf.value.decode()


# plan invariance: programs without grouped expression terms (name -> builder,
# slices); their lane source, register slots and replication are recorded in
# tests/golden/lane_plan_invariance.json from the build before grouped terms
INVARIANT = {
    "hier_small": (lambda ns: W.hierarchical(ns, *W.SHAPES["small"]), 1),
    "varying_intercept": (lambda ns: W.varying_intercept(ns, 200, 100_000), 16),
    "logistic": (lambda ns: W.logistic_regression(ns, 20_000), 8),
}


def observe_plan(name):
    """(lane source, lane_slots, lane_rep) of INVARIANT[name]'s host plan."""
    from _jit_models import host_program
    from mlx_mcmc_amd import _lib

    lib = _lib.load()
    build, S = INVARIANT[name]
    lp, init = build(W.ns_product())
    h = host_program(lp, init)
    try:
        rc = lib.mc_debug_lane_plan_host(h, S)
        assert rc == 0, (lib.mc_last_error() or b"").decode()
        return {"source": lane_source(h), "lane_slots": int(lib.mc_program_lane_slots(h)),
                "lane_rep": int(lib.mc_program_lane_rep(h))}
    finally:
        lib.mc_program_destroy(h)


# ---- the float64 reference of a Normal likelihood with a linear mean ---------
HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)
U = 2.0 ** -24
# Roundings one element's term carries before it enters a sum, in units of U
# (a <= 1 ulp operation counts 2): the mean, a product and a sum per gathered
# vector (<= 2 * 4), y - m (1), the division by s (2), its square and the half
# (2), log s (hardware log <= 1 ulp, the ln 2 product: 4; a log-affine scale's
# exp: 4 more), joining the parts (2), the weight (1), and for a cotangent the
# second division by s (2), the feature's product (1): 27 at most.
C_TERM = 27


def _gamma(k):
    return k * U / (1.0 - k * U)


def layout_of(lp, init):
    """name -> offset of the traced parameter layout."""
    from mlx_mcmc_amd import _trace

    lay = _trace.trace(lp, init).layout
    return {n: int(o) for n, o in zip(lay.names, lay.offsets)}, int(lay.size)


def slopes_spec(G, off, D, seed=11):
    x, y, group = ragged_slopes_data(G, seed)
    return dict(D=D, G=G, y=y, w=np.ones(len(y)), group=group,
                vec=[(off["alpha"], np.ones(len(y))), (off["beta"], x)], sh_mean=[],
                scale=("param", off["sigma"]),
                priors=[("normal", off["mu_a"], 1, ("c", 0.0), 5.0),
                        ("normal", off["mu_b"], 1, ("c", 0.0), 5.0),
                        ("halfnormal", off["sigma"], 1, None, 2.0),
                        ("normal", off["alpha"], G, ("p", off["mu_a"]), 2.0),
                        ("normal", off["beta"], G, ("p", off["mu_b"]), 2.0)])


def poly_spec(G, N, off, D, nvec=3, seed=12):
    rng = np.random.default_rng(seed)
    group = rng.integers(0, G, N).astype(np.int32)
    coef = rng.normal(0.3, 0.6, (nvec, G))
    x = rng.normal(0.0, 0.8, N).astype(np.float32)
    mean = sum(coef[k][group] * x.astype(np.float64) ** k for k in range(nvec))
    y = (mean + rng.normal(0.0, 0.5, N)).astype(np.float32)
    feats, xp = [np.ones(N)], np.ones(N, np.float32)
    for k in range(1, nvec):
        xp = (xp * x).astype(np.float32) if k > 1 else x      # the model's f32 powers
        feats.append(xp)
    return dict(D=D, G=G, y=y, w=np.ones(N), group=group,
                vec=[(off["c%d" % k], feats[k]) for k in range(nvec)], sh_mean=[],
                scale=("param", off["sigma"]),
                priors=[("halfnormal", off["sigma"], 1, None, 2.0)] +
                       [("normal", off["c%d" % k], G, ("c", 0.0), 2.0) for k in range(nvec)])


def weighted_spec(G, n, off, D):
    group, z, w, y = W.weighted_indexed_data(G, n)
    zg = z[group]
    return dict(D=D, G=G, y=y, w=w, group=group.astype(np.int32),
                vec=[(off["alpha"], np.ones(n))], sh_mean=[(off["beta"], zg)],
                scale=("logaff", off["log_sigma"], off["c"], zg),
                priors=[("normal", off["alpha"], G, ("c", 0.0), 2.0),
                        ("normal", off["beta"], 1, ("c", 0.0), 2.0),
                        ("normal", off["log_sigma"], 1, ("c", 0.0), 1.0),
                        ("normal", off["c"], 1, ("c", 0.0), 1.0)])


def glm_eval(spec, q, weights=None, mags=False):
    """(log p, gradient[D]) of the model in float64 at the float32 point q,
    closed form (tests/test_lane_gather_reference.py checks it against float64
    autograd).  weights: each observation counted 0, 1 or 2 times.  mags: the
    sums of the addends' magnitudes instead (the error bounds' scale)."""
    q = np.asarray(q, np.float32).astype(np.float64)
    A = np.abs if mags else (lambda v: v)
    sgn = 1.0 if mags else -1.0
    y, g, G = spec["y"].astype(np.float64), spec["group"], spec["G"]
    Wt = spec["w"].astype(np.float64) * (1.0 if weights is None else np.asarray(weights, np.float64))
    m = np.zeros(len(y))
    for off, f in spec["vec"]:
        m = m + q[off + g] * f.astype(np.float64)
    for idx, f in spec["sh_mean"]:
        m = m + q[idx] * f.astype(np.float64)
    if spec["scale"][0] == "param":
        s = np.full(len(y), q[spec["scale"][1]])
    else:
        _, ils, ic, zf = spec["scale"]
        s = np.exp(q[ils] + q[ic] * zf.astype(np.float64))
    z = (y - m) / s
    lp = np.sum(Wt * (sgn * 0.5 * z * z + sgn * A(np.log(s)) + sgn * HALF_LOG_2PI))
    dm = Wt * A(z) / s
    ds = Wt * (z * z + (1.0 if mags else -1.0)) / s
    grad = np.zeros(spec["D"])
    for off, f in spec["vec"]:
        grad[off:off + G] += np.bincount(g, weights=dm * A(f.astype(np.float64)), minlength=G)
    for idx, f in spec["sh_mean"]:
        grad[idx] += np.sum(dm * A(f.astype(np.float64)))
    if spec["scale"][0] == "param":
        grad[spec["scale"][1]] += np.sum(ds)
    else:
        grad[ils] += np.sum(ds * s)
        grad[ic] += np.sum(ds * s * A(zf.astype(np.float64)))
    for kind, off, n, loc, sc in spec["priors"]:
        x = q[off:off + n]
        if kind == "normal":
            mu = loc[1] if loc[0] == "c" else q[loc[1]]
            d = x - mu
            lp += np.sum(sgn * 0.5 * (d / sc) ** 2 + sgn * abs(np.log(sc)) + sgn * HALF_LOG_2PI) \
                if mags else np.sum(-0.5 * (d / sc) ** 2 - np.log(sc) - HALF_LOG_2PI)
            grad[off:off + n] += sgn * A(d) / sc ** 2 if mags else -d / sc ** 2
            if loc[0] == "p":
                grad[loc[1]] += np.sum(A(d)) / sc ** 2
        else:
            lp += np.sum(0.5 * (x / sc) ** 2) + n * (np.log(2.0) + abs(np.log(sc)) + HALF_LOG_2PI) \
                if mags else np.sum(-0.5 * (x / sc) ** 2) + n * (np.log(2.0) - np.log(sc) - HALF_LOG_2PI)
            grad[off:off + n] += A(x) / sc ** 2 if mags else -x / sc ** 2
    return float(lp), grad


def glm_bounds(spec, q):
    """Absolute error bounds (log p, gradient[D]) of a float32 evaluation on
    the lane layout, derived: a float32 sum of depth k whose terms carry c
    roundings of their own is within gamma(k + c) * sum |term| of the exact
    sum (Higham, Accuracy and Stability, eq. 4.4), gamma(k) = k U / (1 - k U).
    A private parameter's gradient is summed inside its lane: its group's run
    and its prior, depth count_g + 1.  Log p and a broadcast parameter's
    gradient are summed per lane over its runs (a lane's 4 register slots hold
    at most 4 // B bundles of B gathered vectors, each at most the longest
    group), then over the wave (a 6-level tree), the slices (a 4-level tree)
    and the model's other terms (at most 8): depth (4 // B) max_g count_g + 18."""
    mlp, mg = glm_eval(spec, q, mags=True)
    counts = np.bincount(spec["group"], minlength=spec["G"])
    ex_lp, ex_g = _residual_bounds(spec, q)
    deep = (4 // len(spec["vec"])) * int(counts.max()) + 18
    k = np.full(spec["D"], float(deep))
    for off, _ in spec["vec"]:
        k[off:off + spec["G"]] = counts + 1
    return (_gamma(deep + C_TERM) * mlp + ex_lp,
            (k + C_TERM) * U / (1.0 - (k + C_TERM) * U) * mg + ex_g)


def _residual_bounds(spec, q):
    """The part of the bounds the terms' own magnitudes do not carry: the
    residual y - m cancels, so the roundings of the mean m = sum_v q_v f_v (a
    product and a partial sum per addend: 2 per addend, relative to sum_v |q_v
    f_v|) reach the term with the weight of its derivative in m, to first
    order: |z| / s into log p, 1 / s^2 times the feature into a mean
    parameter's gradient, 2 |z| / s^2 into the scale's."""
    q = np.asarray(q, np.float32).astype(np.float64)
    y, g, G = spec["y"].astype(np.float64), spec["group"], spec["G"]
    Wt = spec["w"].astype(np.float64)
    m, am = np.zeros(len(y)), np.zeros(len(y))
    for off, f in spec["vec"]:
        m, am = m + q[off + g] * f, am + np.abs(q[off + g] * f)
    for idx, f in spec["sh_mean"]:
        m, am = m + q[idx] * f, am + np.abs(q[idx] * f)
    dm = 2 * (len(spec["vec"]) + len(spec["sh_mean"])) * U * am
    if spec["scale"][0] == "param":
        s = np.full(len(y), q[spec["scale"][1]])
    else:
        _, ils, ic, zf = spec["scale"]
        s = np.exp(q[ils] + q[ic] * zf.astype(np.float64))
    z = np.abs(y - m) / s
    ex = np.zeros(spec["D"])
    for off, f in spec["vec"]:
        ex[off:off + G] += np.bincount(g, weights=Wt * dm * np.abs(f) / s ** 2, minlength=G)
    for idx, f in spec["sh_mean"]:
        ex[idx] += np.sum(Wt * dm * np.abs(f) / s ** 2)
    if spec["scale"][0] == "param":
        ex[spec["scale"][1]] += np.sum(Wt * 2 * z * dm / s ** 2)
    else:
        ex[ils] += np.sum(Wt * 2 * z * dm / s)
        ex[ic] += np.sum(Wt * 2 * z * dm / s * np.abs(zf))
    return float(np.sum(Wt * z * dm / s)), ex


def check_glm_state(spec, q, g, logp, what=""):
    """Every chain's gradient and log p at its own position q[c] against the
    float64 closed form within glm_bounds; prints the worst error / bound."""
    q = np.atleast_2d(np.asarray(q, np.float32))
    no_g = g is None          # (a sampler that keeps no gradient: log p alone)
    g = np.atleast_2d(np.zeros(q.shape) if no_g else np.asarray(g))
    logp = np.atleast_1d(np.asarray(logp))
    assert np.all(np.isfinite(g)) and np.all(np.isfinite(logp)), f"{what}: not finite"
    worst_g = worst_lp = 0.0
    fails = []
    for c in range(q.shape[0]):
        rl, rg = glm_eval(spec, q[c])
        bl, bg = glm_bounds(spec, q[c])
        eg = np.zeros_like(rg) if no_g else np.abs(g[c].astype(np.float64) - rg)
        el = abs(float(logp[c]) - rl)
        worst_g = max(worst_g, float(np.max(eg / np.maximum(bg, 1e-300))))
        worst_lp = max(worst_lp, el / bl)
        bad = np.nonzero(~(eg <= bg))[0]
        if bad.size:
            j = int(bad[np.argmax(eg[bad] / np.maximum(bg[bad], 1e-300))])
            fails.append(f"chain {c}: g[{j}] = {g[c][j]!r}, f64 {rg[j]!r}, |err| {eg[j]:.3e} > "
                         f"bound {bg[j]:.3e} ({bad.size} components out)")
        if not el <= bl:
            fails.append(f"chain {c}: log p = {logp[c]!r}, f64 {rl!r}, |err| {el:.3e} > {bl:.3e}")
    print(f"{what}: worst |err| / bound: gradient {worst_g:.3f}, log p {worst_lp:.3f}")
    assert not fails, f"{what}: " + "; ".join(fails[:6])
