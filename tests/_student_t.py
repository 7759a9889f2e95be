"""The Student-t family (StudentT, Cauchy, HalfStudentT, HalfCauchy) for its
tests: tests/test_student_t_host.py (no device) and
tests/test_gpu_student_t.py.

Nodes.  ``fwd64`` / ``vjp64`` / ``fwd32`` / ``vjp32`` state MC_EX_STUDENT_T_LP
and MC_EX_HALF_STUDENT_T_LP of include/mcmc355.h once — value and VJP
(cotangent 1) as NumPy code that keeps the dtype of its inputs and performs
eval.h's operations in eval.h's order (the pattern of tests/_expr_ops.py and
tests/_discrete.py): on float64 copies of the float32 inputs it is the
reference, on the float32 inputs the one-rounding-per-operation evaluation that
decides the class of an edge result.  nu is the float32 node constant in both.

    d = v - m (half: v);  z = d / s;  q = z z;  w = q / nu;  h = (nu + 1) / 2
    lp = (-log s) - h log1p(w)
    r = z / (nu + q);  g = (nu + 1) r;  t = g / s
    dv = -t,  dm = t,  ds = (g z - 1) / s;   q = inf: the cotangents are 0
    half form: -inf and no cotangent unless v >= 0

Ulp gates.  Derived from eval.h's documented figures, never from the new
nodes: ex_div within K_DIV = 1 ulp and ex_log within K_LOG = 2 ulp
(_expr_ops.DOCUMENTED_ULP); ex_log1p has no documented bound and its
_expr_ops.MEASURED_ULP entry, measured before these nodes existed, stands in:
K_L1P = 2.828 ulp.  An error of K ulp of x is at most K 2^-23 |x| relative, and
a relative error of K 2^-23 of y is at most 2 K ulp of y, so the relative
errors below are summed in units of 2^-23 and the gate is twice the sum.

  z = d / s       d rounds once (0.5), the quotient K_DIV:       K_Z = 1.5
  w = z z / nu    2 K_Z, the square rounds (0.5), the quotient:  K_W = 4.5
  B = h log1p(w)  d log1p(w) = dw / (1 + w) and log1p(w) >= w / (1 + w): a
                  relative error of w is at most the same relative error of
                  log1p(w); log1p adds K_L1P; h = (nu + 1) / 2 rounds once
                  (0.5) and the product once (0.5):              K_B = 8.328
  A = -log s      K_LOG = 2 of |log s|
  lp = A - B      rounds once (0.5 of |lp| <= |A| + |B|):
                  K_VAL = max(K_B, K_LOG) + 0.5 = 8.828 of |log s| + h log1p(w)
                  FWD_GATE = ceil(2 K_VAL) = 18 ulp of that magnitude
  r = z / (nu + q)   q carries 2 K_Z + 0.5 = 3.5, weighted by q / (nu + q) <= 1;
                  the sum rounds (0.5): 4; with z (K_Z) and the quotient:
                                                                 K_R = 6.5
  g = (nu + 1) r  nu + 1 rounds (0.5), the product (0.5):        K_G = 7.5
  t = g / s       K_G + K_DIV = 8.5: VJP_GATE (value, loc) = 17 ulp of |t|
  ds              g z: K_G + K_Z + 0.5 = 9.5 of |g z|; the difference with 1
                  rounds (0.5 of |g z| + 1); the quotient K_DIV: 11,
                  VJP_GATE (scale) = 22 ulp of (|g z| + 1) / s

  (recorded, not used: over the bulk sweep an MI355X measures at most 3.31 ulp
  for the value, 3.25 for the value / loc VJP and 3.05 for the scale VJP)

Samplers.  ``host_draws`` applies the library's scalar definition
(mc_predictive_draw_student_t) to arrays.

Models.  N = 67 observations (no multiple of 64): a robust regression
``StudentT(4, a + b x, exp(log_s))`` with Normal priors, and a hierarchy
``theta[g] ~ Normal(mu, tau)``, ``tau = exp(log_tau) ~ HalfCauchy(1)`` (with the
log-Jacobian), ``y ~ StudentT(3, theta[g], 1)`` over 8 groups — each for the
product namespace and as a float64 torch restatement
(torch.distributions.StudentT) for oracle.samplers.EagerModel; the one-parameter
location model of the exact-posterior test; the likelihoods alone with seeded
draws (C = 3, S = 37) for WAIC / LOO / replicates.  The likelihoods alone take
the scale as a parameter itself (not through exp): a replicate is compared bit
for bit with the host definition, which needs the device's operand bits, and
ex_exp is within 2 ulp of NumPy's, not equal to it.
"""
from __future__ import annotations

import ctypes
import math
from types import SimpleNamespace

import numpy as np

import _expr_ops as X
from mlx_mcmc_amd import _lib

F32 = np.float32
OP = {"student_t": _lib.MC_EX_STUDENT_T_LP, "half_student_t": _lib.MC_EX_HALF_STUDENT_T_LP}
NODES = tuple(OP)
NUS = (1.0, 4.0, 30.0)
N_VEC = X.N_VEC
N_OBS = 67

K_DIV = X.DOCUMENTED_ULP["div"]
K_LOG = X.DOCUMENTED_ULP["log"]
K_L1P = X.MEASURED_ULP["log1p"]["fwd"]
K_Z = 0.5 + K_DIV
K_W = 2 * K_Z + 0.5 + K_DIV
K_B = K_W + K_L1P + 0.5 + 0.5
K_VAL = max(K_B, K_LOG) + 0.5
K_R = K_Z + (2 * K_Z + 0.5 + 0.5) + K_DIV
K_G = K_R + 0.5 + 0.5
FWD_GATE = math.ceil(2 * K_VAL)
VJP_GATE = {"v": math.ceil(2 * (K_G + K_DIV)), "m": math.ceil(2 * (K_G + K_DIV)),
            "s": math.ceil(2 * (K_G + K_Z + 0.5 + 0.5 + K_DIV))}


# ---- the nodes: eval.h's operations in eval.h's order ----------------------------
def _c(x, c):
    return x.dtype.type(c)


def is_half(name):
    return name == "half_student_t"


def diff_names(name):
    return ("v", "s") if is_half(name) else ("v", "m", "s")


def _fwd(name, nu, v, m, s):
    nu = _c(v, F32(nu))
    d = v if is_half(name) else v - m
    z = X._div(d, s)
    q = z * z
    w = X._div(q, nu)
    h = _c(v, 0.5) * (nu + _c(v, 1))
    lp = (-np.log(s)) - h * np.log1p(w)
    if is_half(name):
        lp = np.where(v >= 0, lp, _c(v, -np.inf))
    return lp.astype(v.dtype)


def _vjp(name, nu, v, m, s):
    """{"v": dv, "m": dm, "s": ds} (no "m" for the half form)."""
    nu = _c(v, F32(nu))
    d = v if is_half(name) else v - m
    z = X._div(d, s)
    q = z * z
    r = X._div(z, nu + q)
    g = (nu + _c(v, 1)) * r
    far = q == np.inf
    zero = np.zeros_like(v)
    t = np.where(far, zero, X._div(g, s)).astype(v.dtype)
    u = np.where(far, zero, X._div(g * z - _c(v, 1), s)).astype(v.dtype)
    out = {"v": -t, "s": u}
    if is_half(name):
        ok = v >= 0
        return {k: np.where(ok, a, zero).astype(v.dtype) for k, a in out.items()}
    out["m"] = t
    return out


def _args(dt, v, m, s):
    v, m, s = np.broadcast_arrays(np.asarray(v, F32), np.asarray(0 if m is None else m, F32),
                                  np.asarray(s, F32))
    return v.astype(dt), m.astype(dt), s.astype(dt)


@X._quiet
def fwd64(name, nu, v, m, s):
    return _fwd(name, nu, *_args(np.float64, v, m, s))


@X._quiet
def vjp64(name, nu, v, m, s):
    return _vjp(name, nu, *_args(np.float64, v, m, s))


@X._quiet
def fwd32(name, nu, v, m, s):
    return _fwd(name, nu, *_args(F32, v, m, s))


@X._quiet
def vjp32(name, nu, v, m, s):
    return _vjp(name, nu, *_args(F32, v, m, s))


@X._quiet
def units(name, nu, v, m, s):
    """(value unit, {argument: VJP unit}): the float32 spacing of the summed
    magnitudes of the formula's terms (never less than the result's)."""
    v, m, s = _args(np.float64, v, m, s)
    nu = float(F32(nu))
    d = v if is_half(name) else v - m
    z = d / s
    q = z * z
    f = np.abs(fwd64(name, nu, v, m, s))
    g = vjp64(name, nu, v, m, s)
    sf = np.abs(np.log(s)) + 0.5 * (nu + 1.0) * np.log1p(q / nu)
    gz = (nu + 1.0) * q / (nu + q)
    ss = (np.abs(gz) + 1.0) / np.abs(s)
    sf = np.where(np.isfinite(sf), np.maximum(sf, f), f)
    ss = np.where(np.isfinite(ss), np.maximum(ss, np.abs(g["s"])), np.abs(g["s"]))
    out = {k: X.ulp(np.abs(a)) for k, a in g.items()}
    out["s"] = X.ulp(ss)
    return X.ulp(sf), out


def norm64(nu, half):
    """The normaliser of the float32 nu in float64."""
    nu = float(F32(nu))
    c = math.lgamma(0.5 * (nu + 1.0)) - math.lgamma(0.5 * nu) - 0.5 * math.log(nu * math.pi)
    return c + (math.log(2.0) if half else 0.0)


# ---- inputs of the per-node GPU tests ---------------------------------------------
def bulk(name, nu, n=X.P_BULK):
    """P_BULK points: v and m of both signs, log-uniform magnitudes in
    [1e-3, 30] (half form: v >= 0), s log-uniform in [1e-2, 30]."""
    rng = np.random.default_rng(2000 + 10 * OP[name] + int(nu))
    v = X._logu(rng, n, 1e-3, 30.0, not is_half(name))
    m = X._logu(rng, n, 1e-3, 30.0, True)
    s = X._logu(rng, n, 1e-2, 30.0)
    return v, m, s


def edges(name):
    """The edge points (v, m, s): v = +-inf, NaN; |z| beyond 2e19 (q overflows);
    s in {0, -1, inf, NaN}, s = 0 beside d = 0; the half form's v in {-0, -1,
    NaN}; and benign neighbours.  No divisor between 2^126 and FLT_MAX or
    subnormal (outside ex_div's range: |z| in [2^63, 1.8e19] is left out)."""
    inf, nan = np.inf, np.nan
    pts = [(0.7, -0.4, 1.3), (0.0, 0.0, 1.0), (inf, 0.2, 1.5), (-inf, 0.2, 1.5), (nan, 0.2, 1.5),
           (3e19, 0.0, 1.0), (-3e19, 0.0, 1.0), (1e25, 0.5, 1e3), (2.5, 0.5, 1e-20),
           (0.3, inf, 2.0), (0.3, -inf, 2.0), (0.3, nan, 2.0), (inf, inf, 1.0),
           (0.7, -0.4, 0.0), (0.7, 0.7, 0.0), (0.7, -0.4, -1.0), (0.7, -0.4, inf),
           (0.7, -0.4, nan), (inf, 0.0, inf), (1e30, 0.0, 1e30)]
    if is_half(name):
        pts = [(v, 0.0, s) for v, m, s in pts if m in (0.0, 0.2, -0.4)]
        pts += [(-0.0, 0.0, 1.3), (-1.0, 0.0, 1.3), (-1e-30, 0.0, 1.3), (-inf, 0.0, 1.3),
                (-1.0, 0.0, nan), (-1.0, 0.0, 0.0)]
    a = np.array(pts, F32)
    return a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy()


def _node(name, nu, v, m, s):
    from mlx_mcmc_amd import _trace
    E = _trace.Expr
    ev, es = E.of(v), E.of(s)
    if is_half(name):
        return E(OP[name], [ev, None, es], leaf=float(nu),
                 shape=_trace._bshape(name, [ev.shape, es.shape]))
    em = E.of(m)
    return E(OP[name], [ev, em, es], leaf=float(nu),
             shape=_trace._bshape(name, [ev.shape, em.shape, es.shape]))


# parameter names of the forms (tests/_expr_ops.py's): value, loc, scale
PK = {"v": "a", "m": "b", "s": "c"}


def build_S(name, nu):
    """Form S: n = 1, every argument a PSCALAR leaf."""
    from mlx_mcmc_amd import _trace

    def log_prob(p):
        return _trace.expr_term(_node(name, nu, p["a"], p.get("b"), p["c"]))
    return log_prob, {PK[k]: F32(0.5) for k in diff_names(name)}


def build_V(name, nu, form="V"):
    """Forms V / VF / V32 of tests/_expr_ops.py: every argument a PVEC leaf of
    N_VEC elements; V32 pushes the term past 16 nodes with multiplications by
    1, VF multiplies the root by a weight vector whose cotangent is the value."""
    from mlx_mcmc_amd import _trace

    def log_prob(p):
        v = _trace.Expr.of(p["a"])
        if form == "V32":
            for _ in range(17):
                v = _trace.Expr.binary(_lib.MC_EX_MUL, v, 1.0)
        root = _node(name, nu, v, p.get("b"), p["c"])
        if form == "VF":
            root = _trace.Expr.binary(_lib.MC_EX_MUL, p["w"], root)
        return _trace.expr_term(root).sum()
    init = {PK[k]: np.full(N_VEC, 0.5, F32) for k in diff_names(name)}
    if form == "VF":
        init["w"] = np.ones(N_VEC, F32)
    return log_prob, init


def _program(built):
    from mlx_mcmc_amd import _trace
    _lib.require_device()
    return _trace.Program(_trace.trace(*built))


def run_S(name, nu, v, m, s):
    """Device value and VJPs of form S at the points: (value [P], {arg: vjp [P]})."""
    from mlx_mcmc_amd import _engine
    cols = {"v": v, "m": m, "s": s}
    names = diff_names(name)
    lp, g = _engine.logp_grad(_program(build_S(name, nu)),
                              np.stack([np.asarray(cols[k], F32) for k in names], 1))
    lp, g = lp.cpu().numpy(), g.cpu().numpy()
    return lp, {k: g[:, i] for i, k in enumerate(names)}


def run_V(name, nu, v, m, s, form="V"):
    """Device VJPs of form V / V32 per element ({arg: [P]}), or (form VF) the
    values [P]: the P points are laid out N_VEC to a launch point (padded with
    the first points)."""
    from mlx_mcmc_amd import _engine
    cols = {"v": v, "m": m, "s": s}
    names = diff_names(name)
    n = len(v)
    rows = -(-n // N_VEC)
    pad = [np.resize(np.asarray(cols[k], F32), rows * N_VEC).reshape(rows, N_VEC) for k in names]
    if form == "VF":
        pad.append(np.ones((rows, N_VEC), F32))
    _, g = _engine.logp_grad(_program(build_V(name, nu, form)), np.concatenate(pad, 1))
    g = g.cpu().numpy().reshape(rows, len(pad), N_VEC)
    if form == "VF":
        return g[:, -1].reshape(-1)[:n]
    return {k: g[:, j].reshape(-1)[:n] for j, k in enumerate(names)}


# ---- samplers ------------------------------------------------------------------------
def host_draw(nu, m, s, half, seed, chain, it, obs):
    out = ctypes.c_float()
    rc = _lib.load().mc_predictive_draw_student_t(float(nu), float(m), float(s), int(half),
                                                  int(seed), int(chain), int(it), int(obs),
                                                  ctypes.byref(out))
    assert rc == 0, rc
    return F32(out.value)


def host_draws(nu, m, s, half, seed, chain, it, obs):
    """mc_predictive_draw_student_t over broadcast arrays (float32 out)."""
    fn = _lib.load().mc_predictive_draw_student_t
    args = np.broadcast_arrays(np.asarray(m, F32), np.asarray(s, F32), np.asarray(chain),
                               np.asarray(it), np.asarray(obs))
    res = np.empty(args[0].shape, F32)
    out = ctypes.c_float()
    ref = ctypes.byref(out)
    flat = res.reshape(-1)
    seed, nu, half = int(seed), float(nu), int(half)
    for k, (a, b, c, i, o) in enumerate(zip(*(x.reshape(-1).tolist() for x in args))):
        assert fn(nu, a, b, half, seed, c, i, o, ref) == 0
        flat[k] = out.value
    return res


# ---- models ----------------------------------------------------------------------------
def _mx():
    import mlx_mcmc_amd as m
    import mlx_mcmc_amd.core as mx
    return m, mx


def data(seed=33, N=N_OBS, G=8):
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 1.0, N).astype(F32)
    g = rng.integers(0, G, N).astype(np.int32)
    g[:G] = np.arange(G)[::-1]
    y = (0.5 + 0.8 * x + 0.7 * rng.standard_t(4, N)).astype(F32)
    th = rng.normal(0.3, 0.8, G)
    yh = (th[g] + rng.standard_t(3, N)).astype(F32)
    return SimpleNamespace(x=x, g=g, y=y, yh=yh, N=N, G=G)


def regression(oracle, d=None):
    """y ~ StudentT(4, a + b x, exp(log_s)); a, b ~ Normal(0, 2), log_s ~
    Normal(0, 1).  Returns (log_prob, init)."""
    d = d or data()
    init = {"a": F32(0.0), "b": F32(0.0), "log_s": F32(0.0)}
    if not oracle:
        def log_prob(p):
            m, mx = _mx()
            lp = (m.Normal(0.0, 2.0).log_prob(p["a"]) + m.Normal(0.0, 2.0).log_prob(p["b"])
                  + m.Normal(0.0, 1.0).log_prob(p["log_s"]))
            return lp + mx.sum(m.StudentT(4.0, p["a"] + p["b"] * d.x,
                                          mx.exp(p["log_s"])).log_prob(d.y))
        return log_prob, init
    import torch
    from torch import distributions as TD
    x, y = torch.tensor(d.x.astype(np.float64)), torch.tensor(d.y.astype(np.float64))

    def log_prob(p):
        q = {k: v.to(torch.float64) for k, v in p.items()}
        lp = (TD.Normal(0.0, 2.0).log_prob(q["a"]) + TD.Normal(0.0, 2.0).log_prob(q["b"])
              + TD.Normal(0.0, 1.0).log_prob(q["log_s"]))
        return lp + TD.StudentT(4.0, q["a"] + q["b"] * x, torch.exp(q["log_s"])).log_prob(y).sum()
    return log_prob, init


def hierarchy(oracle, d=None):
    """theta[g] ~ Normal(mu, tau), tau = exp(log_tau) ~ HalfCauchy(1) (plus the
    log-Jacobian log_tau), mu ~ Normal(0, 2), y ~ StudentT(3, theta[g], 1)."""
    d = d or data()
    init = {"mu": F32(0.0), "log_tau": F32(0.0), "theta": np.zeros(d.G, F32)}
    if not oracle:
        def log_prob(p):
            m, mx = _mx()
            tau = mx.exp(p["log_tau"])
            lp = m.Normal(0.0, 2.0).log_prob(p["mu"]) + m.HalfCauchy(1.0).log_prob(tau)
            lp = lp + p["log_tau"]
            lp = lp + mx.sum(m.Normal(p["mu"], tau).log_prob(p["theta"]))
            return lp + mx.sum(m.StudentT(3.0, p["theta"][d.g], 1.0).log_prob(d.yh))
        return log_prob, init
    import torch
    from torch import distributions as TD
    y, g = torch.tensor(d.yh.astype(np.float64)), torch.tensor(d.g.astype(np.int64))

    def log_prob(p):
        q = {k: v.to(torch.float64) for k, v in p.items()}
        tau = torch.exp(q["log_tau"])
        lp = TD.Normal(0.0, 2.0).log_prob(q["mu"]) + TD.HalfCauchy(1.0).log_prob(tau)
        lp = lp + q["log_tau"] + TD.Normal(q["mu"], tau).log_prob(q["theta"]).sum()
        return lp + TD.StudentT(3.0, q["theta"][g], 1.0).log_prob(y).sum()
    return log_prob, init


MODELS = {"regression": regression, "hierarchy": hierarchy}


def location(oracle):
    """y_i ~ StudentT(4, mu, 1), mu ~ Normal(0, 10), N = 67: (log_prob, init,
    exact posterior mean, exact sd) — the moments by float64 quadrature on a
    grid of 40001 points over +-12 prior-free standard errors of the median."""
    rng = np.random.default_rng(71)
    y = (1.3 + rng.standard_t(4, N_OBS)).astype(F32)
    y64 = y.astype(np.float64)
    c = float(np.median(y64))
    grid = c + np.linspace(-2.0, 2.0, 40001)
    z2 = (y64[None, :] - grid[:, None]) ** 2
    lp = -2.5 * np.log1p(z2 / 4.0).sum(1) - 0.5 * (grid / 10.0) ** 2
    w = np.exp(lp - lp.max())
    w /= w.sum()
    mean = float((w * grid).sum())
    sd = float(np.sqrt((w * (grid - mean) ** 2).sum()))
    assert w[0] < 1e-30 and w[-1] < 1e-30
    init = {"mu": F32(1.0)}
    if oracle:
        import torch
        from torch import distributions as TD
        ty = torch.tensor(y64)

        def log_prob(p):
            mu = p["mu"].to(torch.float64)
            return TD.Normal(0.0, 10.0).log_prob(mu) + TD.StudentT(4.0, mu, 1.0).log_prob(ty).sum()
    else:
        def log_prob(p):
            m, mx = _mx()
            return m.Normal(0.0, 10.0).log_prob(p["mu"]) + mx.sum(
                m.StudentT(4.0, p["mu"], 1.0).log_prob(y))
    return log_prob, init, mean, sd


def location_step(sd):
    """The fixed step size of the exact-posterior run: ten steps span 1.5
    posterior standard deviations."""
    return round(0.15 * sd, 4)


def likelihood(name, d=None):
    """The likelihoods alone: "regression" StudentT(4, a + b x, s), "cauchy"
    Cauchy(a + b x, s), "half" HalfStudentT(3, s) of |y| — parameters a, b, s
    (half: s).  (product log-likelihood, parameter shapes, float64 / float32
    matrix ll(q, dt), per-draw sampler operands(q) -> (m, s, y), nu, half)."""
    d = d or data()
    x = d.x
    half = name == "half"
    nu = {"regression": 4.0, "cauchy": 1.0, "half": 3.0}[name]
    y = np.abs(d.y).astype(F32) if half else d.y
    shapes = {"s": ()} if half else {"a": (), "b": (), "s": ()}

    def lik(p):
        m, mx = _mx()
        if half:
            return mx.sum(m.HalfStudentT(nu, p["s"]).log_prob(y))
        loc = p["a"] + p["b"] * x
        dist = m.Cauchy(loc, p["s"]) if name == "cauchy" else m.StudentT(nu, loc, p["s"])
        return mx.sum(dist.log_prob(y))

    def ops(q, dt):
        q = np.asarray(q)
        if half:
            return np.zeros(q.shape[:-1] + (d.N,), dt), q[..., 0:1].astype(dt)
        loc = q[..., 0:1].astype(dt) + (q[..., 1:2].astype(dt) * x.astype(dt)).astype(dt)
        return loc.astype(dt), q[..., 2:3].astype(dt)

    node = "half_student_t" if half else "student_t"

    def ll(q, dt):
        loc, s = ops(q, dt)
        with np.errstate(all="ignore"):
            core = _fwd(node, nu, *np.broadcast_arrays(y.astype(dt), loc, s))
        return (core + dt(F32(norm64(nu, half)))).astype(dt)

    def operands(q):
        loc, s = ops(np.asarray(q, F32), F32)
        shp = loc.shape
        return loc, np.broadcast_to(s, shp), np.broadcast_to(y, shp)

    return SimpleNamespace(log_likelihood=lik, shapes=shapes, ll=ll, operands=operands, M=d.N,
                           nu=nu, half=half, y=y)


def draws(model, C=3, S=37, seed=43):
    """[C, S, D] float32: a, b ~ 0.5 N(0, 1); the scale column exp(0.3 N(0, 1))."""
    D = len(model.shapes)
    q = (np.random.default_rng(seed).standard_normal((C, S, D)) * 0.5).astype(F32)
    q[..., -1] = np.exp(0.6 * q[..., -1]).astype(F32)
    return q


def layout_of(model):
    from mlx_mcmc_amd import _trace
    return _trace.layout_of({k: np.zeros(s, F32) for k, s in model.shapes.items()})
