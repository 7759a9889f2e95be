"""The count likelihoods (Bernoulli, Binomial, Poisson) for their tests:
tests/test_discrete_host.py (no device) and tests/test_gpu_discrete.py.

Nodes.  ``NODES`` states each count node of include/mcmc355.h once — value and
VJP as NumPy code that keeps the dtype of its inputs and performs eval.h's
operations in eval.h's order (the pattern of tests/_expr_ops.py): on float64
copies of the float32 inputs it is the reference (``fwd64`` / ``vjp64``), on
the float32 inputs the one-rounding-per-operation evaluation that decides the
class of an edge result (``fwd32`` / ``vjp32``).

Ulp bounds.  Derived from eval.h's documented figures, never from the new
nodes: ex_exp within K_EXP = 2 ulp (_expr_ops.DOCUMENTED_ULP).  ex_log1p and
the sigmoid quotient 1 / (1 + exp(-x)) — exactly what MC_EX_SIGMOID forms —
have no documented bound: their existing _expr_ops.MEASURED_ULP entries,
measured on the parent commit, stand in: K_L1P = 2.828, K_SIG = 2.022 ulp of
the value.  An error of K ulp of x is at most K 2^-23 |x| and at least
K 2^-24 |x|, so carrying a relative error from one quantity to another costs
a factor of at most 2 in ulp.

  softplus(s) = max(s, 0) + L, L = log1p(e), e = exp(-|s|) in (0, 1]:
      e is K_EXP ulp(e) off; d log1p / d e = 1 / (1 + e) and L >= e / (1 + e),
      so that moves L by at most 2 K_EXP ulp(L); log1p itself adds K_L1P; the
      sum rounds once (0.5 ulp of the result, which is >= L):
      K_SP = 2 K_EXP + K_L1P + 0.5 = 7.328
  Bernoulli value   -softplus(+-eta): K_SP, gate 8 ulp of the value
  Binomial value    y eta - n softplus(eta): the product y eta rounds once
      (0.5), n softplus rounds once more (K_SP + 0.5), the difference once
      (0.5): K_SP + 1.5 = 8.828, gate 9 in ulp of |y eta| + n softplus(eta)
      (the terms' magnitudes, as _expr_ops.units counts the log densities)
  Poisson value     y theta - e: 0.5 + K_EXP + 0.5 = 3 in ulp of |y theta| + e
      (y = 0: -e, K_EXP)
  Bernoulli VJP     y - sigma: K_SIG + 0.5 = 2.522, gate 3 in ulp of |y| + sigma
  Binomial VJP      y - n sigma: K_SIG + 0.5 + 0.5 = 3.022, gate 4 in ulp of
      |y| + n sigma
  Poisson VJP       y - exp(theta): K_EXP + 0.5, gate 3 in ulp of |y| + e

Samplers.  ``bernoulli_draw`` restates csrc/predictive.h pp_bernoulli in
float32 through oracle/philox.py (bit for bit); ``host_draws`` applies the
library's scalar definition (mc_predictive_draw_discrete) to arrays.

Models.  N = 67 observations (no multiple of 64): Bernoulli(logits = a + b x),
Binomial(n_i, logits = alpha[g] + b x) with 8 groups, Poisson(log_rate =
a + b x), each with Normal(0, 2) priors, for the product namespace and as a
float64 torch restatement (torch.nn.functional.softplus) for
oracle.samplers.EagerModel; the two conjugate models; the likelihoods alone
(with seeded draws) for WAIC / LOO / replicates.
"""
from __future__ import annotations

import ctypes
import math
from types import SimpleNamespace

import numpy as np

import _expr_ops as X
from mlx_mcmc_amd import _lib

F32 = np.float32
# mc_discrete_kind and the nodes' mc_expr_op codes, as the binding states them
BERNOULLI, BINOMIAL, POISSON = (_lib.MC_DISCRETE_BERNOULLI, _lib.MC_DISCRETE_BINOMIAL,
                                _lib.MC_DISCRETE_POISSON)
OP = {"bernoulli": _lib.MC_EX_BERNOULLI_LOGIT_LP, "binomial": _lib.MC_EX_BINOMIAL_LOGIT_LP,
      "poisson": _lib.MC_EX_POISSON_LOG_LP}
N_VEC = X.N_VEC
N_OBS = 67

K_EXP = X.DOCUMENTED_ULP["exp"]
K_L1P = X.MEASURED_ULP["log1p"]["fwd"]
K_SIG = X.MEASURED_ULP["sigmoid"]["fwd"]
K_SP = 2 * K_EXP + K_L1P + 0.5
FWD_GATE = {"bernoulli": math.ceil(K_SP), "binomial": math.ceil(K_SP + 1.5),
            "poisson": math.ceil(K_EXP + 1.0)}
VJP_GATE = {"bernoulli": math.ceil(K_SIG + 0.5), "binomial": math.ceil(K_SIG + 1.0),
            "poisson": math.ceil(K_EXP + 0.5)}


# ---- the nodes: eval.h's operations in eval.h's order ----------------------------
def _c(x, c):
    return x.dtype.type(c)


def _is_count(y):
    return (y >= 0) & np.isfinite(y) & (y == np.floor(y))


def _softplus(x):
    return np.maximum(x, _c(x, 0)) + np.log1p(X._exp(-np.abs(x)))


def _sigmoid(x):
    return _c(x, 1) / (_c(x, 1) + X._exp(-x))


def _support(name, y, n):
    if name == "bernoulli":
        return (y == 0) | (y == 1)
    if name == "binomial":
        return _is_count(y) & _is_count(n) & (y <= n)
    return _is_count(y)


def _fwd(name, y, n, eta):
    ok = _support(name, y, n)
    if name == "bernoulli":
        v = -_softplus(np.where(y != 0, -eta, eta).astype(eta.dtype))
    elif name == "binomial":
        v = y * eta - n * _softplus(eta)
    else:
        e = X._exp(eta)
        v = np.where(y == 0, -e, y * eta - e).astype(eta.dtype)
    return np.where(ok, v, _c(eta, -np.inf)).astype(eta.dtype)


def _vjp(name, y, n, eta):
    ok = _support(name, y, n)
    if name == "bernoulli":
        g = y - _sigmoid(eta)
    elif name == "binomial":
        g = y - n * _sigmoid(eta)
    else:
        g = y - X._exp(eta)
    return np.where(ok, g, _c(eta, 0)).astype(eta.dtype)


def _args(dt, y, n, eta):
    y, n, eta = np.broadcast_arrays(np.asarray(y, F32), np.asarray(0 if n is None else n, F32),
                                    np.asarray(eta, F32))
    return y.astype(dt), n.astype(dt), eta.astype(dt)


@X._quiet
def fwd64(name, y, n, eta):
    return _fwd(name, *_args(np.float64, y, n, eta))


@X._quiet
def vjp64(name, y, n, eta):
    return _vjp(name, *_args(np.float64, y, n, eta))


@X._quiet
def fwd32(name, y, n, eta):
    return _fwd(name, *_args(F32, y, n, eta))


@X._quiet
def vjp32(name, y, n, eta):
    return _vjp(name, *_args(F32, y, n, eta))


@X._quiet
def units(name, y, n, eta):
    """(value unit, VJP unit): the float32 spacing of the summed magnitudes of
    the formula's terms (never less than the result's), see the docstring."""
    y, n, eta = _args(np.float64, y, n, eta)
    f, g = np.abs(fwd64(name, y, n, eta)), np.abs(vjp64(name, y, n, eta))
    if name == "bernoulli":
        sf, sg = f, np.abs(y) + _sigmoid(eta)
    elif name == "binomial":
        sf, sg = np.abs(y * eta) + n * _softplus(eta), np.abs(y) + n * _sigmoid(eta)
    else:
        sf, sg = np.abs(y * eta) + np.exp(eta), np.abs(y) + np.exp(eta)
    sf = np.where(np.isfinite(sf), np.maximum(sf, f), f)
    sg = np.where(np.isfinite(sg), np.maximum(sg, g), g)
    return X.ulp(sf), X.ulp(sg)


def _torch_softplus():
    """torch.nn.functional.softplus as log1p(exp(x)) throughout (its default
    threshold returns x itself above 20: off by exp(-20))."""
    import torch
    return lambda x: torch.nn.functional.softplus(x, threshold=700.0)


def torch_node(name):
    """The node as a plain torch function (autograd is the independent check)."""
    import torch
    sp = _torch_softplus()
    return {"bernoulli": lambda y, n, eta: -sp(torch.where(y != 0, -eta, eta)),
            "binomial": lambda y, n, eta: y * eta - n * sp(eta),
            "poisson": lambda y, n, eta: y * eta - torch.exp(eta)}[name]


# ---- inputs of the per-node GPU tests ------------------------------------------------
ETA_EDGES = np.array([0.0, 17.0, -17.0, 90.0, -90.0, np.inf, -np.inf, np.nan], F32)
# (y, n) per element of form V, cycled over the 193 elements: inside the
# support (n = 0 and y = n among them) and outside it
_YN = {"bernoulli": [(0, 0), (1, 0), (2, 0), (-1, 0), (0.5, 0), (np.nan, 0)],
       "binomial": [(0, 0), (3, 7), (7, 7), (0, 7), (8, 7), (2.5, 7), (2, 6.5), (-1, 7), (1, -3),
                    (40, 100)],
       "poisson": [(0, 0), (4, 0), (1, 0), (250, 0), (-1, 0), (2.5, 0), (np.inf, 0)]}
S_COMBOS = {"bernoulli": [(0, 0), (1, 0), (2, 0)],
            "binomial": [(0, 0), (3, 7), (7, 7), (8, 7)],
            "poisson": [(0, 0), (4, 0), (-1, 0), (2.5, 0)]}
N_BULK_ROWS, N_CONST_BULK = 12, 24


def yn_data(name):
    rows = _YN[name]
    y = np.array([rows[j % len(rows)][0] for j in range(N_VEC)], F32)
    n = np.array([rows[j % len(rows)][1] for j in range(N_VEC)], F32)
    return y, n


def eta_rows(name):
    """[R, N_VEC] float32: N_BULK_ROWS rows of per-element values (log-uniform
    magnitudes in [1e-3, 30], both signs), then rows constant along the
    elements — N_CONST_BULK bulk values and ETA_EDGES — so that every (y, n)
    meets every edge and form S (one eta per point) sees the same inputs.
    Returns (rows, number of bulk rows)."""
    rng = np.random.default_rng(1000 + OP[name])
    hi = 15.0 if name == "poisson" else 30.0
    bulk = X._logu(rng, N_BULK_ROWS * N_VEC, 1e-3, hi, True).reshape(N_BULK_ROWS, N_VEC)
    const = np.concatenate([X._logu(rng, N_CONST_BULK, 1e-3, hi, True), ETA_EDGES])
    rows = np.concatenate([bulk, np.repeat(const[:, None], N_VEC, 1)]).astype(F32)
    return rows, N_BULK_ROWS + N_CONST_BULK


def const_etas(name):
    rows, _ = eta_rows(name)
    return rows[N_BULK_ROWS:, 0].copy()


def _node(name, y, n, eta):
    from mlx_mcmc_amd import _trace
    E = _trace.Expr
    ey, ee = E.of(np.ascontiguousarray(y, F32)), E.of(eta)
    if name == "binomial":
        en = E.of(np.ascontiguousarray(n, F32))
        return E(OP[name], [ey, en, ee], shape=_trace._bshape(name, [ey.shape, en.shape, ee.shape]))
    return E(OP[name], [ey, ee], shape=_trace._bshape(name, [ey.shape, ee.shape]))


def build_S(name, y, n):
    """Form S: n = 1, eta a PSCALAR leaf, y (and n) one-element DATA leaves."""
    from mlx_mcmc_amd import _trace

    def log_prob(p):
        return _trace.expr_term(_node(name, np.array([y], F32), np.array([n], F32), p["a"])).sum()
    return log_prob, {"a": F32(0.5)}


def build_V(name, form="V"):
    """Forms V / VF / V32 of tests/_expr_ops.py: eta a PVEC leaf of N_VEC
    elements, y (and n) DATA leaves (yn_data)."""
    from mlx_mcmc_amd import _lib, _trace
    y, n = yn_data(name)

    def log_prob(p):
        e = _trace.Expr.of(p["a"])
        if form == "V32":
            for _ in range(17):
                e = _trace.Expr.binary(_lib.MC_EX_MUL, e, 1.0)
        root = _node(name, y, n, e)
        if form == "VF":
            root = _trace.Expr.binary(_lib.MC_EX_MUL, p["w"], root)
        return _trace.expr_term(root).sum()
    init = {"a": np.full(N_VEC, 0.5, F32)}
    if form == "VF":
        init["w"] = np.ones(N_VEC, F32)
    return log_prob, init


def run_S(name, y, n, etas):
    from mlx_mcmc_amd import _engine, _trace
    lp_fn, init = build_S(name, y, n)
    prog = _trace.Program(_trace.trace(lp_fn, init))
    lp, g = _engine.logp_grad(prog, np.asarray(etas, F32)[:, None])
    return lp.cpu().numpy(), g.cpu().numpy()[:, 0]


def run_V(name, rows, form="V"):
    """Per element: the VJPs (V / V32) or the values (VF), [R, N_VEC]."""
    from mlx_mcmc_amd import _engine, _trace
    lp_fn, init = build_V(name, form)
    prog = _trace.Program(_trace.trace(lp_fn, init))
    q = rows if form != "VF" else np.concatenate([rows, np.ones_like(rows)], 1)
    _, g = _engine.logp_grad(prog, np.ascontiguousarray(q, F32))
    g = g.cpu().numpy()
    return g[:, N_VEC:] if form == "VF" else g


# ---- samplers -----------------------------------------------------------------------
def bernoulli_draw(eta, seed, chain, it, obs):
    """csrc/predictive.h pp_bernoulli in float32 (oracle/philox.py's operations)."""
    from oracle import philox as R
    eta = np.asarray(eta, F32)
    w = R.draw(seed, chain, it, 7, 0, obs)
    u = R.u01_boxf(w[..., 0])
    um = (F32(1.0) - u).astype(F32)
    with np.errstate(all="ignore"):
        lg = (R.logf_unit(u) - R.logf_unit(np.where(um > 0, um, F32(0.5)))).astype(F32)
    y = np.where(um > 0, (lg < eta).astype(F32), F32(0.0)).astype(F32)
    return np.where(np.isnan(eta), F32(np.nan), y).astype(F32)


def host_draw(kind, total, eta, seed, chain, it, obs):
    from mlx_mcmc_amd import _lib
    out = ctypes.c_float()
    rc = _lib.load().mc_predictive_draw_discrete(int(kind), float(total), float(eta), int(seed),
                                                 int(chain), int(it), int(obs), ctypes.byref(out))
    assert rc == 0, rc
    return F32(out.value)


def host_draws(kind, total, eta, seed, chain, it, obs):
    """mc_predictive_draw_discrete over broadcast arrays (float32 out)."""
    from mlx_mcmc_amd import _lib
    fn = _lib.load().mc_predictive_draw_discrete
    args = np.broadcast_arrays(np.asarray(kind), np.asarray(total, F32), np.asarray(eta, F32),
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


def stats_of(rep, value):
    """tests/_predictive.stats_of plus ``equal``."""
    import _predictive as PP
    out = PP.stats_of(rep, value)
    x = np.asarray(rep, np.float64).reshape(-1, rep.shape[-1])
    v = np.broadcast_to(np.asarray(value, np.float64), rep.shape).reshape(x.shape)
    out["equal"] = (np.isfinite(x) & (x == v)).sum(axis=0).astype(np.float64)
    return out


# ---- models ---------------------------------------------------------------------------
def _mx():
    import mlx_mcmc_amd as m
    import mlx_mcmc_amd.core as mx
    return m, mx


def data(seed=31, N=N_OBS, G=8):
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 1.0, N).astype(F32)
    g = rng.integers(0, G, N).astype(np.int32)
    g[:G] = np.arange(G)[::-1]
    yb = (rng.random(N) < 1.0 / (1.0 + np.exp(-(0.4 + 0.9 * x)))).astype(F32)
    nt = rng.integers(1, 30, N).astype(F32)
    nt[3] = 0.0                                        # an empty trial
    ybin = rng.binomial(nt.astype(np.int64), 1.0 / (1.0 + np.exp(-(-0.2 + 0.7 * x)))).astype(F32)
    yp = rng.poisson(np.exp(0.8 + 0.5 * x)).astype(F32)
    return SimpleNamespace(x=x, g=g, yb=yb, nt=nt, ybin=ybin, yp=yp, N=N, G=G)


def _lgam(v):
    return np.array([math.lgamma(t) for t in np.asarray(v, np.float64).ravel()]).reshape(np.shape(v))


def norm_binomial(y, n):
    """float64 log C(n, y) rounded once to float32 (the tracer's leaf)."""
    y, n = np.asarray(y, np.float64), np.asarray(n, np.float64)
    return (_lgam(n + 1) - _lgam(y + 1) - _lgam(n - y + 1)).astype(F32)


def norm_poisson(y):
    return (-_lgam(np.asarray(y, np.float64) + 1)).astype(F32)


def likelihood(name, d=None):
    """(product log-likelihood, parameter shapes, float64 matrix ll(q, dt) of a
    [.., D] array of draws, per-draw sampler operands(q) -> (kind, total,
    eta, y))."""
    d = d or data()
    x = d.x

    if name == "bernoulli":
        shapes = {"a": (), "b": ()}

        def lik(p):
            m, mx = _mx()
            return mx.sum(m.Bernoulli(logits=p["a"] + p["b"] * x).log_prob(d.yb))

        def eta_of(q, dt):
            return q[..., 0:1].astype(dt) + (q[..., 1:2].astype(dt) * x.astype(dt)).astype(dt)
        kind, tot, y, norm = BERNOULLI, np.zeros(d.N, F32), d.yb, np.zeros(d.N, F32)
    elif name == "binomial":
        shapes = {"alpha": (d.G,), "b": ()}

        def lik(p):
            m, mx = _mx()
            return mx.sum(m.Binomial(d.nt, logits=p["alpha"][d.g] + p["b"] * x).log_prob(d.ybin))

        def eta_of(q, dt):
            return (q[..., :d.G][..., d.g].astype(dt)
                    + (q[..., d.G:d.G + 1].astype(dt) * x.astype(dt)).astype(dt)).astype(dt)
        kind, tot, y, norm = BINOMIAL, d.nt, d.ybin, norm_binomial(d.ybin, d.nt)
    else:
        shapes = {"a": (), "b": ()}

        def lik(p):
            m, mx = _mx()
            return mx.sum(m.Poisson(log_rate=p["a"] + p["b"] * x).log_prob(d.yp))

        def eta_of(q, dt):
            return q[..., 0:1].astype(dt) + (q[..., 1:2].astype(dt) * x.astype(dt)).astype(dt)
        kind, tot, y, norm = POISSON, np.zeros(d.N, F32), d.yp, norm_poisson(d.yp)

    node = {BERNOULLI: "bernoulli", BINOMIAL: "binomial", POISSON: "poisson"}[kind]

    def ll(q, dt):
        eta = eta_of(np.asarray(q), dt)
        with np.errstate(all="ignore"):
            core = _fwd(node, *np.broadcast_arrays(y.astype(dt), tot.astype(dt), eta))
        return (core + norm.astype(dt)).astype(dt)

    def operands(q):
        eta = eta_of(np.asarray(q, F32), F32)
        shp = eta.shape
        return (np.full(shp, kind), np.broadcast_to(tot, shp), eta, np.broadcast_to(y, shp))

    return SimpleNamespace(log_likelihood=lik, shapes=shapes, ll=ll, operands=operands, M=d.N,
                           kind=kind, y=y)


def draws(model, C=3, S=37, seed=41, scale=0.5):
    D = sum(int(np.prod(s)) if s else 1 for s in model.shapes.values())
    return (np.random.default_rng(seed).standard_normal((C, S, D)) * scale).astype(F32)


def layout_of(model):
    from mlx_mcmc_amd import _trace
    return _trace.layout_of({k: np.zeros(s, F32) for k, s in model.shapes.items()})


def posterior_model(name, oracle, d=None):
    """log_prob(params), init: the likelihood under Normal(0, 2) priors — the
    product model, or its float64 torch restatement for oracle.samplers."""
    d = d or data()
    lk = likelihood(name, d)
    init = {k: (np.zeros(s, F32) if s else F32(0.0)) for k, s in lk.shapes.items()}
    if not oracle:
        def log_prob(p):
            m, mx = _mx()
            lp = lk.log_likelihood(p)
            for k in lk.shapes:
                lp = lp + mx.sum(m.Normal(0.0, 2.0).log_prob(p[k]))
            return lp
        return log_prob, init

    import torch
    sp = _torch_softplus()
    t = lambda a: torch.tensor(np.asarray(a, np.float64))   # noqa: E731
    x = t(d.x)
    c0 = float(X.C0_NORMAL) - math.log(2.0)

    def log_prob(p):
        q = {k: v.to(torch.float64) for k, v in p.items()}
        lp = sum((c0 - 0.5 * (q[k] / 2.0) ** 2).sum() for k in lk.shapes)
        if name == "bernoulli":
            eta = q["a"] + q["b"] * x
            return lp + (-sp(torch.where(t(d.yb) != 0, -eta, eta))).sum()
        if name == "binomial":
            eta = q["alpha"][torch.tensor(d.g.astype(np.int64))] + q["b"] * x
            return lp + (t(d.ybin) * eta - t(d.nt) * sp(eta) + t(norm_binomial(d.ybin, d.nt))).sum()
        eta = q["a"] + q["b"] * x
        return lp + (t(d.yp) * eta - torch.exp(eta) + t(norm_poisson(d.yp))).sum()
    return log_prob, init


# ---- conjugate posteriors ------------------------------------------------------------
def conjugate(name, oracle=False):
    """p ~ Beta(2, 3), y_i ~ Binomial(n_i, probs = p): Beta(2 + sum y, 3 +
    sum (n - y)); r ~ Gamma(2, 1), y_i ~ Poisson(rate = r): Gamma(2 + sum y,
    1 + N).  20 observations; both posteriors sit well inside their domains
    (mean 0.36, sd 0.03; mean 3.3, sd 0.4).  Returns (log_prob, init, exact
    mean, exact sd, parameter name)."""
    rng = np.random.default_rng(51)
    if name == "binomial":
        n = rng.integers(5, 20, 20).astype(F32)
        y = rng.binomial(n.astype(np.int64), 0.35).astype(F32)
        a, b = 2.0 + float(y.sum()), 3.0 + float((n - y).sum())
        mean, sd = a / (a + b), math.sqrt(a * b / ((a + b) ** 2 * (a + b + 1)))
        if oracle:
            import torch
            t = lambda v: torch.tensor(np.asarray(v, np.float64))   # noqa: E731

            def log_prob(p):
                q = p["p"].to(torch.float64)
                return (torch.log(q) + 2.0 * torch.log1p(-q)
                        + (t(y) * torch.log(q) + t(n - y) * torch.log1p(-q)).sum())
        else:
            def log_prob(p):
                m, mx = _mx()
                return m.Beta(2.0, 3.0).log_prob(p["p"]) + mx.sum(
                    m.Binomial(n, probs=p["p"]).log_prob(y))
        return log_prob, {"p": F32(0.4)}, mean, sd, "p"
    y = rng.poisson(3.2, 20).astype(F32)
    a, b = 2.0 + float(y.sum()), 1.0 + 20.0
    mean, sd = a / b, math.sqrt(a) / b
    if oracle:
        import torch

        def log_prob(p):
            r = p["r"].to(torch.float64)
            return torch.log(r) - r + float(y.sum()) * torch.log(r) - 20.0 * r
    else:
        def log_prob(p):
            m, mx = _mx()
            return m.Gamma(2.0, 1.0).log_prob(p["r"]) + mx.sum(m.Poisson(rate=p["r"]).log_prob(y))
    return log_prob, {"r": F32(3.0)}, mean, sd, "r"
