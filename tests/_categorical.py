"""The Categorical likelihood for its tests: tests/test_categorical_host.py (no
device) and tests/test_gpu_categorical.py.

Nodes.  MC_EX_LOGADDEXP and MC_EX_PICK of include/mcmc355.h, value and VJP
(cotangent 1) as NumPy code that keeps the dtype of its inputs and performs
eval.h's operations in eval.h's order (the pattern of tests/_expr_ops.py and
tests/_discrete.py): on float64 copies of the float32 inputs the reference
(``lae64`` / ``lae_vjp64``), on the float32 inputs the one-rounding-per-
operation evaluation that decides the class of an edge result (``lae32`` /
``lae_vjp32``).  PICK is a selection: exact.

Ulp gates.  Derived from eval.h's documented figures and the existing
_expr_ops entries, never from the new nodes (tests/_discrete.py derives K_SP
the same way): ex_exp within K_EXP = 2 ulp (_expr_ops.DOCUMENTED_ULP); ex_log1p
and the sigmoid quotient 1 / (1 + exp(-x)) at their _expr_ops.MEASURED_ULP
entries, K_L1P = 2.828 and K_SIG = 2.022 ulp of the value.  An error of K ulp
of x is at most K 2^-23 |x| and at least K 2^-24 |x|: carrying a relative
error from one quantity to another costs a factor of at most 2 in ulp.

  value  v = m + L, m = max(a, b), L = log1p(e), e = exp(-|d|), d = a - b,
      counted in U = ulp(max(|a|, |b|) + L) (never less than ulp(v), ulp(m) or
      ulp(L)):
      d rounds once, 0.5 ulp(d) <= ulp(max(|a|, |b|)) since |d| <= 2 max; it
          moves L by |dL/dd| = e / (1 + e) <= 1/2 of that:            0.5 U
      e is K_EXP ulp(e) off; dL/de = 1 / (1 + e) and L >= e / (1 + e), so L
          moves by at most 2 K_EXP ulp(L):                        2 K_EXP U
      log1p itself:                                                 K_L1P U
      the sum m + L rounds once, |v| <= max(|a|, |b|) + L:            0.5 U
      K_LAE = 2 K_EXP + K_L1P + 1 = 7.828, gate 8
      (ex_exp flushes e below FLT_MIN to 0: L is off by < 1.2e-38 there while
      |d| > 87 makes U >= ulp(43): nothing)
  VJP   da = c sigma(d), db = c - da, counted in ulp of the cotangent c (a
      vanishing sigma would set a unit of nothing):
      d's rounding, 2^-24 |d|, moves sigma by |d| sigma (1 - sigma) 2^-24
          <= 0.2240 2^-24 (the maximum of x e^-x / (1 + e^-x)^2, at 1.5434),
          times c, and c 2^-24 <= ulp(c):                        0.224 ulp(c)
      sigma is K_SIG ulp(sigma) <= K_SIG 2^-23 sigma <= K_SIG 2^-23 off, times
          c, and c 2^-23 <= 2 ulp(c):                          2 K_SIG ulp(c)
      the product rounds once, |da| <= |c|:                        0.5 ulp(c)
      K_DA = 2 K_SIG + 0.724 = 4.768, gate 5
      db carries da's error and rounds once more, |db| <= |c|:
      K_DB = K_DA + 0.5 = 5.268, gate 6

Models.  N = 67 observations (no multiple of 64, odd for the pair code), three
classes, class 0 the reference: the intercept-only model (two scalar logits)
and the regression [0, a1 + b1 x, a2 + b2 x], Normal(0, 2) priors, for the
product namespace and as float64 torch restatements (torch.logsumexp) for
oracle.samplers.EagerModel; the example-05 probs= model (p3 = 1 - p1 - p2,
Beta(2, 2) priors) with its float64 restatement (a Python branch outside the
simplex, as the reference example has it); the exact-posterior model (counts
14 / 9 / 7) with its 2-D quadrature; the regression likelihood alone with
seeded draws for WAIC / LOO.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np

import _expr_ops as X
from mlx_mcmc_amd import _lib

F32 = np.float32
LAE, PICK = _lib.MC_EX_LOGADDEXP, _lib.MC_EX_PICK
N_OBS = 67
N_VEC = 67            # the node forms' element count

K_EXP = X.DOCUMENTED_ULP["exp"]
K_L1P = X.MEASURED_ULP["log1p"]["fwd"]
K_SIG = X.MEASURED_ULP["sigmoid"]["fwd"]
K_LAE = 2 * K_EXP + K_L1P + 1.0
K_DA = 2 * K_SIG + 0.224 + 0.5
K_DB = K_DA + 0.5
LAE_GATE, DA_GATE, DB_GATE = math.ceil(K_LAE), math.ceil(K_DA), math.ceil(K_DB)


# ---- the nodes: eval.h's operations in eval.h's order ----------------------------
def _c(x, c):
    return x.dtype.type(c)


def _diff(a, b):
    return np.where(a == b, _c(a, 0), a - b).astype(a.dtype)


def _lae(a, b):
    d = _diff(a, b)
    # (np.fmax: fmaxf drops a NaN argument; the NaN arrives through d)
    return np.fmax(a, b) + np.log1p(X._exp(-np.abs(d)))


def _lae_vjp(a, b):
    da = _c(a, 1) / (_c(a, 1) + X._exp(-_diff(a, b)))
    return da, _c(a, 1) - da


def _pair(dt, a, b):
    a, b = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32))
    return a.astype(dt), b.astype(dt)


@X._quiet
def lae64(a, b):
    return _lae(*_pair(np.float64, a, b))


@X._quiet
def lae32(a, b):
    return _lae(*_pair(F32, a, b))


@X._quiet
def lae_vjp64(a, b):
    return _lae_vjp(*_pair(np.float64, a, b))


@X._quiet
def lae_vjp32(a, b):
    return _lae_vjp(*_pair(F32, a, b))


@X._quiet
def lae_unit(a, b):
    """ulp of max(|a|, |b|) + log1p(e), never less than the value's."""
    a, b = _pair(np.float64, a, b)
    s = np.maximum(np.abs(a), np.abs(b)) + np.log1p(np.exp(-np.abs(_diff(a, b))))
    f = np.abs(lae64(a, b))
    return X.ulp(np.where(np.isfinite(s), np.maximum(s, f), f))


def pick(y, k, b, c):
    """y == k ? b : c per element (a NaN y takes c), and the cotangents' 1 / 0."""
    y, b, c = np.broadcast_arrays(np.asarray(y, F32), np.asarray(b, F32), np.asarray(c, F32))
    hit = y == F32(k)
    return np.where(hit, b, c).astype(F32), hit.astype(F32), (~hit).astype(F32)


def log_softmax64(etas, y):
    """float64 log mass of labels y under class logits etas [K, ...]: the
    chained nodes' value in exact arithmetic (-inf outside 0 .. K-1)."""
    etas = np.asarray(etas, np.float64)
    y = np.asarray(y, np.float64)
    with np.errstate(all="ignore"):
        m = np.max(etas, axis=0)
        lse = m + np.log(np.sum(np.exp(etas - m), axis=0))
        out = np.full(np.broadcast_shapes(lse.shape, y.shape), -np.inf)
        for k in range(etas.shape[0]):
            out = np.where(y == k, etas[k] - lse, out)
    return out


# ---- inputs of the per-node GPU tests ------------------------------------------------
# (a, b) pairs constant along the elements: the edges, which form S sees too
_INF, _NAN = np.inf, np.nan
LAE_EDGES = np.array([(0.7, 0.7), (-3.25, -3.25), (0.0, -0.0), (1e30, 1e30),
                      (17.0, 0.0), (0.0, 17.0), (-2.0, 15.0), (90.0, 0.0), (0.0, 90.0),
                      (45.5, -44.5), (-44.5, 45.5), (1000.0, 0.0), (-1000.0, 0.0),
                      (-_INF, 1.5), (1.5, -_INF), (-_INF, -_INF), (_INF, 1.0), (1.0, _INF),
                      (_INF, _INF), (_INF, -_INF), (_NAN, 1.0), (1.0, _NAN), (_NAN, _NAN),
                      (_NAN, -_INF)], F32)
N_BULK_ROWS, N_CONST_BULK = 24, 24


def lae_rows():
    """(A, B) [R, N_VEC] float32: N_BULK_ROWS rows of per-element pairs — b of
    log-uniform magnitude in [1e-3, 50] and both signs, the difference a - b
    over +-100 (uniform, and every fourth of log-uniform magnitude from 1e-3,
    so that near-equal arguments are covered) — then rows constant along the
    elements, N_CONST_BULK bulk pairs and LAE_EDGES.  Returns (A, B, number of bulk rows)."""
    rng = np.random.default_rng(2800)
    nb = N_BULK_ROWS * N_VEC
    b = X._logu(rng, nb, 1e-3, 50.0, True)
    d = rng.uniform(-100.0, 100.0, nb)
    d[::4] = X._logu(rng, nb, 1e-3, 100.0, True)[::4]
    a = (b + d).astype(F32)
    cb = X._logu(rng, N_CONST_BULK, 1e-3, 50.0, True)
    ca = (cb + rng.uniform(-100.0, 100.0, N_CONST_BULK)).astype(F32)
    const = np.concatenate([np.stack([ca, cb], 1), LAE_EDGES]).astype(F32)
    A = np.concatenate([a.reshape(N_BULK_ROWS, N_VEC), np.repeat(const[:, :1], N_VEC, 1)])
    B = np.concatenate([b.reshape(N_BULK_ROWS, N_VEC), np.repeat(const[:, 1:], N_VEC, 1)])
    return A.astype(F32), B.astype(F32), N_BULK_ROWS + N_CONST_BULK


# labels in, out of and between the classes (cycled over the elements)
PICK_LABELS = np.array([0.0, 1.0, 2.0, 3.0, -1.0, 0.5, 1.5, -0.0, _NAN, _INF, 1.0000001], F32)


def pick_labels():
    return np.array([PICK_LABELS[j % len(PICK_LABELS)] for j in range(N_VEC)], F32)


def pick_rows():
    rng = np.random.default_rng(2900)
    b = rng.normal(0, 3, (6, N_VEC)).astype(F32)
    c = rng.normal(0, 3, (6, N_VEC)).astype(F32)
    b[4], c[4] = F32(-np.inf), F32(np.inf)       # infinite branches pass through
    b[5, ::2], c[5, 1::2] = F32(np.nan), F32(np.nan)
    return b, c


def _node(op, args, leaf=None):
    from mlx_mcmc_amd import _trace
    ea = [_trace.Expr.of(a) for a in args]
    return _trace.Expr(op, ea, leaf=leaf, shape=_trace._bshape("node", [e.shape for e in ea]))


def _build(kind, form, k=1.0, y=None):
    """Forms V / V32 / VF (a, b PVEC leaves of N_VEC elements, PICK's label a
    DATA leaf) and S (one element, a and b PSCALAR leaves, the label a
    one-element DATA leaf) of tests/_expr_ops.py."""
    from mlx_mcmc_amd import _trace

    def log_prob(p):
        a, b = p["a"], p["b"]
        if form == "V32":
            e = _trace.Expr.of(a)
            for _ in range(17):
                e = _trace.Expr.binary(_lib.MC_EX_MUL, e, 1.0)
            a = e
        root = _node(LAE, [a, b]) if kind == "lae" else _node(PICK, [y, a, b], leaf=float(k))
        if form == "VF":
            root = _trace.Expr.binary(_lib.MC_EX_MUL, p["w"], root)
        return _trace.expr_term(root).sum()
    if form == "S":
        return log_prob, {"a": F32(0.5), "b": F32(0.25)}
    init = {"a": np.full(N_VEC, 0.5, F32), "b": np.full(N_VEC, 0.25, F32)}
    if form == "VF":
        init["w"] = np.ones(N_VEC, F32)
    return log_prob, init


def run(kind, form, A, B, k=1.0, y=None):
    """Device results at the rows (A, B): form V / V32 the VJPs (da, db)
    [R, N_VEC]; VF the values [R, N_VEC]; S (A, B one value per row) the
    values and VJPs ([R], ([R], [R]))."""
    from mlx_mcmc_amd import _engine, _trace
    lp_fn, init = _build(kind, form, k, y)
    prog = _trace.Program(_trace.trace(lp_fn, init))
    if form == "S":
        lp, g = _engine.logp_grad(prog, np.ascontiguousarray(np.stack([A, B], 1), F32))
        g = g.cpu().numpy()
        return lp.cpu().numpy(), (g[:, 0], g[:, 1])
    q = [A, B] + ([np.ones_like(A)] if form == "VF" else [])
    _, g = _engine.logp_grad(prog, np.ascontiguousarray(np.concatenate(q, 1), F32))
    g = g.cpu().numpy()
    if form == "VF":
        return g[:, 2 * N_VEC:]
    return g[:, :N_VEC], g[:, N_VEC:2 * N_VEC]


# ---- models ---------------------------------------------------------------------------
def _mx():
    import mlx_mcmc_amd as m
    import mlx_mcmc_amd.core as mx
    return m, mx


def data(seed=37, N=N_OBS):
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 1.0, N).astype(F32)
    eta = np.stack([np.zeros(N), 0.3 + 0.8 * x, -0.4 - 0.6 * x])
    p = np.exp(eta - eta.max(0))
    p /= p.sum(0)
    y = np.array([rng.choice(3, p=p[:, i]) for i in range(N)]).astype(F32)
    return SimpleNamespace(x=x, y=y, N=N)


C0 = float(X.C0_NORMAL) - math.log(2.0)     # Normal(0, 2)'s normaliser


def _t(a):
    import torch
    return torch.tensor(np.asarray(a, np.float64))


def _torch_cat(etas, y):
    """sum_i (eta_{y_i} - logsumexp_k eta_k) in torch: the independent check."""
    import torch
    E = torch.stack([e + torch.zeros_like(etas[-1]) for e in etas], 0)
    idx = torch.tensor(np.asarray(y, np.int64))[None, :]
    return (torch.gather(E, 0, idx)[0] - torch.logsumexp(E, 0)).sum()


REG_SHAPES = {"a1": (), "b1": (), "a2": (), "b2": ()}
INT_SHAPES = {"e1": (), "e2": ()}


def posterior_model(name, oracle, d=None, y=None):
    """name "intercept" (logits [0, e1, e2]) or "regression" ([0, a1 + b1 x,
    a2 + b2 x]) under Normal(0, 2) priors: log_prob(params), init."""
    d = d or data()
    y = d.y if y is None else np.asarray(y, F32)
    shapes = INT_SHAPES if name == "intercept" else REG_SHAPES
    init = {k: F32(0.0) for k in shapes}
    if not oracle:
        def log_prob(p):
            m, mx = _mx()
            if name == "intercept":
                logits = [0.0, p["e1"], p["e2"]]
            else:
                logits = [0.0, p["a1"] + p["b1"] * d.x, p["a2"] + p["b2"] * d.x]
            lp = mx.sum(m.Categorical(logits=logits).log_prob(y))
            for k in shapes:
                lp = lp + m.Normal(0.0, 2.0).log_prob(p[k])
            return lp
        return log_prob, init

    import torch
    x = _t(d.x if y.size == d.N else np.zeros(y.size))

    def log_prob(p):
        q = {k: v.to(torch.float64) for k, v in p.items()}
        lp = sum(C0 - 0.5 * (q[k] / 2.0) ** 2 for k in shapes)
        zero = torch.zeros(y.size, dtype=torch.float64)
        if name == "intercept":
            etas = [zero, q["e1"] + zero, q["e2"] + zero]
        else:
            etas = [zero, q["a1"] + q["b1"] * x, q["a2"] + q["b2"] * x]
        return lp + _torch_cat(etas, y)
    return log_prob, init


def likelihood(d=None):
    """The regression likelihood alone: (product log-likelihood, shapes, the
    float64 matrix ll(q, dt) of a [.., 4] array of draws)."""
    d = d or data()

    def lik(p):
        m, mx = _mx()
        return mx.sum(m.Categorical(
            logits=[0.0, p["a1"] + p["b1"] * d.x, p["a2"] + p["b2"] * d.x]).log_prob(d.y))

    def etas_of(q, dt):
        q = np.asarray(q).astype(dt)
        x = d.x.astype(dt)
        e1 = q[..., 0:1] + (q[..., 1:2] * x).astype(dt)
        e2 = q[..., 2:3] + (q[..., 3:4] * x).astype(dt)
        return np.stack([np.zeros_like(e1), e1.astype(dt), e2.astype(dt)])

    def ll(q, dt=np.float64):
        return log_softmax64(etas_of(q, dt), d.y).astype(dt)

    return SimpleNamespace(log_likelihood=lik, shapes=REG_SHAPES, ll=ll, etas_of=etas_of, M=d.N,
                           y=d.y)


def draws(model, C=3, S=37, seed=43, scale=0.5):
    D = len(model.shapes)
    return (np.random.default_rng(seed).standard_normal((C, S, D)) * scale).astype(F32)


def layout_of(model):
    from mlx_mcmc_amd import _trace
    return _trace.layout_of({k: np.zeros(s, F32) for k, s in model.shapes.items()})


# ---- the example-05 model ------------------------------------------------------------
SIMPLEX_COUNTS = (40, 26, 1)     # the posterior hugs p3 = 0: proposals leave the simplex


def simplex_model(oracle):
    """p1, p2 ~ Beta(2, 2), p3 = 1 - p1 - p2, y_i ~ Categorical(probs = [p1,
    p2, p3]) (examples/05_categorical_model.py).  The product model has no
    Python branch: the probs= lowering gives -inf outside the simplex.  The
    float64 restatement branches as the reference example does."""
    y = np.repeat(np.arange(3), SIMPLEX_COUNTS).astype(F32)
    init = {"p1": F32(0.33), "p2": F32(0.33)}
    if not oracle:
        def log_prob(p):
            m, mx = _mx()
            p3 = 1.0 - p["p1"] - p["p2"]
            return (m.Beta(2.0, 2.0).log_prob(p["p1"]) + m.Beta(2.0, 2.0).log_prob(p["p2"])
                    + mx.sum(m.Categorical(probs=[p["p1"], p["p2"], p3]).log_prob(y)))
        return log_prob, init

    import torch
    n = [float(c) for c in SIMPLEX_COUNTS]
    lbeta = math.lgamma(2.0) * 2 - math.lgamma(4.0)

    def log_prob(p):
        p1, p2 = p["p1"].to(torch.float64), p["p2"].to(torch.float64)
        # (p3 as the float32 tape forms it: two roundings)
        p3 = ((torch.tensor(1.0) - p["p1"].float()) - p["p2"].float()).to(torch.float64)
        if float(p1) <= 0 or float(p2) <= 0 or float(p3) <= 0 or float(p1) >= 1 or float(p2) >= 1:
            return torch.tensor(-math.inf, dtype=torch.float64)
        prior = sum(torch.log(t) + torch.log1p(-t) - lbeta for t in (p1, p2))
        tot = torch.log(p1 + p2 + p3)
        return prior + sum(c * (torch.log(t) - tot) for c, t in zip(n, (p1, p2, p3)))
    return log_prob, init


# ---- the exact posterior ---------------------------------------------------------------
EXACT_COUNTS = (14, 9, 7)


def exact_posterior(grid=1201, half=6.0):
    """Means and standard deviations of (e1, e2) under logits [0, e1, e2],
    Normal(0, 2) priors and counts 14 / 9 / 7, by 2-D quadrature in float64
    (a uniform grid over +-6: the posterior sits within +-2.5 of the origin,
    the integrand is below 1e-20 of its peak at the border)."""
    t = np.linspace(-half, half, grid)
    e1, e2 = np.meshgrid(t, t, indexing="ij")
    n0, n1, n2 = EXACT_COUNTS
    lse = np.logaddexp(0.0, np.logaddexp(e1, e2))
    lp = n1 * e1 + n2 * e2 - (n0 + n1 + n2) * lse - 0.5 * (e1 ** 2 + e2 ** 2) / 4.0
    w = np.exp(lp - lp.max())
    w /= w.sum()
    mean = np.array([(w * e1).sum(), (w * e2).sum()])
    sd = np.sqrt(np.array([(w * (e1 - mean[0]) ** 2).sum(), (w * (e2 - mean[1]) ** 2).sum()]))
    return mean, sd


def exact_labels():
    return np.repeat(np.arange(3), EXACT_COUNTS).astype(F32)
