"""One table of the expression nodes (include/mcmc355.h mc_expr_op) for the
per-op tests: tests/test_expr_ops_reference.py (CPU) holds the table to torch
float64 autograd, tests/test_gpu_expr_ops.py holds the evaluators to the table.

Every row states the op's value and its documented VJP (csrc/eval.h ex_bwd's
comment) once, as NumPy code that keeps the dtype of its inputs and performs
the operations in eval.h's order.  Called on float64 copies of the float32
inputs it is the reference (`fwd64` / `vjp64`); called on the float32 inputs
themselves it is the "one IEEE float32 rounding per operation" evaluation
(`fwd32` / `vjp32`), which decides the *class* of an edge result (NaN, the sign
of an infinity, zero or not) where an intermediate leaves the float32 range
(var = s * s of a 1e20 scale) and float64 does not.

The programs are built at _trace.Expr level so that the op under test is a
node, its arguments leaves:

  S    n = 1, every argument a PSCALAR leaf, D = arity: lp[p] is the value and
       grad[p] the VJPs of point p, nothing summed (the wave-task path).
       The comparison rows are where(cmp(a, b), a, b): root WHERE over the
       comparison node, which is also how WHERE itself runs in this form; the
       `where` row (a data mask) has no S form.
  V    n = 193, every cotangent-carrying argument its own PVEC leaf, the rest
       DATA leaves: g[i] is the VJP at element i (the strided path).
  VF   form V times a PVEC leaf w: the root is MUL, the op the node below, and
       the cotangent of w[i] is the op's value at element i — form V's forward
       value per element (its lp is a 193-element sum).
  V32  form V with the first argument passed through 17 MUL-by-CONST-1.0 nodes
       (more than 16 nodes: the NMAX = 32 scratch instantiation).
"""
import functools
import math
from collections import namedtuple

import numpy as np

F32 = np.float32
FLT_MIN = float(np.finfo(F32).tiny)
FLT_MAX = float(np.finfo(F32).max)
SUBN = 1e-41                      # a float32 subnormal
N_VEC = 193                       # form V's element count (no multiple of 64)
P_BULK = 4096
C0_NORMAL = F32(-0.5) * F32(math.log(float(F32(2.0 * math.pi))))
C0_HALFNORMAL = F32(math.log(2.0)) + C0_NORMAL

# op codes (include/mcmc355.h)
(ADD, SUB, MUL, DIV, NEG, EXP, LOG, SQRT, SQUARE, POW, ABS, LOG1P, TANH, SIGMOID, NORMAL_LP,
 HALFNORMAL_LP, EXPONENTIAL_LP, WHERE, GAMMA_LP, BETA_LP, GT, GE, LT, LE) = range(1, 25)


def _quiet(f):
    @functools.wraps(f)
    def g(*a, **k):
        with np.errstate(all="ignore"):
            return f(*a, **k)
    return g


def _lgamma(a):
    """float64 lgamma of the values, rounded once to their dtype (eval.h's
    (float)lgamma((double)a)); +inf at the poles."""
    def one(t):
        if math.isnan(t):
            return math.nan
        if math.isinf(t):
            return math.inf
        try:
            return math.lgamma(t)
        except ValueError:
            return math.inf
    a = np.asarray(a)
    return np.array([one(float(t)) for t in a.ravel()], np.float64).reshape(a.shape).astype(a.dtype)


def _lbeta(a, b):
    a64, b64 = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(all="ignore"):
        return (_lgamma(a64) + _lgamma(b64) - _lgamma(a64 + b64)).astype(np.asarray(a).dtype)


def _c(x, c):
    return x.dtype.type(c)


def _sel(cond, a, b):
    return np.where(cond, a, b).astype(a.dtype)


# ---- values and VJPs (cotangent 1), eval.h's operations in eval.h's order ----
# Two behaviours of eval.h's primitives that are not IEEE's are stated here,
# pinned from what an MI355X returns (commit MEASURED_AT) and from eval.h's
# comments, and apply to the float32 evaluation only:
#   ex_div: divisors beyond 2^126 in magnitude and subnormal divisors are
#           outside its range: nothing is promised there, and `unspecified`
#           reports the points at which a division of the formula meets one;
#   ex_exp: the transcendental unit flushes subnormal results to zero.
_REC = None


def _div(x, y):
    if _REC is not None and y.dtype == F32:
        ay = np.abs(y)
        _REC.append((np.isfinite(y) & (ay > 2.0 ** 126)) | ((ay > 0) & (ay < FLT_MIN)))
    return x / y


_ROUND_OPERANDS = True


def _operand(t):
    """An intermediate that a library routine takes as a float32 operand
    (pow's y - 1): rounded to float32 in the float64 reference as well."""
    return t.astype(F32).astype(t.dtype) if _ROUND_OPERANDS else t


def _exp(x):
    r = np.exp(x)
    return _sel(r < FLT_MIN, np.zeros_like(r), r) if x.dtype == F32 else r


def _normal(v, m, s):
    var = s * s
    d = v - m
    d2 = d * d
    lp = (_c(v, C0_NORMAL) - np.log(s)) - _div(_c(v, 0.5) * d2, var)
    t = _div(d, var)
    return lp, (-t, t, _div(d2, var * s) - _div(_c(v, 1), s))


def _halfnormal(v, s):
    var = s * s
    v2 = v * v
    ok = v >= 0
    lp = (_c(v, C0_HALFNORMAL) - np.log(s)) - _div(_c(v, 0.5) * v2, var)
    zero = np.zeros_like(v)
    return (_sel(ok, lp, _c(v, -np.inf)),
            (_sel(ok, -_div(v, var), zero), _sel(ok, _div(v2, var * s) - _div(_c(v, 1), s), zero)))


def _exponential(v, r):
    ok = v >= 0
    zero = np.zeros_like(v)
    return (_sel(ok, np.log(r) - r * v, _c(v, -np.inf)),
            (_sel(ok, -r, zero), _sel(ok, _div(_c(v, 1), r) - v, zero)))


def _gamma(v, a, b):
    ok = v > 0
    zero = np.zeros_like(v)
    one = _c(v, 1)
    lp = ((a * np.log(b) - _lgamma(a)) + (a - one) * np.log(v)) - b * v
    return (_sel(ok, lp, _c(v, -np.inf)),
            (_sel(ok, _div(a - one, v) - b, zero), _sel(ok, np.log(b) + np.log(v), zero),
             _sel(ok, _div(a, b) - v, zero)))


def _beta(v, a, b):
    ok = (v > 0) & (v < 1)
    zero = np.zeros_like(v)
    one = _c(v, 1)
    lp = ((a - one) * np.log(v) + (b - one) * np.log(one - v)) - _lbeta(a, b)
    return (_sel(ok, lp, _c(v, -np.inf)),
            (_sel(ok, _div(a - one, v) - _div(b - one, one - v), zero), _sel(ok, np.log(v), zero),
             _sel(ok, np.log(one - v), zero)))


def _cmp_row(cmp):
    """where(cmp(a, b), a, b): the branch taken gets the cotangent, a NaN
    operand compares false."""
    def fwd(a, b, z):
        return _sel(cmp(a, b), a, b)

    def vjp(a, b, z, v):
        m = cmp(a, b)
        return (m.astype(a.dtype), (~m).astype(a.dtype))
    return fwd, vjp


def _abs_vjp(x, y, z, v):
    return (_sel(x > 0, np.ones_like(x), _sel(x < 0, -np.ones_like(x), np.zeros_like(x))),)


# name -> (op code, arity, which arguments carry a cotangent, fwd, vjp)
#   fwd(x, y, z) -> value;  vjp(x, y, z, v) -> one entry per cotangent argument
_FORMULAS = {
    "add": (ADD, 2, (1, 1), lambda x, y, z: x + y,
            lambda x, y, z, v: (np.ones_like(x), np.ones_like(x))),
    "sub": (SUB, 2, (1, 1), lambda x, y, z: x - y,
            lambda x, y, z, v: (np.ones_like(x), -np.ones_like(x))),
    "mul": (MUL, 2, (1, 1), lambda x, y, z: x * y, lambda x, y, z, v: (y, x)),
    "div": (DIV, 2, (1, 1), lambda x, y, z: _div(x, y),
            lambda x, y, z, v: (_div(_c(x, 1), y), -_div(x, y * y))),
    "neg": (NEG, 1, (1,), lambda x, y, z: -x, lambda x, y, z, v: (-np.ones_like(x),)),
    "exp": (EXP, 1, (1,), lambda x, y, z: _exp(x), lambda x, y, z, v: (v,)),
    "log": (LOG, 1, (1,), lambda x, y, z: np.log(x), lambda x, y, z, v: (_div(_c(x, 1), x),)),
    "sqrt": (SQRT, 1, (1,), lambda x, y, z: np.sqrt(x),
             lambda x, y, z, v: (_div(_c(x, 1), _c(x, 2) * v),)),
    "square": (SQUARE, 1, (1,), lambda x, y, z: x * x, lambda x, y, z, v: (_c(x, 2) * x,)),
    "pow": (POW, 2, (1, 1), lambda x, y, z: np.power(x, y),
            # (the exponent y - 1 is a float32 operand of powf: rounded so in
            # the float64 reference too)
            lambda x, y, z, v: (y * np.power(x, _operand(y - _c(x, 1))), v * np.log(x))),
    "abs": (ABS, 1, (1,), lambda x, y, z: np.abs(x), _abs_vjp),
    "log1p": (LOG1P, 1, (1,), lambda x, y, z: np.log1p(x),
              lambda x, y, z, v: (_div(_c(x, 1), _c(x, 1) + x),)),
    "tanh": (TANH, 1, (1,), lambda x, y, z: np.tanh(x),
             lambda x, y, z, v: (_c(x, 1) - v * v,)),
    "sigmoid": (SIGMOID, 1, (1,), lambda x, y, z: _div(_c(x, 1), _c(x, 1) + _exp(-x)),
                lambda x, y, z, v: (v * (_c(x, 1) - v),)),
    "normal_lp": (NORMAL_LP, 3, (1, 1, 1), lambda x, y, z: _normal(x, y, z)[0],
                  lambda x, y, z, v: _normal(x, y, z)[1]),
    # (HalfNormal / Exponential: value and scale / rate; the node's loc slot is empty)
    "halfnormal_lp": (HALFNORMAL_LP, 2, (1, 1), lambda x, y, z: _halfnormal(x, y)[0],
                      lambda x, y, z, v: _halfnormal(x, y)[1]),
    "exponential_lp": (EXPONENTIAL_LP, 2, (1, 1), lambda x, y, z: _exponential(x, y)[0],
                       lambda x, y, z, v: _exponential(x, y)[1]),
    "where": (WHERE, 3, (0, 1, 1), lambda x, y, z: _sel(x != 0, y, z),
              lambda x, y, z, v: ((x != 0).astype(y.dtype), (~(x != 0)).astype(y.dtype))),
    "gamma_lp": (GAMMA_LP, 3, (1, 1, 1), lambda x, y, z: _gamma(x, y, z)[0],
                 lambda x, y, z, v: _gamma(x, y, z)[1]),
    "beta_lp": (BETA_LP, 3, (1, 1, 1), lambda x, y, z: _beta(x, y, z)[0],
                lambda x, y, z, v: _beta(x, y, z)[1]),
    "gt": (GT, 2, (1, 1)) + _cmp_row(np.greater),
    "ge": (GE, 2, (1, 1)) + _cmp_row(np.greater_equal),
    "lt": (LT, 2, (1, 1)) + _cmp_row(np.less),
    "le": (LE, 2, (1, 1)) + _cmp_row(np.less_equal),
}
COMPARES = ("gt", "ge", "lt", "le")
OPS = tuple(_FORMULAS)
S_OPS = tuple(n for n in OPS if n != "where")


def code(name):
    return _FORMULAS[name][0]


def arity(name):
    return _FORMULAS[name][1]


def diff_args(name):
    """Indices of the arguments that carry a cotangent."""
    return tuple(i for i, d in enumerate(_FORMULAS[name][2]) if d)


def _pad3(args, dtype):
    args = [np.asarray(a, dtype) for a in args]
    return args + [None] * (3 - len(args))


@_quiet
def fwd64(name, *args):
    """The value in float64 from the float32 inputs."""
    return _FORMULAS[name][3](*_pad3(args, np.float64))


@_quiet
def vjp64(name, *args, round_v=True):
    """The documented VJPs (cotangent 1) in float64, one per cotangent
    argument; v is the float32-rounded fwd64, what a correctly rounded device
    holds (round_v=False: the float64 value, for the comparison with
    autograd)."""
    global _ROUND_OPERANDS
    a = _pad3(args, np.float64)
    v = _FORMULAS[name][3](*a)
    if round_v:
        v = v.astype(F32).astype(np.float64)
    else:
        _ROUND_OPERANDS = False
        try:
            return tuple(_FORMULAS[name][4](*a, v))
        finally:
            _ROUND_OPERANDS = True
    return tuple(_FORMULAS[name][4](*a, v))


@_quiet
def fwd32(name, *args):
    """The value with one IEEE float32 rounding per operation."""
    return _FORMULAS[name][3](*_pad3(args, F32))


@_quiet
def vjp32(name, *args):
    a = _pad3(args, F32)
    return tuple(_FORMULAS[name][4](*a, _FORMULAS[name][3](*a)))


@_quiet
def unspecified(name, *args):
    """(value mask, VJP mask): the points at which a division of the op's
    float32 evaluation has a divisor outside ex_div's stated range."""
    global _REC
    a = _pad3(args, F32)
    out = []
    for f in (lambda: _FORMULAS[name][3](*a),
              lambda: _FORMULAS[name][4](*a, _FORMULAS[name][3](*a))):
        _REC = []
        try:
            f()
            out.append(np.logical_or.reduce([np.zeros(a[0].shape, bool)] + _REC))
        finally:
            _REC = None
    # (the VJP's own divisions; it also recomputes nothing of the value)
    return out[0], out[1]


@_quiet
def vjp_sensitivity(name, *args):
    """|d formula / d v| per cotangent argument for the VJPs stated through the
    node's value v (exp c v, sqrt c / (2 v), pow's c v log x, tanh c (1 - v^2),
    sigmoid c v (1 - v)); 0 elsewhere.  A device value K ulp off moves such a
    VJP by K ulp(v) times this."""
    a = _pad3(args, np.float64)
    v = _FORMULAS[name][3](*a).astype(F32).astype(np.float64)
    zero = np.zeros_like(a[0])
    if name == "exp":
        return (np.ones_like(v),)
    if name == "sqrt":
        return (1.0 / (2.0 * v * v),)
    if name == "pow":
        return (zero, np.abs(np.log(a[0])))
    if name == "tanh":
        return (2.0 * np.abs(v),)
    if name == "sigmoid":
        return (np.abs(1.0 - 2.0 * v),)
    return tuple(zero for _ in diff_args(name))


# ---- bulk domains: log-uniform magnitudes, both signs where legal --------------
def _logu(rng, n, lo, hi, signed=False):
    x = np.exp(rng.uniform(math.log(lo), math.log(hi), n))
    if signed:
        x = x * rng.choice([-1.0, 1.0], n)
    return x.astype(F32)


def _unit(rng, n):
    """(0, 1), log-uniform towards both ends."""
    t = _logu(rng, n, 1e-4, 0.5).astype(np.float64)
    return np.where(rng.random(n) < 0.5, t, 1.0 - t).astype(F32)


_WHERE_MASKS = np.array([0.0, -0.0, 1.0, np.nan, -1.0, 2.5, SUBN, np.inf], F32)


def where_masks(n):
    """The `where` row's data mask: form V bakes one N_VEC-element mask into
    the program, so the mask of element j is a function of j mod N_VEC."""
    return _WHERE_MASKS[(np.arange(n) % N_VEC) % len(_WHERE_MASKS)]


def bulk(name, n=P_BULK):
    """The bulk sweep's inputs (a tuple of `arity` float32 arrays), fixed by
    the op's code.  Sums and differences keep their operands within 2^20 of
    each other so that the float64 reference is exact."""
    rng = np.random.default_rng(1000 + code(name))
    s = lambda lo, hi: _logu(rng, n, lo, hi, True)      # noqa: E731
    p = lambda lo, hi: _logu(rng, n, lo, hi)            # noqa: E731
    if name in ("add", "sub") + COMPARES:
        return s(1e-3, 1e3), s(1e-3, 1e3)
    if name in ("mul", "div"):
        return s(1e-10, 1e10), s(1e-10, 1e10)
    if name in ("neg", "abs", "square"):
        return (s(1e-15, 1e15),)
    if name == "exp":
        return (s(1e-6, 80.0),)
    if name == "log":
        return (p(1e-30, 1e30),)
    if name == "sqrt":
        return (p(1e-30, 1e30),)
    if name == "pow":
        return p(1e-3, 1e3), s(1e-2, 8.0)
    if name == "log1p":
        x = s(1e-9, 1e6)
        return (np.where(x < 0, -_logu(rng, n, 1e-9, 0.999), x).astype(F32),)
    if name in ("tanh", "sigmoid"):
        return (s(1e-5, 30.0),)
    if name == "normal_lp":
        return s(1e-3, 1e2), s(1e-3, 1e2), p(1e-2, 1e2)
    if name in ("halfnormal_lp", "exponential_lp"):
        return p(1e-3, 1e2), p(1e-2, 1e2)
    if name == "where":
        return where_masks(n), s(1e-3, 1e3), s(1e-3, 1e3)
    if name == "gamma_lp":
        return p(1e-3, 1e2), p(0.1, 30.0), p(1e-2, 1e2)
    if name == "beta_lp":
        return _unit(rng, n), p(0.1, 30.0), p(0.1, 30.0)
    raise KeyError(name)


# ---- edges ----------------------------------------------------------------------
SPECIALS = np.array([0.0, -0.0, FLT_MIN, -FLT_MIN, SUBN, -SUBN, FLT_MAX, -FLT_MAX, np.inf, -np.inf,
                     np.nan], F32)
_BENIGN = {"normal_lp": (0.7, -0.4, 1.3), "gamma_lp": (0.7, 2.5, 1.3), "beta_lp": (0.3, 2.5, 1.3),
           "where": (1.0, 0.7, -0.4)}
_P = 2.0 ** -24
_EXTRA = {
    # subnormal divisors; |divisor| around 2^126; exact quotients just below
    # FLT_MIN and just above FLT_MAX; 0/0, x/0, inf/inf (also in the grid)
    "div": [(1.0, SUBN), (SUBN * 8, SUBN), (3.0, -SUBN), (1e-30, 2e-39), (3.0, 2.0 ** 126 * (1 - _P)),
            (3.0, 2.0 ** 126), (3.0, 2.0 ** 126 * (1 + 2 * _P)), (3.0, 2.0 ** 127),
            (-5.0, -1.5 * 2.0 ** 127), (FLT_MIN, 1.0 + 2 * _P), (FLT_MIN * 1.5, 2.0),
            (3e-30, 7e9), (FLT_MAX, 1.0 - _P), (FLT_MAX, 0.5), (3e30, 7e-9), (0.0, 0.0),
            (1.0, 0.0), (-1.0, 0.0), (1.0, -0.0), (np.inf, np.inf), (np.inf, -np.inf)],
    "exp": [(t,) for t in (87.3, -87.3, 88.7, -88.7, 103.9, -103.9, -104.5, 88.72284, -87.33654)],
    "log": [(t,) for t in (SUBN, 1.4e-45, FLT_MIN, 1.0 - _P, 1.0 + 2 * _P, -1.0, -SUBN)],
    "log1p": [(t,) for t in (-1.0, -1.0 + 2 * _P, -_P / 2, _P, -_P, 2.0 ** -12, 1e38, -2.0)],
    "sqrt": [(t,) for t in (0.0, SUBN, 1.4e-45, -1.0)],
    "pow": [(0.0, 2.0), (0.0, 0.0), (-2.0, 3.0), (-2.0, 0.5), (3.7, 1.0), (-3.7, 1.0), (10.0, 38.0),
            (10.0, 39.0), (1e19, 2.0), (1e-19, 2.5), (2.0, -140.0), (0.0, -1.0), (1.0, np.inf)],
    "tanh": [(s * t,) for t in (2.0 ** -13, 8.0, 9.1, 17.0, 89.0, 104.0) for s in (1, -1)],
    "sigmoid": [(s * t,) for t in (2.0 ** -13, 8.0, 9.1, 17.0, 89.0, 104.0) for s in (1, -1)],
    "abs": [(0.0,), (-0.0,)],
    "halfnormal_lp": [(v, 1.3) for v in (-0.0, 0.0, -0.5)]
    + [(0.7, s) for s in (SUBN, 1e-20, 1e20)],
    "exponential_lp": [(v, 1.3) for v in (-0.0, 0.0, -0.5)]
    + [(0.7, s) for s in (SUBN, 1e-20, 1e20)],
    "normal_lp": [(0.7, -0.4, s) for s in (SUBN, 1e-20, 1e20)],
    "gamma_lp": [(v, 2.5, 1.3) for v in (0.0, -0.0, SUBN, -0.5)]
    + [(0.7, 2.5, s) for s in (SUBN, 1e-20, 1e20)] + [(0.7, 1.0, 1.3), (0.7, 1e-20, 1.3)],
    "beta_lp": [(v, 2.5, 1.3) for v in (0.0, 1.0, 1.0 - _P, SUBN, -0.5, 1.5)]
    + [(0.3, 1.0, 1.0), (0.3, 1e-20, 1.3), (0.3, 2.5, 1e20)],
    # ties and NaN operands (the grid holds +-0 ties, inf ties and NaN)
    "gt": [(1.5, 1.5), (-1.5, -1.5)], "ge": [(1.5, 1.5), (-1.5, -1.5)],
    "lt": [(1.5, 1.5), (-1.5, -1.5)], "le": [(1.5, 1.5), (-1.5, -1.5)],
}


def edges(name):
    """The edge inputs (a tuple of `arity` float32 arrays): every pair of
    SPECIALS for one- and two-argument ops, each argument through SPECIALS
    beside benign others for three-argument ops, and the op's own list."""
    k = arity(name)
    rows = []
    if k == 1:
        rows = [(s,) for s in SPECIALS]
    elif k == 2:
        rows = [(a, b) for a in SPECIALS for b in SPECIALS]
    else:
        for i in range(3):
            for s in SPECIALS:
                r = list(_BENIGN[name])
                r[i] = s
                rows.append(tuple(r))
    rows += _EXTRA.get(name, [])
    cols = tuple(np.array([r[i] for r in rows], F32) for i in range(k))
    if name == "where":
        # masks 0, -0.0, 1, NaN (and more) by position; both branches special
        m = where_masks(len(SPECIALS) ** 2)
        return (m, np.repeat(SPECIALS, len(SPECIALS)), np.tile(SPECIALS, len(SPECIALS)))
    return cols


def inputs(name):
    """Bulk sweep followed by the edges; (arrays, number of bulk points)."""
    b, e = bulk(name), edges(name)
    if name == "where":
        n = P_BULK + len(e[1])
        return (where_masks(n),) + tuple(np.concatenate([x, y]) for x, y in zip(b[1:], e[1:])), P_BULK
    return tuple(np.concatenate([x, y]) for x, y in zip(b, e)), P_BULK


# ---- accuracy -------------------------------------------------------------------
EXACT = ("add", "sub", "mul", "neg", "square", "abs", "where") + COMPARES
DOCUMENTED_ULP = {"div": 1.0, "exp": 2.0, "log": 2.0}    # csrc/eval.h's comments

# Maximum error over the bulk sweep on an MI355X against fwd64 / vjp64, in
# `units` (the float32 spacing of the reference, or of the terms it is summed
# from) (a VJP: after the value-sensitivity
# term of ulp_gate is taken off).  "fwd": the value; 0, 1, 2: the VJP of that
# argument.  Measured at commit MEASURED_AT (the parent of the commit that
# added this table).
MEASURED_AT = "370d6b4"
MEASURED_ULP = {
    "div": {"fwd": 0.5, 0: 0.5, 1: 1.406},
    "exp": {"fwd": 0.966, 0: 0.0},
    "log": {"fwd": 1.88, 0: 0.5},
    "sqrt": {"fwd": 0.5, 0: 0.0},
    "pow": {"fwd": 1.162, 0: 1.844, 1: 0.137},
    "log1p": {"fwd": 2.828, 0: 1.483},
    "tanh": {"fwd": 0.947, 0: 0.5},
    "sigmoid": {"fwd": 2.022, 0: 1.483},
    # (log densities: in ulp of their terms' magnitudes, see `units`)
    "normal_lp": {"fwd": 3.083, 0: 2.112, 1: 2.112, 2: 3.117},
    "halfnormal_lp": {"fwd": 2.581, 0: 1.316, 1: 2.157},
    "exponential_lp": {"fwd": 2.246, 0: 0.0, 1: 0.995},
    "gamma_lp": {"fwd": 2.731, 0: 1.433, 1: 2.175, 2: 0.991},
    "beta_lp": {"fwd": 2.93, 0: 1.701, 1: 1.848, 2: 1.874},
}


def fwd_gate(name):
    """The forward bound in ulp: 0 (exact), the documented figure, or twice the
    measured one rounded up (at least 1: two correct float32 evaluations
    differ by the rounding of each intermediate)."""
    if name in EXACT:
        return 0.0
    if name in DOCUMENTED_ULP:
        return DOCUMENTED_ULP[name]
    return max(1.0, math.ceil(2.0 * MEASURED_ULP[name]["fwd"]))


def vjp_gate(name, arg):
    if name in EXACT:
        return 0.0
    return max(1.0, math.ceil(2.0 * MEASURED_ULP[name][arg]))


def ulp(ref):
    """float32 spacing at the float64 reference value."""
    with np.errstate(all="ignore"):
        return np.spacing(np.abs(np.asarray(ref, np.float64)).astype(F32)).astype(np.float64)


def ulp_err(dev, ref):
    with np.errstate(all="ignore"):
        return np.abs(np.asarray(dev, np.float64) - ref) / ulp(ref)


def vjp_slack(name, args, k_fwd):
    """K_fwd ulp(v) |d formula / d v| per cotangent argument (absolute)."""
    with np.errstate(all="ignore"):
        v = fwd64(name, *args)
        return tuple(np.where(s == 0, 0.0, np.nan_to_num(k_fwd * ulp(v) * s, nan=0.0))
                     for s in vjp_sensitivity(name, *args))


@_quiet
def units(name, *args):
    """The ulp in which an error is counted: (value, (VJP, ...)).  The float32
    spacing of the reference — except where the formula is a sum of larger
    terms (the log densities and their cotangents): each term carries its own
    rounding, so there the spacing is that of the terms' magnitudes summed
    (never less than the result's).  Without this a cancelling point (lp near
    0, a / b - v near 0) sets a gate of thousands of ulp for every point."""
    a = _pad3(args, np.float64)
    x, y, z = a
    L = lambda t: np.abs(np.log(t))   # noqa: E731
    f, g = fwd64(name, *args), vjp64(name, *args)
    sf, sg = np.abs(f), [np.abs(t) for t in g]
    if name == "normal_lp":
        d2 = (x - y) ** 2
        sf = abs(float(C0_NORMAL)) + L(z) + 0.5 * d2 / z ** 2
        sg[2] = d2 / z ** 3 + 1 / z
    elif name == "halfnormal_lp":
        sf = abs(float(C0_HALFNORMAL)) + L(y) + 0.5 * x * x / y ** 2
        sg[1] = x * x / y ** 3 + 1 / y
    elif name == "exponential_lp":
        sf = L(y) + y * x
        sg[1] = 1 / y + x
    elif name == "gamma_lp":
        sf = y * L(z) + np.abs(_lgamma(y)) + np.abs(y - 1) * L(x) + z * x
        sg = [np.abs(y - 1) / x + z, L(z) + L(x), y / z + x]
    elif name == "beta_lp":
        # (log(1 - v): the float32 difference 1 - v carries 2^-24 relative,
        # which the logarithm turns into 2^-24 absolute — a term of size 1)
        sf = (np.abs(y - 1) * L(x) + np.abs(z - 1) * (L(1 - x) + 1.0) + np.abs(_lbeta(y, z)))
        sg[0] = np.abs(y - 1) / x + np.abs(z - 1) / (1 - x)
        sg[2] = L(1 - x) + 1.0
    sf = np.where(np.isfinite(sf), np.maximum(sf, np.abs(f)), np.abs(f))
    sg = [np.where(np.isfinite(t), np.maximum(t, np.abs(r)), np.abs(r)) for t, r in zip(sg, g)]
    return ulp(sf), tuple(ulp(t) for t in sg)


def bulk_errors(name, args, fwd, vjps, k_fwd=None):
    """Maximum errors of device results over the points `args`, in `units`:
    {"fwd": value, j: VJP of the j-th cotangent argument after the
    value-sensitivity slack at k_fwd (default: the value's gate) is taken
    off}.  The figures MEASURED_ULP records and the ones the tests gate."""
    uf, ug = units(name, *args)
    with np.errstate(all="ignore"):
        out = {"fwd": float(np.max(np.abs(np.asarray(fwd, np.float64) - fwd64(name, *args)) / uf))}
        if k_fwd is None:
            k_fwd = fwd_gate(name)
        slack = vjp_slack(name, args, k_fwd)
        for j, ref in enumerate(vjp64(name, *args)):
            err = np.maximum(np.abs(np.asarray(vjps[j], np.float64) - ref) - slack[j], 0.0)
            out[j] = float(np.max(err / ug[j]))
    return out


def same_bits(a, b):
    """Equal bits up to the sign of zero; NaN equals NaN."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b)) | ((a == 0) & (b == 0))


def edge_failures(dev, ref64, ref32, skip, gate, slack=0.0, unit=None):
    """Indices of the edge points at which a device result is wrong: its class
    (NaN, -inf, +inf, zero, finite) is neither that of the one-rounding-per-
    operation float32 evaluation nor that of the rounded float64 reference,
    or it is finite and further than `gate` ulp (+ slack) from both.  gate 0:
    equal bits with the rounded float64 reference.  `skip`: points where
    eval.h promises nothing."""
    with np.errstate(all="ignore"):
        r64 = np.asarray(ref64, np.float64)
        cd, c32, c64 = classes(dev), classes(ref32), classes(r64.astype(F32))
        if gate == 0:
            bad = ~same_bits(dev, r64.astype(F32))
        else:
            u = ulp(r64) if unit is None else np.where(np.isfinite(unit), unit, ulp(r64))
            r32 = np.asarray(ref32, np.float64)
            # the float32 evaluation is an alternative only where it departs
            # from the float64 reference (an intermediate left the float32
            # range, or lost its bits there): elsewhere the reference alone
            use32 = (c32 != c64) | ~(np.abs(r32 - r64) <= gate * u)
            bad = (cd != c64) & ~(use32 & (cd == c32))
            e64 = np.abs(np.asarray(dev, np.float64) - r64) - slack
            e32 = np.abs(np.asarray(dev, np.float64) - r32)
            far = ~(e64 <= gate * u) & ~(use32 & (e32 <= gate * ulp(ref32)))
            bad |= (cd == 4) & far
    return np.nonzero(bad & ~skip)[0]


def classes(x):
    """0 NaN, 1 -inf, 2 +inf, 3 zero, 4 finite non-zero."""
    x = np.asarray(x)
    return np.where(np.isnan(x), 0, np.where(np.isinf(x), np.where(x < 0, 1, 2),
                                             np.where(x == 0, 3, 4)))


# ---- programs -------------------------------------------------------------------
_NAMES = ("a", "b", "c")
Built = namedtuple("Built", "log_prob init chain")   # chain: ops the node list must end in


def _root(name, args):
    from mlx_mcmc_amd import _trace
    E = _trace.Expr
    op, k = code(name), arity(name)
    if name in COMPARES:
        return E.where(E.binary(op, args[0], args[1]), args[0], args[1])
    if name == "where":
        return E.where(args[0], args[1], args[2])
    if name in ("halfnormal_lp", "exponential_lp"):
        ev, es = E.of(args[0]), E.of(args[1])
        return E(op, [ev, None, es], shape=_trace._bshape(name, [ev.shape, es.shape]))
    if k == 3:
        ea = [E.of(a) for a in args]
        return E(op, ea, shape=_trace._bshape(name, [e.shape for e in ea]))
    return E.unary(op, args[0]) if k == 1 else E.binary(op, args[0], args[1])


def _chain(name):
    return (code(name), WHERE) if name in COMPARES else (code(name),)


def build_S(name):
    """Form S (not for the data-mask `where` row)."""
    from mlx_mcmc_amd import _trace
    assert name != "where"
    k = arity(name)

    def log_prob(p):
        return _trace.expr_term(_root(name, [p[n] for n in _NAMES[:k]]))
    return Built(log_prob, {n: F32(0.5) for n in _NAMES[:k]}, _chain(name))


def build_V(name, data, form="V"):
    """Forms V / VF / V32.  data: the op's arguments (N_VEC elements each); only
    those of the arguments without a cotangent are used (DATA leaves)."""
    from mlx_mcmc_amd import _lib, _trace
    k, diff = arity(name), diff_args(name)
    fixed = {i: np.ascontiguousarray(data[i][:N_VEC], F32) for i in range(k) if i not in diff}

    def log_prob(p):
        args = [p[_NAMES[i]] if i in diff else fixed[i] for i in range(k)]
        if form == "V32":
            j = diff[0]
            e = _trace.Expr.of(args[j])
            for _ in range(17):
                e = _trace.Expr.binary(_lib.MC_EX_MUL, e, 1.0)
            args[j] = e
        root = _root(name, args)
        if form == "VF":
            root = _trace.Expr.binary(_lib.MC_EX_MUL, p["w"], root)
        return _trace.expr_term(root).sum()
    init = {_NAMES[i]: np.full(N_VEC, 0.5, F32) for i in diff}
    if form == "VF":
        init["w"] = np.ones(N_VEC, F32)
    return Built(log_prob, init, _chain(name) + ((MUL,) if form == "VF" else ()))


def traced(built):
    """Trace on the host; asserts one expression term whose node list ends in
    the intended ops."""
    from mlx_mcmc_amd import _lib, _trace
    model = _trace.trace(built.log_prob, built.init)
    assert len(model.terms) == 1 and model.terms[0].dist == _lib.MC_DIST_EXPR
    assert model.terms[0].weight == 1.0 and model.lp_const == 0.0
    ops = [model.c_nodes[i].op for i in range(model.n_nodes)]
    assert tuple(ops[-len(built.chain):]) == built.chain, (ops, built.chain)
    return model


def node_ops(model):
    return [model.c_nodes[i].op for i in range(model.n_nodes)]


def leaf_kinds(model):
    from mlx_mcmc_amd import _lib
    return [model.c_nodes[i].leaf.kind for i in range(model.n_nodes)
            if model.c_nodes[i].op == _lib.MC_EX_LEAF]


def _program(built):
    from mlx_mcmc_amd import _lib, _trace
    _lib.require_device()
    return _trace.Program(traced(built))


def run_S(name, args):
    """Device value and VJPs of form S at the points: (value [P], (vjp [P], ...))."""
    from mlx_mcmc_amd import _engine
    prog = _program(build_S(name))
    lp, g = _engine.logp_grad(prog, np.stack(args, 1))
    lp, g = lp.cpu().numpy(), g.cpu().numpy()
    return lp, tuple(g[:, i] for i in diff_args(name))


def run_V(name, args, form="V"):
    """Device VJPs of form V / V32 per element, or (form VF) the values: the
    P points are laid out N_VEC to a launch point (padded with the first)."""
    from mlx_mcmc_amd import _engine
    n = len(args[0])
    rows = -(-n // N_VEC)
    pad = [np.concatenate([a, a[:rows * N_VEC - n]]).reshape(rows, N_VEC) for a in args]
    diff = diff_args(name)
    if name == "where":   # the mask is a function of the position in the row
        assert np.array_equal(args[0], where_masks(n), equal_nan=True)
        pad[0] = where_masks(rows * N_VEC).reshape(rows, N_VEC)
    q = [pad[i] for i in diff]
    if form == "VF":
        q.append(np.ones((rows, N_VEC), F32))
    prog = _program(build_V(name, [p[0] for p in pad], form))
    lp, g = _engine.logp_grad(prog, np.concatenate(q, 1))
    g = g.cpu().numpy().reshape(rows, len(q), N_VEC)
    if form == "VF":
        return g[:, -1].reshape(-1)[:n]
    return tuple(g[:, j].reshape(-1)[:n] for j in range(len(diff)))


# ---- the ops as torch functions (float64 autograd) --------------------------------
def torch_ops(documented=False):
    """name -> torch function of the op's arguments.  documented=False: plain
    autograd of the op (the independent check of this table).  documented=True:
    the Gamma / Beta normalisers detached, so that autograd gives the
    documented shape cotangents (no digamma) — the float64 restatement of
    the models the samplers run."""
    import torch
    c0n, c0h = float(C0_NORMAL), float(C0_HALFNORMAL)
    lg = (lambda t: torch.lgamma(t).detach()) if documented else torch.lgamma
    return {
        "add": lambda x, y: x + y, "sub": lambda x, y: x - y, "mul": lambda x, y: x * y,
        "div": lambda x, y: x / y, "neg": lambda x: -x, "exp": torch.exp, "log": torch.log,
        "sqrt": torch.sqrt, "square": lambda x: x * x, "pow": torch.pow, "abs": torch.abs,
        "log1p": torch.log1p, "tanh": torch.tanh, "sigmoid": torch.sigmoid,
        # (the normalisers are the project's float32 constants)
        "normal_lp": lambda v, m, s: c0n - torch.log(s) - 0.5 * ((v - m) / s) ** 2,
        "halfnormal_lp": lambda v, s: c0h - torch.log(s) - 0.5 * (v / s) ** 2,
        "exponential_lp": lambda v, r: torch.log(r) - r * v,
        "where": lambda m, y, z: torch.where(m != 0, y, z),
        "gamma_lp": lambda v, a, b: a * torch.log(b) - lg(a) + (a - 1) * torch.log(v) - b * v,
        "beta_lp": lambda v, a, b: ((a - 1) * torch.log(v) + (b - 1) * torch.log1p(-v)
                                    - (lg(a) + lg(b) - lg(a + b))),
        "gt": lambda a, b: torch.where(a > b, a, b), "ge": lambda a, b: torch.where(a >= b, a, b),
        "lt": lambda a, b: torch.where(a < b, a, b), "le": lambda a, b: torch.where(a <= b, a, b),
    }


def oracle_V(name):
    """Form V's log density as a float64 torch function of the parameter dict
    (oracle/samplers.py's model form): sum_i op(a_i, b_i, c_i)."""
    import torch
    f = torch_ops(True)[name]
    names = [_NAMES[i] for i in diff_args(name)]
    assert len(names) == arity(name)

    def log_prob(p):
        return f(*[p[n].to(torch.float64) for n in names]).sum()
    return log_prob


# ---- three sampling models that hold every op as a node ---------------------------
# theta[n] under a fused Normal(0, 1) prior, broadcast scalars where an op
# takes a second parameter, terms 0.1 * sum_i op(f(theta_i), x_i) over data
# vectors of the same length; at most 32 nodes and 1 .. 6 data leaves per term
# (the lane planner takes no expression term without a data array, and a
# program with parameter-vector leaves only from 2048 elements on, summed over
# its terms, and at most 256 private parameters in a slice: csrc/host.h
# expr_term_class / kLrAutoMinElements, plan_lanes.hip — hence eight
# expression terms and N_GROUP = 250 elements for the lane runs).  With
# N_TAPE = 96 elements the automatic plan keeps the program on the tape
# kernels, which is what the tape-JIT bit-identity test needs.  Written once
# over a small builder interface B (p: a parameter, d: a data vector, c: a
# constant, op / cmp / where: nodes) with two backends: _trace.Expr nodes for
# the kernels and torch float64 for the restatement.
N_GROUP = 250
N_TAPE = 96
_CMP = {"gt": GT, "ge": GE, "lt": LT, "le": LE}


def _group_data(seed, k, n, lo=0.5, hi=2.0, signed=False):
    rng = np.random.default_rng(seed)
    x = rng.uniform(lo, hi, (k, N_GROUP))
    if signed:
        x = x * rng.choice([-1.0, 1.0], (k, N_GROUP))
    return x.astype(F32)[:, :n]


def _arith_terms(B, n):
    th = B.p("theta")
    s = B.op("mul", B.c(0.1), B.p("s"))   # (a broadcast parameter sums 250 curvatures)
    x = [B.d(a) for a in _group_data(11, 6, n, 0.5, 2.0, True)]
    mask = B.d((np.arange(n) % 3 != 0).astype(F32))
    o = B.op
    terms = [
        o("neg", o("square", o("sub", o("add", th, x[0]), o("mul", s, x[1])))),
        o("neg", o("div", o("abs", th), o("add", o("square", x[2]), B.c(1.0)))),
        B.where(mask, o("mul", th, x[3]), o("neg", o("abs", o("sub", th, x[4])))),
    ]
    terms.append(o("neg", o("div", x[2], o("add", o("square", th), o("abs", x[1])))))
    for k, name in enumerate(COMPARES):
        # (max / min of the parameter and a data value times a parameter
        # product: continuous, so a leapfrog step across a tie keeps its energy)
        terms.append(o("mul", B.where(B.cmp(name, th, x[k]), th, x[k]), o("mul", s, x[5])))
    return terms


def _transc_terms(B, n):
    th, a = B.p("theta"), B.p("a")
    raw = _group_data(12, 10, n)
    x = [B.d(v) for v in raw[:7]]
    o = B.op
    sq = lambda t: o("square", t)   # noqa: E731
    # exp, sigmoid and log1p(exp) at arguments in the tens, where the low part
    # of x log2(e) in ex_exp / ex2_exp is worth several ulp of the result, each
    # under a data weight that brings the term (and its gradient) back to a
    # few units: the gradient then shows in the draw's last bits
    big = lambda c, t: o("add", B.c(c), t)   # noqa: E731
    w_exp = B.d((raw[7] * 5e-13).astype(F32))     # exp(30) = 1.07e13
    w_sig = B.d((raw[8] * 2.5e9).astype(F32))     # sigmoid(-20) = 2.06e-9
    w_l1p = B.d((raw[9] * 8e5).astype(F32))       # exp(-12) = 6.1e-6
    return [
        o("neg", o("mul", w_exp, o("exp", big(30.0, o("mul", th, x[5]))))),
        o("log", o("add", sq(th), x[0])),
        o("neg", o("sqrt", o("add", sq(th), x[1]))),
        # a parameter base and a parameter exponent
        o("neg", o("pow", o("add", sq(th), x[6]), o("add", o("mul", B.c(0.25), a), B.c(0.75)))),
        o("neg", o("add", o("log1p", o("mul", x[2], sq(th))),
                   o("mul", w_sig, o("sigmoid", big(-20.0, o("mul", th, x[4])))))),
        o("tanh", o("mul", th, x[3])),
        o("log", o("sigmoid", o("mul", th, x[4]))),
        o("neg", o("mul", w_l1p, o("log1p", o("exp", big(-12.0, o("mul", o("tanh", th), x[0])))))),
    ]


def _density_terms(B, n):
    th, mu, ls = B.p("theta"), B.p("mu"), B.p("ls")
    x = [B.d(v) for v in _group_data(13, 5, n)]
    o = B.op
    scale = o("exp", o("mul", B.c(0.25), ls))
    shape = o("add", o("exp", o("mul", B.c(0.25), mu)), B.c(1.0))
    pos = o("mul", x[3], o("exp", o("mul", B.c(0.3), th)))
    return [
        o("normal_lp", o("mul", th, x[0]), mu, scale),
        o("halfnormal_lp", pos, scale),
        o("exponential_lp", o("add", o("square", th), x[1]), scale),
        o("gamma_lp", pos, o("add", shape, x[4]), scale),
        o("beta_lp", o("sigmoid", o("mul", th, x[2])), shape, o("add", scale, B.c(0.5))),
        # data values under parameter locs / scales / rates
        o("normal_lp", x[0], th, o("mul", x[1], scale)),
        o("halfnormal_lp", x[1], o("mul", x[3], o("exp", o("mul", B.c(0.3), th)))),
        o("exponential_lp", x[2], pos),
    ]


def _pairs_terms(B, n):
    """Broadcast parameters and data only: the tape JIT runs such terms as
    element pairs (jit.hip gen_term, eval.h ex2_fwd / ex2_bwd), the
    interpreter as scalars, and every cotangent is a sum over the elements.
    exp, sigmoid and log1p(exp) sit at arguments in the tens, where the low
    part of x log2(e) is worth several ulp of exp: a pair routine less
    accurate than the scalar one moves the sums in their sixth digit."""
    a, b = B.p("a"), B.p("b")
    raw = _group_data(14, 6, n)
    x = [B.d(v) for v in raw[:3]]
    o = B.op
    big = lambda c, t: o("add", B.c(c), t)   # noqa: E731
    w_exp = B.d((raw[3] * 2e-14).astype(F32))     # exp(30) = 1.07e13
    w_sig = B.d((raw[4] * 1e8).astype(F32))       # sigmoid(-20) = 2.06e-9
    w_l1p = B.d((raw[5] * 3e4).astype(F32))       # exp(-12) = 6.1e-6
    return [
        o("neg", o("mul", w_exp, o("exp", big(30.0, o("mul", a, x[0]))))),
        o("neg", o("mul", w_sig, o("sigmoid", big(-20.0, o("mul", b, x[1]))))),
        o("neg", o("mul", w_l1p, o("log1p", o("exp", big(-12.0, o("mul", o("tanh", a), x[2])))))),
    ]


GROUPS = {"ops_arith": (_arith_terms, ("theta", "s")),
          "ops_transc": (_transc_terms, ("theta", "a")),
          "ops_density": (_density_terms, ("theta", "mu", "ls"))}
PAIRS = (_pairs_terms, ("a", "b"))    # group_model("ops_pairs"): the tape JIT's pair code
GROUP_OPS = {"ops_arith": ("add", "sub", "mul", "div", "neg", "square", "abs", "where") + COMPARES,
             "ops_transc": ("exp", "log", "sqrt", "pow", "log1p", "tanh", "sigmoid"),
             "ops_density": ("normal_lp", "halfnormal_lp", "exponential_lp", "gamma_lp", "beta_lp")}


class _ExprBackend:
    def __init__(self, params):
        from mlx_mcmc_amd import _trace
        self.E, self.params = _trace.Expr, params

    def p(self, name):
        return self.E.of(self.params[name])

    def d(self, arr):
        return self.E.of(np.ascontiguousarray(arr, F32))

    def c(self, v):
        return self.E.of(float(v))

    def op(self, name, *args):
        return _root(name, list(args))

    def cmp(self, name, a, b):
        return self.E.binary(_CMP[name], a, b)

    def where(self, mask, a, b):
        return self.E.where(mask.leaf if mask.op == 0 else mask, a, b)


class _TorchBackend:
    def __init__(self, params):
        import torch
        self.t, self.params, self.f = torch, params, torch_ops(True)

    def p(self, name):
        return self.params[name].to(self.t.float64)

    def d(self, arr):
        return self.t.tensor(np.asarray(arr, np.float64))

    def c(self, v):
        return self.t.tensor(float(F32(v)), dtype=self.t.float64)

    def op(self, name, *args):
        return self.f[name](*args)

    def cmp(self, name, a, b):
        return {"gt": a > b, "ge": a >= b, "lt": a < b, "le": a <= b}[name]

    def where(self, mask, a, b):
        return self.t.where(mask if mask.dtype == self.t.bool else mask != 0, a, b)


def group_model(group, n=N_GROUP):
    """ns -> (log_prob, initial_params): the model for the product namespace
    (workloads.ns_product(): traced, every op a node) or, for the oracle
    namespace, its float64 torch restatement."""
    terms, names = PAIRS if group == "ops_pairs" else GROUPS[group]

    def factory(ns):
        init = {k: (np.zeros(n, F32) if k == "theta" else F32(0.0)) for k in names}
        if getattr(ns, "name", "") == "oracle":
            def log_prob(p):
                import torch
                lp = sum((float(C0_NORMAL) - 0.5 * p[k].to(torch.float64) ** 2).sum() for k in names)
                for r in terms(_TorchBackend(p), n):
                    lp = lp + float(F32(0.1)) * (r + torch.zeros(n, dtype=torch.float64)).sum()
                return lp
            return log_prob, init

        def log_prob(p):
            from mlx_mcmc_amd import _trace
            lp = sum(ns.sum(ns.Normal(0, 1).log_prob(p[k])) for k in names)
            for r in terms(_ExprBackend(p), n):
                lp = lp + 0.1 * _trace.expr_term(r).sum()
            return lp
        return log_prob, init
    return factory
