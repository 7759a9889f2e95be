"""Distributions of the tape: ``Distribution``, ``Normal``, ``HalfNormal``,
``Exponential``, ``Gamma``, ``Beta``, the count likelihoods ``Bernoulli``,
``Binomial``, ``Poisson``, ``Categorical``, and the Student-t family ``StudentT``,
``Cauchy``, ``HalfStudentT``, ``HalfCauchy``.

Same constructor arguments, ``log_prob(value)`` / ``sample(key, shape)``
contract and formulas as the reference (mlx_mcmc/distributions/base.py:6-54,
normal.py:8-80, halfnormal.py:8-86, exponential.py:5-131, gamma.py:8-149,
beta.py:8-151):

  Normal:      log p(x) = -0.5 log(2 pi) - log(scale) - 0.5 (x - loc)^2 / scale^2
  HalfNormal:  log p(x) = log 2 - 0.5 log(2 pi) - log(scale) - 0.5 x^2 / scale^2
               for x >= 0, -inf otherwise
  Exponential: log p(x) = log(rate) - rate x for x >= 0, -inf otherwise
  Gamma:       log p(x) = alpha log(beta) - gammaln(alpha) + (alpha - 1) log x - beta x
               for x > 0, -inf otherwise
  Beta:        log p(x) = (alpha - 1) log x + (beta - 1) log(1 - x) - log B(alpha, beta)
               for 0 < x < 1, -inf otherwise
  (the gammaln normalisers are values without gradient, as the reference's
  host scipy gammaln)

The count likelihoods (not in the reference) are log masses of observed data
under a traced logit / log rate, with softplus(x) = max(x, 0) + log1p(exp(-|x|)):

  Bernoulli(logits=eta):   log p(y) = -softplus(eta) if y = 0, -softplus(-eta) if y = 1
  Binomial(n, logits=eta): log p(y) = log C(n, y) + y eta - n softplus(eta), y = 0 .. n
  Poisson(log_rate=theta): log p(y) = y theta - exp(theta) - log y!, y = 0, 1, ...
  (-inf outside the support; ``probs=`` / ``rate=`` go through eta = logit p /
  theta = log r and give -inf for p outside (0, 1) / r <= 0; the value and
  total_count are data, never traced)

``Categorical(probs= / logits=)`` (mlx_mcmc/distributions/categorical.py) is the
log mass of a label y in 0 .. K-1 under K class arguments:

  log p(y) = eta_y - log sum_k exp(eta_k),  eta_k the logits or log(p_k)
  (-inf for a label outside 0 .. K-1; traced, two chained expression nodes —
  a selection by the label and a pairwise log-sum-exp; see the class)

``StudentT(df, loc, scale)``, ``Cauchy(loc, scale)``, ``HalfStudentT(df, scale)``
and ``HalfCauchy(scale)`` (not in the reference; the Cauchy classes are df = 1)
are heavy-tailed likelihoods and weakly informative scale priors with a
constant df:

  StudentT:     log p(x) = C(df) - log(scale) - (df + 1) / 2 log1p(z^2 / df),
                z = (x - loc) / scale,
                C(df) = lgamma((df + 1) / 2) - lgamma(df / 2) - log(df pi) / 2
  HalfStudentT: log 2 + the same with loc = 0 for x >= 0, -inf otherwise
  (one expression node plus the normaliser constant; concrete values go
  through ``mc_student_t_log_prob``; ``sample`` draws on the host)

Inside a traced ``log_prob(params)`` (any argument is a traced parameter),
``log_prob`` records a fused term for the HIP tape (see _trace.py).  On
concrete values it is evaluated elementwise on the GPU by the same device
code (``mc_dist_log_prob``) and returned as a float32 NumPy array; ``sample``
draws from the engine's Philox stream on the GPU.
"""
from __future__ import annotations

import numpy as np

from . import _lib, _trace
from .random import Key, _as_key


def _to_f32(x):
    return np.asarray(_trace._to_numpy(x), np.float32)


def _gpu_log_prob(dist: int, value, loc, scale) -> np.ndarray:
    import torch

    dev = _lib.require_device()
    v, s = _to_f32(value), _to_f32(scale)
    m = _to_f32(loc) if loc is not None else None
    shapes = [a.shape for a in (v, m, s) if a is not None]
    out_shape = np.broadcast_shapes(*shapes)
    n = int(np.prod(out_shape)) if out_shape else 1

    def dev_arr(a):
        if a is None:
            return None, 1
        if a.size == 1:
            return torch.from_numpy(a.reshape(1).copy()).to(dev), 1
        return torch.from_numpy(np.broadcast_to(a, out_shape).reshape(-1).copy()).to(dev), 0

    tv, bv = dev_arr(v)
    tm, bm = dev_arr(m)
    ts, bs = dev_arr(s)
    out = torch.empty(n, dtype=torch.float32, device=dev)
    lib = _lib.load()
    _lib.check(lib.mc_dist_log_prob(dist, n, _lib.ptr(tv), bv, _lib.ptr(tm), bm,
                                    _lib.ptr(ts), bs, _lib.ptr(out), _lib.stream_handle()))
    return out.cpu().numpy().reshape(out_shape)


class Distribution:
    """Base class: subclasses implement ``log_prob(value)`` and ``sample(key, shape)``
    (mlx_mcmc/distributions/base.py:6-54)."""

    def log_prob(self, value):
        raise NotImplementedError(f"{self.__class__.__name__} must implement log_prob()")

    def sample(self, key, shape=()):
        raise NotImplementedError(f"{self.__class__.__name__} must implement sample()")

    def __repr__(self):
        return f"{self.__class__.__name__}()"


def _scalar_repr(x):
    try:
        return f"{float(np.asarray(_trace._to_numpy(x)).reshape(())):.3f}"
    except Exception:
        return repr(x)


def _gpu_normals(key, shape) -> np.ndarray:
    """Standard normals from the engine's Philox stream (tag USER)."""
    import torch

    dev = _lib.require_device()
    k = _as_key(key)
    shape = tuple(shape) if isinstance(shape, (tuple, list)) else (int(shape),)
    n = int(np.prod(shape)) if shape else 1
    blocks = (n + 3) // 4
    out = torch.empty(max(1, blocks) * 4, dtype=torch.float32, device=dev)
    _lib.check(_lib.load().mc_rng_fill(k.seed, 0, 0, _lib.MC_RNG_TAG_USER, 0, 0, blocks, 2,
                                       _lib.ptr(out), _lib.stream_handle()))
    return out[:n].cpu().numpy().reshape(shape)


class Normal(Distribution):
    """Normal(loc, scale) (mlx_mcmc/distributions/normal.py:8-80)."""

    def __init__(self, loc, scale):
        self.loc = loc
        self.scale = scale

    def log_prob(self, value):
        if _trace.is_symbolic(value, self.loc, self.scale):
            return _trace.make_term(_lib.MC_DIST_NORMAL, "Normal", value, self.loc, self.scale)
        return _gpu_log_prob(_lib.MC_DIST_NORMAL, value, self.loc, self.scale)

    def sample(self, key, shape=()):
        z = _gpu_normals(key, shape)
        return (z * _to_f32(self.scale) + _to_f32(self.loc)).astype(np.float32)

    def __repr__(self):
        return f"Normal(loc={_scalar_repr(self.loc)}, scale={_scalar_repr(self.scale)})"


class HalfNormal(Distribution):
    """HalfNormal(scale) (mlx_mcmc/distributions/halfnormal.py:8-86)."""

    def __init__(self, scale):
        self.scale = scale

    def log_prob(self, value):
        if _trace.is_symbolic(value, self.scale):
            return _trace.make_term(_lib.MC_DIST_HALFNORMAL, "HalfNormal", value, None,
                                    self.scale)
        return _gpu_log_prob(_lib.MC_DIST_HALFNORMAL, value, None, self.scale)

    def sample(self, key, shape=()):
        z = _gpu_normals(key, shape)
        return np.abs(z * _to_f32(self.scale)).astype(np.float32)

    def __repr__(self):
        return f"HalfNormal(scale={_scalar_repr(self.scale)})"


def _gpu_uniforms(key, shape) -> np.ndarray:
    """Uniforms in (0, 1) from the engine's Philox stream (tag USER)."""
    import torch

    dev = _lib.require_device()
    k = _as_key(key)
    shape = tuple(shape) if isinstance(shape, (tuple, list)) else (int(shape),)
    n = int(np.prod(shape)) if shape else 1
    blocks = (n + 3) // 4
    out = torch.empty(max(1, blocks) * 4, dtype=torch.float32, device=dev)
    _lib.check(_lib.load().mc_rng_fill(k.seed, 0, 0, _lib.MC_RNG_TAG_USER, 1, 0, blocks, 1,
                                       _lib.ptr(out), _lib.stream_handle()))
    return out[:n].cpu().numpy().reshape(shape)


def _host_rng(key) -> np.random.Generator:
    """gamma.py:101-109 / beta.py: the reference draws Gamma and Beta samples with
    NumPy seeded from its key; here the seed is the key's Philox seed."""
    return np.random.default_rng(_as_key(key).seed & 0x7FFFFFFF)


class Exponential(Distribution):
    """Exponential(rate) (mlx_mcmc/distributions/exponential.py:5-131)."""

    def __init__(self, rate):
        self.rate = rate

    def log_prob(self, value):
        if _trace.is_symbolic(value, self.rate):
            return _trace.make_term(_lib.MC_DIST_EXPONENTIAL, "Exponential", value, None,
                                    self.rate)
        return _gpu_log_prob(_lib.MC_DIST_EXPONENTIAL, value, None, self.rate)

    def sample(self, key, shape=()):
        # inverse CDF as exponential.py:73-91: -log(1 - u) / rate
        u = _gpu_uniforms(key, shape)
        return (-np.log(np.float32(1) - u) / _to_f32(self.rate)).astype(np.float32)

    def mean(self):
        return np.float32(1.0) / _to_f32(self.rate)

    def variance(self):
        return np.float32(1.0) / (_to_f32(self.rate) ** 2)

    def mode(self):
        return np.zeros_like(_to_f32(self.rate))

    def __repr__(self):
        return f"Exponential(rate={_scalar_repr(self.rate)})"


class Gamma(Distribution):
    """Gamma(alpha, beta=1.0), shape-rate (mlx_mcmc/distributions/gamma.py:8-149)."""

    def __init__(self, alpha, beta=1.0):
        self.alpha = alpha
        self.beta = beta

    def log_prob(self, value):
        if _trace.is_symbolic(value, self.alpha, self.beta):
            return _trace.make_term(_lib.MC_DIST_GAMMA, "Gamma", value, self.alpha, self.beta)
        return _gpu_log_prob(_lib.MC_DIST_GAMMA, value, self.alpha, self.beta)

    def sample(self, key, shape=()):
        a, b = float(_to_f32(self.alpha)), float(_to_f32(self.beta))
        return _host_rng(key).gamma(a, scale=1.0 / b, size=shape).astype(np.float32)

    def mean(self):
        return _to_f32(self.alpha) / _to_f32(self.beta)

    def variance(self):
        return _to_f32(self.alpha) / (_to_f32(self.beta) ** 2)

    def mode(self):
        a, b = _to_f32(self.alpha), _to_f32(self.beta)
        return np.where(a >= 1, (a - 1) / b, np.float32(0)).astype(np.float32)

    def __repr__(self):
        return f"Gamma(alpha={_scalar_repr(self.alpha)}, beta={_scalar_repr(self.beta)})"


class Beta(Distribution):
    """Beta(alpha, beta) (mlx_mcmc/distributions/beta.py:8-151)."""

    def __init__(self, alpha, beta):
        self.alpha = alpha
        self.beta = beta

    def log_prob(self, value):
        if _trace.is_symbolic(value, self.alpha, self.beta):
            return _trace.make_term(_lib.MC_DIST_BETA, "Beta", value, self.alpha, self.beta)
        return _gpu_log_prob(_lib.MC_DIST_BETA, value, self.alpha, self.beta)

    def sample(self, key, shape=()):
        a, b = float(_to_f32(self.alpha)), float(_to_f32(self.beta))
        return _host_rng(key).beta(a, b, size=shape).astype(np.float32)

    def mean(self):
        a, b = _to_f32(self.alpha), _to_f32(self.beta)
        return a / (a + b)

    def variance(self):
        a, b = _to_f32(self.alpha), _to_f32(self.beta)
        return (a * b) / ((a + b) ** 2 * (a + b + 1))

    def mode(self):
        a, b = _to_f32(self.alpha), _to_f32(self.beta)
        return ((a - 1) / (a + b - 2)).astype(np.float32)

    def __repr__(self):
        return f"Beta(alpha={_scalar_repr(self.alpha)}, beta={_scalar_repr(self.beta)})"


def _gpu_discrete_log_prob(kind: int, name: str, value, total, eta) -> np.ndarray:
    """The count node's value on concrete arguments (mc_discrete_log_prob) plus
    the f32 normaliser, added in f32 as the traced ADD node adds it."""
    import torch

    dev = _lib.require_device()
    v, e = _to_f32(value), _to_f32(eta)
    t = _to_f32(total) if total is not None else None
    shapes = [a.shape for a in (v, t, e) if a is not None]
    out_shape = np.broadcast_shapes(*shapes)
    n = int(np.prod(out_shape)) if out_shape else 1

    def dev_arr(a):
        if a is None:
            return None, 1
        if a.size == 1:
            return torch.from_numpy(a.reshape(1).copy()).to(dev), 1
        return torch.from_numpy(np.broadcast_to(a, out_shape).reshape(-1).copy()).to(dev), 0

    tv, bv = dev_arr(v)
    tt, bt = dev_arr(t)
    te, be = dev_arr(e)
    out = torch.empty(n, dtype=torch.float32, device=dev)
    _lib.check(_lib.load().mc_discrete_log_prob(kind, n, _lib.ptr(tv), bv, _lib.ptr(tt), bt,
                                                _lib.ptr(te), be, _lib.ptr(out),
                                                _lib.stream_handle()))
    core = out.cpu().numpy().reshape(out_shape)
    if name == "Bernoulli":
        return core
    norm = np.broadcast_to(_trace.discrete_norm(name, v, t), out_shape)
    return (core + norm).astype(np.float32)


def _one_of(name: str, **kw):
    """Exactly one parameterisation: (its keyword, its value)."""
    given = [(k, v) for k, v in kw.items() if v is not None]
    if len(given) != 1:
        raise ValueError(f"{name} takes exactly one of " + " / ".join(f"{k}=" for k in kw)
                         + f" (got {len(given)})")
    return given[0]


def _logit64(p):
    p = np.asarray(_to_f32(p), np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log(p) - np.log1p(-p)


def _sigmoid64(x):
    x = np.asarray(_to_f32(x), np.float64)
    with np.errstate(over="ignore"):
        return np.where(x >= 0, 1.0 / (1.0 + np.exp(-x)), np.exp(x) / (1.0 + np.exp(x)))


class _Discrete(Distribution):
    """A count likelihood: one natural argument (logit / log rate) or its
    probability / rate form; log_prob's value (and total_count) are data."""

    _name = ""
    _kind = -1
    _natural = ""

    def _total(self):
        return None

    def log_prob(self, value):
        key, arg = self._param
        natural = key == self._natural
        total = self._total()
        if _trace.is_symbolic(value, total, arg):
            return _trace.discrete_expr(self._name, value, total, arg, natural)
        if natural:
            eta = _to_f32(arg)
        else:
            # the lowering's f32 operations: log p - log1p(-p), log r; outside
            # the parameter's domain -inf
            p = _to_f32(arg)
            with np.errstate(divide="ignore", invalid="ignore"):
                if self._name == "Poisson":
                    eta = np.log(p)
                    ok = p > 0
                else:
                    eta = (np.log(p) - np.log1p(-p)).astype(np.float32)
                    ok = (p > 0) & (p < 1)
            eta = np.where(ok, eta, np.float32(0)).astype(np.float32)
        out = _gpu_discrete_log_prob(self._kind, self._name, value, total, eta)
        if not natural:
            out = np.where(np.broadcast_to(ok, out.shape), out, -np.inf).astype(np.float32)
        return out


class Bernoulli(_Discrete):
    """Bernoulli(probs=None, logits=None): y in {0, 1}."""

    _name, _kind, _natural = "Bernoulli", _lib.MC_DISCRETE_BERNOULLI, "logits"

    def __init__(self, probs=None, logits=None):
        self._param = _one_of("Bernoulli", probs=probs, logits=logits)
        self.probs, self.logits = probs, logits

    def _p(self):
        return _sigmoid64(self.logits) if self.probs is None else np.asarray(
            _to_f32(self.probs), np.float64)

    def sample(self, key, shape=()):
        return _host_rng(key).binomial(1, self._p(), size=shape or None).astype(np.float32)

    def mean(self):
        return self._p().astype(np.float32)

    def variance(self):
        p = self._p()
        return (p * (1 - p)).astype(np.float32)

    def __repr__(self):
        k, v = self._param
        return f"Bernoulli({k}={_scalar_repr(v)})"


class Binomial(_Discrete):
    """Binomial(total_count, probs=None, logits=None): y in {0 .. total_count}."""

    _name, _kind, _natural = "Binomial", _lib.MC_DISCRETE_BINOMIAL, "logits"

    def __init__(self, total_count, probs=None, logits=None):
        self._param = _one_of("Binomial", probs=probs, logits=logits)
        self.total_count, self.probs, self.logits = total_count, probs, logits

    def _total(self):
        return self.total_count

    def _p(self):
        return _sigmoid64(self.logits) if self.probs is None else np.asarray(
            _to_f32(self.probs), np.float64)

    def sample(self, key, shape=()):
        n = np.asarray(_to_f32(self.total_count)).astype(np.int64)
        return _host_rng(key).binomial(n, self._p(), size=shape or None).astype(np.float32)

    def mean(self):
        return (_to_f32(self.total_count) * self._p()).astype(np.float32)

    def variance(self):
        p = self._p()
        return (_to_f32(self.total_count) * p * (1 - p)).astype(np.float32)

    def __repr__(self):
        k, v = self._param
        return f"Binomial(total_count={_scalar_repr(self.total_count)}, {k}={_scalar_repr(v)})"


class Poisson(_Discrete):
    """Poisson(rate=None, log_rate=None): y in {0, 1, ...}."""

    _name, _kind, _natural = "Poisson", _lib.MC_DISCRETE_POISSON, "log_rate"

    def __init__(self, rate=None, log_rate=None):
        self._param = _one_of("Poisson", rate=rate, log_rate=log_rate)
        self.rate, self.log_rate = rate, log_rate

    def _rate(self):
        if self.rate is not None:
            return np.asarray(_to_f32(self.rate), np.float64)
        with np.errstate(over="ignore"):
            return np.exp(np.asarray(_to_f32(self.log_rate), np.float64))

    def sample(self, key, shape=()):
        return _host_rng(key).poisson(self._rate(), size=shape or None).astype(np.float32)

    def mean(self):
        return self._rate().astype(np.float32)

    def variance(self):
        return self._rate().astype(np.float32)

    def __repr__(self):
        k, v = self._param
        return f"Poisson({k}={_scalar_repr(v)})"


class Categorical(Distribution):
    """Categorical(probs=None, logits=None): a label y in {0 .. K-1}
    (mlx_mcmc/distributions/categorical.py).  Exactly one of the two.

    The K class arguments are
      * a concrete array [K];
      * a traced 1-D parameter (or expression) of K elements — K scalar class
        arguments, the reference's meaning (num_categories = shape[0]);
      * a Python sequence of K entries, each a number, a data array [N] or a
        traced scalar / [N] expression — per-observation logits such as
        ``[0.0, a1 + b1 * x, a2 + b2 * x]``.  Entries are scalars or share one
        shape.

    ``log_prob(value)`` with a traced argument records one expression term of
    3K + 2 nodes over scalar classes (_trace.categorical_expr); value is data
    or a constant.  A term holds at most 32 nodes: K <= 10 scalar classes,
    K <= 4 classes with one predictor each (a_k + b_k x: 6K + 3 nodes), K = 3
    with two predictors each (9K + 4).  A reference class (a constant 0 entry)
    saves its predictor's nodes.  ``probs=`` normalises by the same log-sum
    (the reference's p / sum p) and gives -inf where some p_k <= 0.

    On concrete arguments ``log_prob`` is a float32 NumPy array: ``probs=``
    as the reference — a lookup in log(p / sum p), -inf for an invalid index;
    ``logits=`` the normalised log-softmax.  This departs from the reference
    on purpose: its ``logits=`` path returns the un-normalised logits
    (categorical.py:59-65, 88), which is not a log mass."""

    def __init__(self, probs=None, logits=None):
        if probs is None and logits is None:
            raise ValueError("Categorical takes one of probs= / logits= (got neither)")
        if probs is not None and logits is not None:
            raise ValueError("Categorical takes one of probs= / logits= (got both)")
        self._natural = logits is not None
        arg = logits if self._natural else probs
        self._entries = self._classes(arg)
        self._traced = _trace.is_symbolic(*self._entries)
        self.num_categories = len(self._entries)
        if self._traced:
            self.probs, self.logits = probs, logits
            return
        stacked = np.stack([np.asarray(e, np.float32) for e in
                            np.broadcast_arrays(*[_to_f32(e) for e in self._entries])], axis=-1)
        with np.errstate(divide="ignore", invalid="ignore"):
            if self._natural:
                z = stacked - np.max(stacked, axis=-1, keepdims=True)
                lse = np.log(np.sum(np.exp(z), axis=-1, keepdims=True, dtype=np.float32))
                self.logits = (z - lse).astype(np.float32)
                self.probs = np.exp(self.logits).astype(np.float32)
            else:
                self.probs = (stacked / np.sum(stacked, axis=-1, keepdims=True,
                                               dtype=np.float32)).astype(np.float32)
                self.logits = np.log(self.probs).astype(np.float32)

    @staticmethod
    def _classes(arg):
        """The K class arguments as a list."""
        if isinstance(arg, (_trace.Param, _trace.Affine, _trace.Expr)):
            shape = tuple(_trace.Expr.of(arg).shape)
            if len(shape) != 1:
                raise _trace.TraceError("Categorical: a traced class argument is a 1-D parameter "
                                        f"of K elements (got shape {shape}); per-observation "
                                        "classes are a sequence of K entries")
            return [arg[k] for k in range(shape[0])]
        if isinstance(arg, (list, tuple)) and _trace.is_symbolic(*arg):
            return list(arg)
        if isinstance(arg, (list, tuple)) and any(np.ndim(_trace._to_numpy(e)) > 0 for e in arg):
            return list(arg)
        a = _to_f32(arg)
        if a.ndim != 1:
            raise ValueError(f"Categorical: the class argument is a 1-D array (got shape {a.shape})")
        return [a[k] for k in range(a.shape[0])]

    def log_prob(self, value):
        if self._traced or _trace.is_symbolic(value):
            return _trace.categorical_expr(value, self._entries, self._natural)
        v = np.asarray(_trace._to_numpy(value))
        # (the reference casts the value to int32; a non-integer label is invalid
        # here, as on the device)
        vf = v.astype(np.float64)
        ok = (vf >= 0) & (vf < self.num_categories) & (vf == np.floor(vf))
        idx = np.where(ok, vf, 0).astype(np.int64)
        table = self.logits
        if table.ndim == 1:
            lp = table[idx]
        else:
            shape = np.broadcast_shapes(table.shape[:-1], idx.shape)
            lp = np.take_along_axis(np.broadcast_to(table, shape + table.shape[-1:]),
                                    np.broadcast_to(idx, shape)[..., None], axis=-1)[..., 0]
        return np.where(ok, lp, -np.inf).astype(np.float32)

    def _concrete_probs(self, what):
        if self._traced or self.probs.ndim != 1:
            raise ValueError(f"Categorical.{what} needs one concrete probability vector [K]")
        return self.probs

    def sample(self, key, shape=()):
        """The reference's rule: the number of cumulative probabilities that a
        uniform exceeds, on the engine's Philox uniforms."""
        cum = np.cumsum(self._concrete_probs("sample"), dtype=np.float32)
        u = _gpu_uniforms(key, shape)
        return np.sum(u[..., None] > cum, axis=-1).astype(np.int32)

    def entropy(self):
        p = self._concrete_probs("entropy")
        with np.errstate(divide="ignore"):
            lp = np.where(p > 0, np.log(p), np.float32(0))
        return np.float32(-np.sum(p * lp, dtype=np.float32))

    def mode(self):
        return int(np.argmax(self._concrete_probs("mode")))

    def __repr__(self):
        return f"Categorical(num_categories={self.num_categories})"


def _gpu_student_t_log_prob(df: float, half: bool, value, loc, scale) -> np.ndarray:
    """The Student-t node's value on concrete arguments (mc_student_t_log_prob)
    plus the f32 normaliser, added in f32 as the traced ADD node adds it."""
    import torch

    dev = _lib.require_device()
    v, s = _to_f32(value), _to_f32(scale)
    m = None if half else _to_f32(loc)
    shapes = [a.shape for a in (v, m, s) if a is not None]
    out_shape = np.broadcast_shapes(*shapes)
    n = int(np.prod(out_shape)) if out_shape else 1

    def dev_arr(a):
        if a is None:
            return None, 1
        if a.size == 1:
            return torch.from_numpy(a.reshape(1).copy()).to(dev), 1
        return torch.from_numpy(np.broadcast_to(a, out_shape).reshape(-1).copy()).to(dev), 0

    tv, bv = dev_arr(v)
    tm, bm = dev_arr(m)
    ts, bs = dev_arr(s)
    out = torch.empty(n, dtype=torch.float32, device=dev)
    _lib.check(_lib.load().mc_student_t_log_prob(df, int(half), n, _lib.ptr(tv), bv, _lib.ptr(tm),
                                                 bm, _lib.ptr(ts), bs, _lib.ptr(out),
                                                 _lib.stream_handle()))
    core = out.cpu().numpy().reshape(out_shape)
    with np.errstate(invalid="ignore"):
        return (core + _trace.student_t_norm(df, half)).astype(np.float32)


class StudentT(Distribution):
    """StudentT(df, loc=0.0, scale=1.0): the location-scale Student-t,

      log p(x) = lgamma((df + 1) / 2) - lgamma(df / 2) - log(df pi) / 2 - log(scale)
                 - (df + 1) / 2 * log1p(((x - loc) / scale)^2 / df)

    df is a constant — one finite positive number (ValueError otherwise; a
    traced df is a TraceError: its normaliser would need an lgamma node with a
    digamma VJP); value, loc and scale may each be traced, data or constants.
    Traced, ``log_prob`` records ADD(MC_EX_STUDENT_T_LP, normaliser): three
    nodes beside its arguments (_trace.student_t_expr)."""

    _half = False

    def __init__(self, df, loc=0.0, scale=1.0):
        self.df = _trace.student_t_df(type(self).__name__, df)
        self.loc = loc
        self.scale = scale

    def log_prob(self, value):
        name = type(self).__name__
        if _trace.is_symbolic(value, self.loc, self.scale):
            return _trace.student_t_expr(name, self.df, value, self.loc, self.scale, self._half)
        return _gpu_student_t_log_prob(self.df, self._half, value, self.loc, self.scale)

    def _standard(self, key, shape):
        """Standard t draws on the host (NumPy seeded from the key, as Gamma's)."""
        return _host_rng(key).standard_t(self.df, size=shape or None)

    def sample(self, key, shape=()):
        t = self._standard(key, shape)
        return (_to_f32(self.loc) + _to_f32(self.scale) * t).astype(np.float32)

    def mean(self):
        loc = _to_f32(self.loc)
        return loc if self.df > 1.0 else np.full_like(loc, np.nan)

    def variance(self):
        s2 = _to_f32(self.scale) ** 2
        if self.df > 2.0:
            return (s2 * np.float32(self.df / (self.df - 2.0))).astype(np.float32)
        return np.full_like(s2, np.inf if self.df > 1.0 else np.nan)

    def mode(self):
        return _to_f32(self.loc)

    def __repr__(self):
        return (f"StudentT(df={self.df:.3f}, loc={_scalar_repr(self.loc)}, "
                f"scale={_scalar_repr(self.scale)})")


class Cauchy(StudentT):
    """Cauchy(loc=0.0, scale=1.0): StudentT with df = 1."""

    def __init__(self, loc=0.0, scale=1.0):
        super().__init__(1.0, loc, scale)

    def __repr__(self):
        return f"Cauchy(loc={_scalar_repr(self.loc)}, scale={_scalar_repr(self.scale)})"


class HalfStudentT(StudentT):
    """HalfStudentT(df, scale=1.0): |T| for T ~ StudentT(df, 0, scale) — twice
    its density on x >= 0, -inf below (MC_EX_HALF_STUDENT_T_LP; HalfNormal's
    convention at the edge)."""

    _half = True

    def __init__(self, df, scale=1.0):
        super().__init__(df, 0.0, scale)

    def sample(self, key, shape=()):
        return np.abs(_to_f32(self.scale) * self._standard(key, shape)).astype(np.float32)

    def mean(self):
        # E|T| = 2 sqrt(df) Gamma((df + 1) / 2) / ((df - 1) sqrt(pi) Gamma(df / 2))
        import math

        s = _to_f32(self.scale)
        if not self.df > 1.0:
            return np.full_like(s, np.inf)
        nu = self.df
        c = (2.0 * math.sqrt(nu) / ((nu - 1.0) * math.sqrt(math.pi))
             * math.exp(math.lgamma(0.5 * (nu + 1.0)) - math.lgamma(0.5 * nu)))
        return (s * np.float32(c)).astype(np.float32)

    def variance(self):
        s2 = _to_f32(self.scale) ** 2
        if not self.df > 2.0:
            return np.full_like(s2, np.inf if self.df > 1.0 else np.nan)
        nu = self.df
        m = self.mean().astype(np.float64)
        return (s2 * (nu / (nu - 2.0)) - m * m).astype(np.float32)

    def mode(self):
        return np.zeros_like(_to_f32(self.scale))

    def __repr__(self):
        return f"HalfStudentT(df={self.df:.3f}, scale={_scalar_repr(self.scale)})"


class HalfCauchy(HalfStudentT):
    """HalfCauchy(scale=1.0): HalfStudentT with df = 1."""

    def __init__(self, scale=1.0):
        super().__init__(1.0, scale)

    def __repr__(self):
        return f"HalfCauchy(scale={_scalar_repr(self.scale)})"


__all__ = ["Distribution", "Normal", "HalfNormal", "Exponential", "Gamma", "Beta", "Bernoulli",
           "Binomial", "Poisson", "Categorical", "StudentT", "Cauchy", "HalfStudentT",
           "HalfCauchy", "Key"]
