"""Design-matrix GLM forms beyond tests/_glm.py's (a parameter intercept, beta
right after it, exp(log_sigma), weight-1 Normal priors): a form is a plain
record, one factory writes its log density against a namespace (the product's,
the oracle's float32 torch one, or a float64 torch one for autograd), and one
closed form gives the log density and gradient in NumPy at a chosen precision."""
import math
from types import SimpleNamespace

import numpy as np

import _glm

A_CONST, SIGMA_CONST, LEAD = 0.25, 0.75, 2  # (exact in f32); elements of w before beta


def _form(family, shapes, beta, icpt=None, scale=None, offset=False, priors=(), domain=None):
    """shapes: {name: shape} in layout order; beta: (name, first element); icpt:
    None, a constant or a parameter's name; scale (normal): a constant, ("exp",
    name) or ("raw", name); offset: add the data's offset vector; priors: (dist,
    args, name, slice or None, transform of the value, weight); domain: {name:
    "pos" | "unit" | "gt1"} for the test points (default: the real line)."""
    return SimpleNamespace(family=family, shapes=shapes, beta=beta, icpt=icpt, scale=scale,
                           offset=offset, priors=list(priors), domain=domain or {})


def _pr(dist, args, name, sl=None, xf="none", w=1.0):
    return (dist, tuple(args), name, sl, xf, w)


FORMS = {
    "normal": ("bare", "const", "sliced", "rawscale", "priors_a", "priors_b"),
    "bernoulli": ("bare", "const", "sliced", "priors_a", "priors_b"),
    "poisson": ("bare", "const", "const_nooff", "sliced", "priors_a", "priors_b"),
}
CASES = [(fam, name) for fam in _glm.FAMILIES for name in FORMS[fam]]


def form(name, family, P):
    nrm = family == "normal"
    if name == "plain":   # tests/_glm.py's own form
        sh = {"a": (), "beta": (P,)}
        pri = [_pr("Normal", (0.0, _glm.SIGMA_A), "a"), _pr("Normal", (0.0, _glm.SIGMA_B), "beta")]
        if nrm:
            sh["log_sigma"] = ()
            pri.append(_pr("Normal", (0.0, 1.0), "log_sigma"))
        return _form(family, sh, ("beta", 0), "a", ("exp", "log_sigma") if nrm else None,
                     family == "poisson", pri)
    if name == "bare":
        return _form(family, {"beta": (P,)}, ("beta", 0), None, SIGMA_CONST if nrm else None,
                     False, [_pr("Normal", (0.0, 2.0), "beta")])
    if name in ("const", "const_nooff"):
        return _form(family, {"beta": (P,)}, ("beta", 0), A_CONST, SIGMA_CONST if nrm else None,
                     name == "const", [_pr("Normal", (0.0, 2.0), "beta")])
    if name == "sliced":  # u: in no term
        sh = {"w": (P + LEAD + 1,), "a": (), "u": ()}
        pri = [_pr("Normal", (0.0, 2.0), "w", (LEAD, LEAD + P)),
               _pr("Normal", (0.5, 1.5), "w", (0, LEAD)),
               _pr("Normal", (0.5, 1.5), "w", (LEAD + P, LEAD + P + 1)),
               _pr("Normal", (0.0, 5.0), "a")]
        if nrm:
            sh["log_sigma"] = ()
            pri.append(_pr("Normal", (0.0, 1.0), "log_sigma"))
        return _form(family, sh, ("w", LEAD), "a", ("exp", "log_sigma") if nrm else None,
                     family == "poisson", pri)
    if name == "rawscale":
        return _form(family, {"a": (), "beta": (P,), "s": ()}, ("beta", 0), "a", ("raw", "s"),
                     False, [_pr("Normal", (0.0, 5.0), "a"), _pr("Normal", (0.0, 2.0), "beta"),
                      _pr("HalfNormal", (1.0,), "s")], {"s": "pos"})
    if name == "priors_a":
        # HalfNormal and Gamma on mx.exp of a parameter with the Jacobian's identity
        # term; Beta; a weighted Normal on beta[1:3] over the one on all of beta
        return _form(family, {"a": (), "beta": (P,), "t": (), "g": (2,), "b": ()}, ("beta", 0), "a",
                     ("exp", "t") if nrm else None, family == "poisson",
                     [_pr("Normal", (0.0, 5.0), "a"), _pr("Normal", (0.0, 2.0), "beta"),
                      _pr("Normal", (0.5, 1.0), "beta", (1, 3), w=0.5),
                      _pr("HalfNormal", (1.5,), "t", xf="exp"), _pr("Identity", (), "t"),
                      _pr("Gamma", (2.5, 1.5), "g", xf="exp"), _pr("Identity", (), "g"),
                      _pr("Beta", (2.0, 3.0), "b")], {"b": "unit"})
    if name == "priors_b":
        # Exponential; Gamma on mx.log of a parameter with -log as its Jacobian; a
        # Normal of weight 2; HalfNormal on the (positive) intercept; Exponential
        # and Beta overlapping on beta[0]
        return _form(family, {"beta": (P,), "r": (), "e": (2,), "a": ()}, ("beta", 0), "a",
                     ("raw", "r") if nrm else None, False,
                     [_pr("Normal", (0.0, 2.0), "beta", (1, P), w=2.0),
                      _pr("Exponential", (0.7,), "beta", (0, 1)),
                      _pr("Beta", (1.5, 2.5), "beta", (0, 1), w=0.25),
                      _pr("Exponential", (0.7,), "r"),
                      _pr("Gamma", (3.0, 2.0), "e", xf="log"),
                      _pr("Identity", (), "e", xf="log", w=-1.0),
                      _pr("HalfNormal", (2.0,), "a")],
                     {"r": "pos", "e": "gt1", "a": "pos", ("beta", 0): "unit"})
    raise KeyError(name)


def data(family, N, P, seed=0):
    """_glm.data with an offset vector on every family."""
    d = _glm.data(family, N, P, seed)
    if d.off is None:
        d.off = np.random.default_rng(77 + N + P).normal(0.0, 0.3, N).astype(np.float32)
    return d


def layout(f):
    """{name: (offset, size)} and D."""
    out, o = {}, 0
    for k, s in f.shapes.items():
        out[k] = (o, int(np.prod(s, dtype=np.int64)))
        o += out[k][1]
    return out, o


def init(f):
    """Initial parameters inside every prior's support."""
    val = {"pos": 1.0, "unit": 0.5, "gt1": 2.0}
    out = {}
    for k, s in f.shapes.items():
        v = np.full(s, val.get(f.domain.get(k), 0.0), np.float32)
        for key, dom in f.domain.items():
            if isinstance(key, tuple) and key[0] == k:
                v[key[1]] = val[dom]
        out[k] = v if s else np.float32(v)
    return out


def points(f, C, seed=5):
    """q [C, D] float32: standard normal, or inside the support the form names."""
    lay, D = layout(f)
    rng = np.random.default_rng(seed)
    q = rng.normal(size=(C, D))
    draw = {"pos": lambda n: rng.uniform(0.3, 3.0, (C, n)),
            "unit": lambda n: rng.uniform(0.1, 0.9, (C, n)),
            "gt1": lambda n: rng.uniform(1.2, 3.0, (C, n))}
    for key, dom in f.domain.items():
        if isinstance(key, tuple):
            o = lay[key[0]][0] + key[1]
            q[:, o:o + 1] = draw[dom](1)
        else:
            o, n = lay[key]
            q[:, o:o + n] = draw[dom](n)
    return q.astype(np.float32)


def ns_product():
    import mlx_mcmc_amd as m
    import mlx_mcmc_amd.core as mx
    ns = _glm.ns_product()
    ns.HalfNormal, ns.Exponential, ns.Gamma, ns.Beta, ns.log = (m.HalfNormal, m.Exponential,
                                                                m.Gamma, m.Beta, mx.log)
    return ns


def ns_torch():
    """The oracle's float32 namespace (oracle.samplers differentiates it)."""
    from oracle import ns as o
    ns = _glm.ns_torch()
    ns.HalfNormal, ns.Exponential, ns.Gamma, ns.Beta, ns.log = (o.HalfNormal, o.Exponential,
                                                                o.Gamma, o.Beta, o.log)
    return ns


def ns_torch64():
    """The same calls in float64 torch, for autograd as the reference of
    closed_form (the oracle's namespace rounds its constants to float32)."""
    import torch

    def T(x):
        return x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x, np.float64))

    def dist(logpdf):
        class Dist:
            def __init__(self, *args, **kw):
                self.args = [T(a) for a in args] + [T(a) for a in kw.values()]

            def log_prob(self, v):
                return logpdf(T(v), *self.args)
        return Dist

    ln2pi = math.log(2 * math.pi)
    lg = torch.lgamma

    def normal(v, m, s):
        return -0.5 * ln2pi - torch.log(s) - 0.5 * ((v - m) / s) ** 2

    return SimpleNamespace(
        Normal=dist(normal),
        HalfNormal=dist(lambda v, s: math.log(2.0) + normal(v, T(0.0), s)),
        Exponential=dist(lambda v, r: torch.log(r) - r * v),
        Gamma=dist(lambda v, a, b: a * torch.log(b) - lg(a) + (a - 1) * torch.log(v) - b * v),
        Beta=dist(lambda v, a, b: (a - 1) * torch.log(v) + (b - 1) * torch.log(1 - v)
                  - (lg(a) + lg(b) - lg(a + b))),
        Bernoulli=dist(lambda y, eta: -torch.nn.functional.softplus(
            torch.where(y != 0, -eta, eta), threshold=700.0)),
        Poisson=dist(lambda y, eta: y * eta - torch.exp(eta) - lg(y + 1.0)),
        sum=lambda x: torch.sum(T(x)), exp=lambda x: torch.exp(T(x)), log=lambda x: torch.log(T(x)),
        array=T)


def model(ns, f, d):
    """log_prob(params), init of the form f on the data d."""
    bname, b0 = f.beta

    def log_prob(p):
        def part(name, sl):
            return p[name] if sl is None else p[name][sl[0]:sl[1]]

        eta = ns.array(d.X) @ part(bname, None if f.shapes[bname] == (d.P,) else (b0, b0 + d.P))
        if isinstance(f.icpt, str):
            eta = eta + p[f.icpt]
        elif f.icpt is not None:
            eta = eta + f.icpt
        if f.offset:
            eta = eta + ns.array(d.off)
        if f.family == "normal":
            s = f.scale if not isinstance(f.scale, tuple) else (
                ns.exp(p[f.scale[1]]) if f.scale[0] == "exp" else p[f.scale[1]])
            lp = ns.sum(ns.Normal(eta, s).log_prob(ns.array(d.y)))
        elif f.family == "bernoulli":
            lp = ns.sum(ns.Bernoulli(logits=eta).log_prob(d.y))
        else:
            lp = ns.sum(ns.Poisson(log_rate=eta).log_prob(d.y))
        for dist, args, name, sl, xf, w in f.priors:
            v = part(name, sl)
            v = ns.exp(v) if xf == "exp" else ns.log(v) if xf == "log" else v
            t = v if dist == "Identity" else getattr(ns, dist)(*args).log_prob(v)
            if f.shapes[name] != ():
                t = ns.sum(t)
            lp = lp + (t if w == 1.0 else w * t)
        return lp

    return log_prob, init(f)


def closed_form(f, d, q, dt=np.float64):
    """(log p [C], gradient [C, D]) of the form f at the points q [C, D], every
    operation in `dt`.  An observation outside its family's support gives log p
    = -inf and no residual, as the kernels do."""
    q = np.asarray(q, dt)
    lay, D = layout(f)
    assert q.shape[1] == D
    X, y = d.X.astype(dt), d.y.astype(dt)
    half, one, ln2pi = dt(0.5), dt(1), dt(math.log(2 * math.pi))
    b0 = lay[f.beta[0]][0] + f.beta[1]
    eta = q[:, b0:b0 + d.P] @ X.T
    if isinstance(f.icpt, str):
        eta = eta + q[:, lay[f.icpt][0], None]
    elif f.icpt is not None:
        eta = eta + dt(f.icpt)
    if f.offset:
        eta = eta + d.off.astype(dt)
    g = np.zeros_like(q)
    with np.errstate(all="ignore"):
        if f.family == "normal":
            if isinstance(f.scale, tuple):
                so = lay[f.scale[1]][0]
                s = np.exp(q[:, so, None]) if f.scale[0] == "exp" else q[:, so, None]
            else:
                s = np.full((q.shape[0], 1), f.scale, dt)
            z = (y - eta) / s
            ll = -half * ln2pi - np.log(s) - half * z * z
            r = z / s
            if isinstance(f.scale, tuple):
                ds = ((z * z - one) / s).sum(1)
                g[:, so] += ds * s[:, 0] if f.scale[0] == "exp" else ds
        elif f.family == "bernoulli":
            ok = (d.y == 0) | (d.y == 1)
            ll = np.where(ok, -np.logaddexp(dt(0), np.where(y != 0, -eta, eta)), -np.inf).astype(dt)
            r = np.where(ok, y - one / (one + np.exp(-eta)), dt(0))
        else:
            ok = (d.y >= 0) & (d.y == np.floor(d.y))
            lgam = np.array([math.lgamma(v + 1.0) if k else 0.0 for v, k in zip(d.y, ok)], dt)
            ll = np.where(ok, y * eta - np.exp(eta) - lgam, -np.inf).astype(dt)
            r = np.where(ok, y - np.exp(eta), dt(0))
    lp = ll.sum(1)
    g[:, b0:b0 + d.P] += r @ X
    if isinstance(f.icpt, str):
        g[:, lay[f.icpt][0]] += r.sum(1)

    def normal(v, m, s):
        z = (v - dt(m)) / dt(s)
        return -half * ln2pi - np.log(dt(s)) - half * z ** 2, -z / dt(s)

    for dist, args, name, sl, xf, w in f.priors:
        o, n = lay[name]
        if sl is not None:
            o, n = o + sl[0], sl[1] - sl[0]
        x = q[:, o:o + n]
        v, dv = x, np.ones_like(x)
        if xf != "none":
            v, dv = (np.exp(x), np.exp(x)) if xf == "exp" else (np.log(x), one / x)
        a = [dt(t) for t in args]
        if dist == "Normal":
            l, dl = normal(v, *args)
        elif dist == "HalfNormal":
            l, dl = normal(v, 0.0, args[0])
            l = l + dt(math.log(2.0))
        elif dist == "Exponential":
            l, dl = np.log(a[0]) - a[0] * v, np.full_like(v, -a[0])
        elif dist == "Gamma":
            l = a[0] * np.log(a[1]) - dt(math.lgamma(args[0])) + (a[0] - one) * np.log(v) - a[1] * v
            dl = (a[0] - one) / v - a[1]
        elif dist == "Beta":
            lb = dt(math.lgamma(args[0]) + math.lgamma(args[1]) - math.lgamma(args[0] + args[1]))
            l = (a[0] - one) * np.log(v) + (a[1] - one) * np.log(one - v) - lb
            dl = (a[0] - one) / v - (a[1] - one) / (one - v)
        else:
            l, dl = v, np.ones_like(v)
        lp = lp + dt(w) * l.sum(1)
        g[:, o:o + n] += dt(w) * dl * dv
    return lp, g


# ---- the gate of tests/test_gpu_glm.py, and the inputs of tests/test_gpu_glm_forms.py
# (tests/test_glm_forms_reference.py holds the float32 closed form to the same gate
# at every one of them) --------------------------------------------------------------
SHAPES = [(33, 3, 5, 1), (97, 33, 33, 3)]  # (N, P, C, S)
WIDE = (33, 129, 5, 1)


def gate_fractions(lp, g, rlp, rg):
    """(worst |lp - ref| over its bound 1e-5 max(1, |ref|), worst gradient error
    over its bound 2e-5 max(1, max |g|) + 2e-4 |ref|)."""
    flp = np.abs(lp - rlp) / (1e-5 * np.maximum(1.0, np.abs(rlp)))
    fg = np.abs(g - rg) / (2e-5 * max(1.0, np.abs(rg).max()) + 2e-4 * np.abs(rg))
    return float(flp.max()), float(fg.max())


def assert_gate(lp, g, rlp, rg, what=""):
    err = np.abs(lp - rlp) / np.maximum(1.0, np.abs(rlp))
    flp, fg = gate_fractions(lp, g, rlp, rg)
    print(f"{what}: lp {flp:.3f} of the bound, gradient {fg:.3f} (max |g| {np.abs(rg).max():.2e})")
    assert np.all(err <= 1e-5)
    np.testing.assert_allclose(g, rg, rtol=2e-4, atol=2e-5 * max(1.0, np.abs(rg).max()))


SATURATION = [("bernoulli", 100.0), ("poisson", 20.0), ("poisson", 10.0), ("poisson", 5.0),
              ("exp", -4.0), ("exp", 4.0), ("raw", 0.05), ("raw", 20.0)]


def saturated(kind, level, N, P, C):
    """(form, data, q): Bernoulli / Poisson with the intercept and coefficients
    scaled until max |a + X beta| (Poisson: max a + X beta, the side on which
    exp grows) is `level`; Normal with log_sigma (kind "exp")
    or the raw scale (kind "raw") set to `level` on every chain."""
    if kind in ("bernoulli", "poisson"):
        f, d = form("plain", kind, P), _glm.data(kind, N, P)
        q = points(f, C).astype(np.float64)
        eta = q[:, :1] + q[:, 1:1 + P] @ d.X.astype(np.float64).T
        top = np.abs(eta).max() if kind == "bernoulli" else eta.max()
        return f, d, (q * (level / top)).astype(np.float32)
    f = form("plain" if kind == "exp" else "rawscale", "normal", P)
    d = _glm.data("normal", N, P)
    q = points(f, C)
    q[:, -1] = level
    return f, d, q
