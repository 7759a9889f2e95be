"""Design-matrix likelihoods for tests/test_gpu_glm_pointwise.py: the product's
``log_likelihood(params)``, seeded draws, and the float64 NumPy [C, S, N]
matrix with the per-entry error bound of an f32 evaluation (in the style of
_glm.closed_form)."""
import math
from types import SimpleNamespace

import numpy as np

import _glm
from _pointwise import ATOL, RTOL

A_CONST, SIGMA_CONST, LEAD = 0.25, 0.75, 2  # (exact in f32); parameters before a sliced beta


def case(family, N, P, C, S, icpt="none", scale="const", sliced=False, offset=True, seed=0):
    """icpt: "none" / "const" / "param"; scale (normal): "const" / "exp";
    sliced: beta is w[LEAD : LEAD + P] of a longer vector (boff != 0, D > P);
    offset: keep the Poisson offset of _glm.data."""
    d = _glm.data(family, N, P, seed)
    if not offset:
        d.off = None
    shapes = {"w": (P + LEAD + 1,) if sliced else (P,)}
    if icpt == "param":
        shapes["a"] = ()
    if family == "normal" and scale == "exp":
        shapes["log_sigma"] = ()
    D = sum(int(np.prod(s)) for s in shapes.values())
    boff = LEAD if sliced else 0
    rng = np.random.default_rng(17 + seed + N + P)
    draws = (0.5 * rng.standard_normal((C, S, D))).astype(np.float32)

    def log_likelihood(p):
        ns = _glm.ns_product()
        eta = ns.array(d.X) @ (p["w"][LEAD:LEAD + P] if sliced else p["w"])
        if icpt != "none":
            eta = eta + (p["a"] if icpt == "param" else A_CONST)
        if d.off is not None:
            eta = eta + ns.array(d.off)
        if family == "normal":
            s = ns.exp(p["log_sigma"]) if scale == "exp" else SIGMA_CONST
            return ns.sum(ns.Normal(eta, s).log_prob(ns.array(d.y)))
        if family == "bernoulli":
            return ns.sum(ns.Bernoulli(logits=eta).log_prob(d.y))
        return ns.sum(ns.Poisson(log_rate=eta).log_prob(d.y))

    def ref(q):
        """(float64 matrix [C, S, N], the bound's third term [C, S, N])."""
        q = np.asarray(q, np.float64)
        X, y = d.X.astype(np.float64), d.y.astype(np.float64)
        beta = q[..., boff:boff + P]
        a = (q[..., -2 if "log_sigma" in shapes else -1, None] if icpt == "param"
             else np.float64(A_CONST if icpt == "const" else 0.0))
        off = d.off.astype(np.float64) if d.off is not None else np.zeros(N)
        eta = beta @ X.T + a + off
        A = np.abs(beta) @ np.abs(X).T + np.abs(a) + np.abs(off)
        with np.errstate(all="ignore"):
            if family == "normal":
                sg = np.exp(q[..., -1:]) if scale == "exp" else np.float64(SIGMA_CONST)
                ll = -0.5 * math.log(2 * math.pi) - np.log(sg) - 0.5 * ((y - eta) / sg) ** 2
                r = (y - eta) / sg ** 2
            elif family == "bernoulli":
                ll = -np.logaddexp(0.0, np.where(y != 0, -eta, eta))
                r = y - 1.0 / (1.0 + np.exp(-eta))
            else:
                ok = (y >= 0) & (y == np.floor(y))
                lg = np.array([math.lgamma(v + 1.0) if k else 0.0 for v, k in zip(y, ok)])
                ll = np.where(ok, y * eta - np.exp(eta) - lg, -np.inf)
                r = y - np.exp(eta)
        return ll, 2.0 * (P + 4) * 2.0 ** -24 * np.abs(r) * A

    return SimpleNamespace(d=d, family=family, N=N, P=P, shapes=shapes, draws=draws,
                           log_likelihood=log_likelihood, ref=ref)


def entry_bound(ref, third):
    """ATOL + RTOL |ref| + the dot product's share, per entry."""
    with np.errstate(invalid="ignore"):
        return ATOL + RTOL * np.abs(ref) + third


def layout_of(c):
    from mlx_mcmc_amd import _trace

    return _trace.layout_of({k: np.zeros(s, np.float32) for k, s in c.shapes.items()})
