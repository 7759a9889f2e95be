"""Design-matrix GLM test models: one factory written against a namespace
(the product's, or an eager torch one for oracle.samplers) and the closed-form
log density and gradient in NumPy at a chosen precision."""
import math
from types import SimpleNamespace

import numpy as np

FAMILIES = ("normal", "bernoulli", "poisson")
SIGMA_B, SIGMA_A = 2.0, 5.0  # prior scales of beta and the intercept


def data(family, N, P, seed=0):
    """X ~ N(0, 1) / sqrt(P), so |eta| stays O(1); y from the family at a random
    beta; an offset for Poisson."""
    rng = np.random.default_rng(1000 * seed + 7 * N + P)
    X = (rng.normal(size=(N, P)) / math.sqrt(P)).astype(np.float32)
    eta = X.astype(np.float64) @ rng.normal(size=P) + 0.3
    off = None
    if family == "normal":
        y = eta + 0.7 * rng.normal(size=N)
    elif family == "bernoulli":
        y = rng.random(N) < 1.0 / (1.0 + np.exp(-eta))
    else:
        off = rng.normal(0.0, 0.3, N).astype(np.float32)
        y = rng.poisson(np.exp(eta + off))
    return SimpleNamespace(family=family, N=N, P=P, X=X, y=np.asarray(y, np.float32), off=off)


def ns_product():
    import mlx_mcmc_amd as m
    import mlx_mcmc_amd.core as mx
    return SimpleNamespace(Normal=m.Normal, Bernoulli=m.Bernoulli, Poisson=m.Poisson,
                           sum=mx.sum, exp=mx.exp, array=mx.array)


def ns_torch():
    """The same calls on float32 torch tensors (autograd differentiates them)."""
    import torch
    from oracle import ns

    sp = lambda x: torch.nn.functional.softplus(x, threshold=700.0)   # noqa: E731

    class Bernoulli:
        def __init__(self, logits):
            self.eta = logits

        def log_prob(self, y):
            return -sp(torch.where(ns.array(y) != 0, -self.eta, self.eta))

    class Poisson:
        def __init__(self, log_rate):
            self.eta = log_rate

        def log_prob(self, y):
            y = ns.array(y)
            return y * self.eta - torch.exp(self.eta) - torch.lgamma(y + 1.0)

    return SimpleNamespace(Normal=ns.Normal, Bernoulli=Bernoulli, Poisson=Poisson, sum=ns.sum,
                           exp=ns.exp, array=ns.array)


def model(ns, d):
    """log_prob(params), init: intercept a, coefficients beta (and log_sigma for
    the normal family) under Normal priors."""
    def log_prob(p):
        eta = p["a"] + ns.array(d.X) @ p["beta"]
        if d.off is not None:
            eta = eta + ns.array(d.off)
        lp = ns.Normal(0.0, SIGMA_A).log_prob(p["a"]) + ns.sum(
            ns.Normal(0.0, SIGMA_B).log_prob(p["beta"]))
        if d.family == "normal":
            lp = lp + ns.Normal(0.0, 1.0).log_prob(p["log_sigma"])
            return lp + ns.sum(ns.Normal(eta, ns.exp(p["log_sigma"])).log_prob(ns.array(d.y)))
        if d.family == "bernoulli":
            return lp + ns.sum(ns.Bernoulli(logits=eta).log_prob(d.y))
        return lp + ns.sum(ns.Poisson(log_rate=eta).log_prob(d.y))

    init = {"a": np.float32(0.0), "beta": np.zeros(d.P, np.float32)}
    if d.family == "normal":
        init["log_sigma"] = np.float32(0.0)
    return log_prob, init


def closed_form(d, q, dt=np.float64):
    """(log p [C], gradient [C, D]) at the points q [C, D] (a, beta, log_sigma),
    every operation in `dt`."""
    q = np.asarray(q, dt)
    X, y = d.X.astype(dt), d.y.astype(dt)
    a, beta = q[:, :1], q[:, 1:1 + d.P]
    eta = a + beta @ X.T + (d.off.astype(dt) if d.off is not None else dt(0))
    ln2pi = dt(math.log(2 * math.pi))

    def normal(v, s):
        return -dt(0.5) * ln2pi - np.log(dt(s)) - dt(0.5) * (v / dt(s)) ** 2

    lp = normal(a[:, 0], SIGMA_A) + normal(beta, SIGMA_B).sum(1)
    g = np.zeros_like(q)
    g[:, 0] = -a[:, 0] / dt(SIGMA_A) ** 2
    g[:, 1:1 + d.P] = -beta / dt(SIGMA_B) ** 2
    if d.family == "normal":
        ls = q[:, -1:]
        z = (y - eta) / np.exp(ls)
        lp = lp + normal(ls[:, 0], 1.0) + (-dt(0.5) * ln2pi - ls - dt(0.5) * z * z).sum(1)
        r = z / np.exp(ls)
        g[:, -1] = -ls[:, 0] + (z * z - dt(1)).sum(1)
    elif d.family == "bernoulli":
        lp = lp + (-np.logaddexp(dt(0), np.where(y != 0, -eta, eta))).sum(1)
        r = y - dt(1) / (dt(1) + np.exp(-eta))
    else:
        lgam = np.array([math.lgamma(v + 1.0) for v in d.y], dt)
        lp = lp + (y * eta - np.exp(eta) - lgam).sum(1)
        r = y - np.exp(eta)
    g[:, 0] += r.sum(1)
    g[:, 1:1 + d.P] += r @ X
    return lp, g
