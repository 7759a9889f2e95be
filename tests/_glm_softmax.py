"""Softmax regression on a design matrix: the test model written against a
namespace (the product's, or an eager torch one for oracle.samplers) and the
closed-form log density and gradient in NumPy at a chosen precision."""
import math
from types import SimpleNamespace

import numpy as np

SIGMA_B, SIGMA_A = 2.0, 5.0  # prior scales of B and the class intercepts


def data(N, P, K, seed=0):
    """X ~ N(0, 1) / sqrt(P), as _glm.data; labels drawn from the softmax at a
    random B."""
    rng = np.random.default_rng(1000 * seed + 7 * N + 31 * P + K)
    X = (rng.normal(size=(N, P)) / math.sqrt(P)).astype(np.float32)
    eta = X.astype(np.float64) @ (2.0 * rng.normal(size=(P, K)))
    pr = np.exp(eta - eta.max(1, keepdims=True))
    cum = np.cumsum(pr / pr.sum(1, keepdims=True), axis=1)
    y = np.minimum((rng.random((N, 1)) > cum).sum(1), K - 1)
    return SimpleNamespace(N=N, P=P, K=K, X=X, y=y.astype(np.int64))


def ns_product():
    import mlx_mcmc_amd as m
    import mlx_mcmc_amd.core as mx
    return SimpleNamespace(Normal=m.Normal, Categorical=m.Categorical, sum=mx.sum, array=mx.array)


def ns_torch():
    """The same calls on float32 torch tensors (autograd differentiates them)."""
    import torch
    from oracle import ns

    class Categorical:
        def __init__(self, logits):
            self.logits = logits

        def log_prob(self, y):
            idx = torch.as_tensor(np.asarray(y), dtype=torch.int64)[:, None]
            return torch.log_softmax(self.logits, dim=1).gather(1, idx)[:, 0]

    return SimpleNamespace(Normal=ns.Normal, Categorical=Categorical, sum=ns.sum, array=ns.array)


def model(ns, d, intercept=True):
    """log_prob(params), init: coefficients B [P, K] and (intercept) the class
    intercepts a [K], under Normal priors."""
    def log_prob(p):
        eta = ns.array(d.X) @ p["B"]
        lp = ns.sum(ns.Normal(0.0, SIGMA_B).log_prob(p["B"]))
        if intercept:
            eta = eta + p["a"]
            lp = lp + ns.sum(ns.Normal(0.0, SIGMA_A).log_prob(p["a"]))
        return lp + ns.sum(ns.Categorical(logits=eta).log_prob(d.y))

    init = {"B": np.zeros((d.P, d.K), np.float32)}
    if intercept:
        init["a"] = np.zeros(d.K, np.float32)
    return log_prob, init


def closed_form(d, q, intercept=True, dt=np.float64):
    """(log p [C], gradient [C, D]) at the points q [C, D] = (B row-major, a),
    every operation in `dt`."""
    q = np.asarray(q, dt)
    C, PK = q.shape[0], d.P * d.K
    X = d.X.astype(dt)
    B = q[:, :PK].reshape(C, d.P, d.K)
    eta = np.einsum("np,cpk->cnk", X, B)
    if intercept:
        eta = eta + q[:, None, PK:]
    m = eta.max(2, keepdims=True)
    ll = eta - (m + np.log(np.exp(eta - m).sum(2, keepdims=True)))
    onehot = (d.y[:, None] == np.arange(d.K)[None, :]).astype(dt)
    r = onehot[None] - np.exp(ll)
    ln2pi = dt(math.log(2 * math.pi))

    def normal(v, s):
        return -dt(0.5) * ln2pi - np.log(dt(s)) - dt(0.5) * (v / dt(s)) ** 2

    lp = (ll * onehot[None]).sum((1, 2)) + normal(q[:, :PK], SIGMA_B).sum(1)
    g = np.zeros_like(q)
    g[:, :PK] = np.einsum("np,cnk->cpk", X, r).reshape(C, PK) - q[:, :PK] / dt(SIGMA_B) ** 2
    if intercept:
        lp = lp + normal(q[:, PK:], SIGMA_A).sum(1)
        g[:, PK:] = r.sum(1) - q[:, PK:] / dt(SIGMA_A) ** 2
    return lp, g
