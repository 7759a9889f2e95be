#!/usr/bin/env python3
"""Throughput of the design-matrix GLM kernels (csrc/glm.h).

    python scripts/bench_glm.py [--n 100000] [--chains 256] [--L 20] [--p 16 64 256]
        [--reps 7] [--out FILE.json]

Logistic regression y ~ Bernoulli(logits = a + X beta), per P:
 a  mc_logp_grad of `--chains` points (one k_glm_grad launch and its reduce), by
    device events;
 b  the f32 torch statement eta = X @ B; R = y - sigmoid(eta); G = X.T @ R at the
    same shapes; a and b alternate inside this one call after a warm-up, `--reps`
    times each, and the spread is reported;
 c  chain-leapfrog-steps/s of mc_hmc_run end to end (device events around the
    launches of a block of iterations), and the share of that time not covered
    by L gradient evaluations of (a): launch gaps and the step kernels;
 d  at P = 2 also the lane-resident expression route on
    workloads.two_predictor_regression at the same N, the one older path that
    can state such a model.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(fn):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return float(a.elapsed_time(b))


def _spread(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def logistic(N, P, seed=1):
    import mlx_mcmc_amd as m
    import mlx_mcmc_amd.core as mx

    rng = np.random.default_rng(seed)
    X = (rng.normal(size=(N, P)) / np.sqrt(P)).astype(np.float32)
    y = (rng.random(N) < 1 / (1 + np.exp(-(X @ rng.normal(size=P))))).astype(np.float32)

    def lp(p):
        return (mx.sum(m.Bernoulli(logits=p["a"] + X @ p["beta"]).log_prob(y))
                + mx.sum(m.Normal(0.0, 2.0).log_prob(p["beta"])) + m.Normal(0.0, 5.0).log_prob(p["a"]))
    return lp, {"a": np.float32(0.0), "beta": np.zeros(P, np.float32)}, X, y


class Hmc:
    """Blocks of `iters` iterations of mc_hmc_run at a fixed step size."""

    def __init__(self, lp, init, chains, L, iters=5, eps=1e-3):
        import torch

        from mlx_mcmc_amd import _engine, _trace

        self.prog = _trace.compile_model(lp, init)
        self.cs = _engine.ChainSet(self.prog, chains, self.prog.layout.flatten(init), eps)
        self.samples = torch.empty((chains, 1, self.prog.D), dtype=torch.float32, device="cuda")
        self.cfg = dict(chain_offset=0, num_warmup=10 ** 6, num_samples=1, sample_begin=0,
                        sample_capacity=1, seed=0, step_size=eps, target_accept=0.8,
                        num_leapfrog_steps=L, adapt_step_size=False)
        self.chains, self.L, self.iters, self.at = chains, L, iters, 0
        self.once()

    def once(self):
        ms = _timed(lambda: self.cs.run_hmc(samples=self.samples, iter_begin=self.at,
                                            iter_count=self.iters, **self.cfg))
        self.at += self.iters
        return ms

    def rate(self, ms):
        return self.chains * self.L * self.iters / (ms * 1e-3)


def bench_p(N, P, C, L, reps):
    import torch

    from mlx_mcmc_amd import _engine

    lp, init, X, y = logistic(N, P)
    run = Hmc(lp, init, C, L)
    q = torch.randn(C, run.prog.D, device="cuda")
    Xd, yd = torch.as_tensor(X).cuda(), torch.as_tensor(y).cuda()[:, None]
    B = torch.randn(P, C, device="cuda")

    def ours():
        _engine.logp_grad(run.prog, q)

    def stmt():
        R = yd - torch.sigmoid(Xd @ B)
        return Xd.T @ R

    for f in (ours, stmt):
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    t_ours, t_stmt, t_hmc = [], [], []
    for _ in range(reps):
        t_ours.append(_timed(ours))
        t_stmt.append(_timed(stmt))
        t_hmc.append(run.once())
    g = float(np.median(t_ours))
    it = float(np.median(t_hmc)) / run.iters
    return {"P": P, "N": N, "chains": C, "L": L, "slices": run.prog.glm_slices(C),
            "logp_grad": _spread(t_ours), "torch_statement": _spread(t_stmt),
            "hmc_block": _spread(t_hmc), "hmc_steps_per_s": run.rate(float(np.median(t_hmc))),
            "hmc_us_per_leapfrog": 1e3 * it / L,
            # (negative: the call-level time of (a), with its reduce and host work,
            # exceeds a leapfrog step of the stream — the share cannot be formed)
            "share_outside_gradients": 1.0 - L * g / it}


def bench_p2(N, C, L, reps):
    """P = 2: the GLM route and the expression route on the same data."""
    import mlx_mcmc_amd as m
    import mlx_mcmc_amd.core as mx
    import workloads as W

    x1, x2, y = W.two_predictor_data(N)
    X = np.stack([x1, x2], 1)

    def glm(p):
        s = mx.exp(p["log_sigma"])
        lp = m.Normal(0, 10).log_prob(p["a"]) + mx.sum(m.Normal(0, 10).log_prob(p["b"]))
        lp = lp + m.HalfNormal(5).log_prob(s) + p["log_sigma"]
        return lp + mx.sum(m.Normal(p["a"] + X @ p["b"], s).log_prob(y))

    old_lp, old_init = W.two_predictor_regression(W.ns_product(), N)
    runs = {"glm": Hmc(glm, {"a": np.float32(0), "b": np.zeros(2, np.float32),
                             "log_sigma": np.float32(0)}, C, L),
            "expression": Hmc(old_lp, old_init, C, L)}
    ms = {k: [] for k in runs}
    for _ in range(reps):
        for k, r in runs.items():
            ms[k].append(r.once())
    return {k: {"kernel": runs[k].prog.slice_kernel, **_spread(v),
                "hmc_steps_per_s": runs[k].rate(float(np.median(v)))} for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--chains", type=int, default=256)
    ap.add_argument("--L", type=int, default=20)
    ap.add_argument("--p", type=int, nargs="*", default=[16, 64, 256])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_glm.py measures on the GPU: no device is visible")
    out = {"rows": [bench_p(a.n, P, a.chains, a.L, a.reps) for P in a.p],
           "p2": bench_p2(a.n, a.chains, a.L, a.reps)}
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
