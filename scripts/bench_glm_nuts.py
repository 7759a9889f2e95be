#!/usr/bin/env python3
"""Leaf rate of nuts(nuts_kernel="glm") (csrc/glm_nuts.h) against hmc() on the
same design-matrix program.

    python scripts/bench_glm_nuts.py [--n 100000] [--chains 256] [--p 2 16 64 256]
        [--families bernoulli poisson] [--warmup 10] [--samples 40] [--depth 6]
        [--leapfrog 16] [--reps 3] [--batch T] [--out FILE.json]

Per family and P, at a fixed step size 0.5 sqrt(P / N) (about a quarter of a
coefficient's posterior scale: trees of depth 3-6):
 a  nuts(nuts_kernel="glm"): leaf-steps/s = the trace's leapfrog steps of all
    chains over the run's wall time (the entry synchronises, so wall time is
    device time plus the host's polls);
 b  hmc(num_leapfrog_steps=L) on the same program and chains: chain-leapfrog
    steps/s.  Both pay one k_glm_grad launch per step of all chains, so a / b is
    the price of the tree step, of the ticks in which a chain has nothing to do
    and of the polls.
a and b alternate `--reps` times in this process after one warm-up run each;
medians and spreads are reported.  Per run of (a): the ticks enqueued and polls
(mc_debug_glm_nuts_stats), the ticks needed (per launch window the largest
per-chain total of leaves), `tail_share` = 1 - needed / enqueued (ticks after the
last chain finished) and `idle_share` = 1 - leaves / (enqueued x chains) (chain
columns computed and ignored, tail included).  `--batch` sets T
(MC_GLM_NUTS_BATCH) for the process.  With P = 2 the same regression written
elementwise, a + b0 * x0 + b1 * x1, runs under the default nuts() (the sliced
kernel) for its leaf rate.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _spread(x):
    return {"median": float(np.median(x)), "min": float(min(x)), "max": float(max(x))}


def bench(family, N, P, a):
    import mlx_mcmc_amd as m
    import mlx_mcmc_amd.core as mx
    from mlx_mcmc_amd import _lib

    rng = np.random.default_rng(1)
    X = (rng.normal(size=(N, P)) / np.sqrt(P)).astype(np.float32)
    eta = X @ rng.normal(size=P) + 0.3
    if family == "bernoulli":
        y = (rng.random(N) < 1 / (1 + np.exp(-eta))).astype(np.float32)
        like = lambda e: m.Bernoulli(logits=e).log_prob(y)            # noqa: E731
    else:
        y = rng.poisson(np.exp(eta)).astype(np.float32)
        like = lambda e: m.Poisson(log_rate=e).log_prob(y)            # noqa: E731

    def prior(p):
        return m.Normal(0.0, 5.0).log_prob(p["a"]) + mx.sum(m.Normal(0.0, 2.0).log_prob(p["beta"]))

    def lp(p):
        return prior(p) + mx.sum(like(p["a"] + mx.array(X) @ p["beta"]))

    def lp_elementwise(p):
        return prior(p) + mx.sum(like(p["a"] + p["beta"][0] * X[:, 0] + p["beta"][1] * X[:, 1]))

    init = {"a": np.float32(0.0), "beta": np.zeros(P, np.float32)}
    eps = 0.5 * float(np.sqrt(P / N))
    W, S, C, iters = a.warmup, a.samples, a.chains, a.warmup + a.samples
    kw = dict(num_samples=S, num_warmup=W, step_size=eps, adapt_step_size=False,
              key=m.random.key(5), num_chains=C, progress=False, return_info=True,
              return_trace=True)
    lib = _lib.load()

    def nuts_run(fn, **extra):
        t, q = ctypes.c_int64(), ctypes.c_int64()
        lib.mc_debug_glm_nuts_stats(ctypes.byref(t), ctypes.byref(q))  # (reset)
        _, _, info = m.nuts(fn, init, max_tree_depth=a.depth, **kw, **extra)
        lib.mc_debug_glm_nuts_stats(ctypes.byref(t), ctypes.byref(q))
        lf = info.trace["n_leapfrog"][:, :iters].astype(np.int64)
        sec = info.warmup_seconds + info.sampling_seconds
        need = int(lf[:, :W].sum(1).max() + lf[:, W:].sum(1).max())
        return {"kernel": info.extra["kernel"], "seconds": sec, "leaves": int(lf.sum()),
                "rate": lf.sum() / sec, "ticks": t.value, "polls": q.value, "needed": need,
                "mean_depth": float(info.trace["tree_depth"][:, :iters].mean())}

    def hmc_run():
        _, _, info = m.hmc(lp, init, num_leapfrog_steps=a.leapfrog, **kw)
        assert info.extra["kernel"] == "glm"
        sec = info.warmup_seconds + info.sampling_seconds
        return {"seconds": sec, "rate": C * a.leapfrog * iters / sec,
                "slices": info.extra["glm_slices"]}

    nuts_run(lp, nuts_kernel="glm"), hmc_run()  # warm-up
    ns, hs = [], []
    for _ in range(a.reps):
        ns.append(nuts_run(lp, nuts_kernel="glm"))
        hs.append(hmc_run())
    r = ns[0]
    assert r["kernel"] == "glm"
    row = {"family": family, "N": N, "P": P, "chains": C, "iterations": iters, "step_size": eps,
           "max_tree_depth": a.depth, "mean_depth": r["mean_depth"], "glm_slices": hs[0]["slices"],
           "leaves": r["leaves"], "ticks_enqueued": r["ticks"], "polls": r["polls"],
           "ticks_needed": r["needed"], "tail_share": 1 - r["needed"] / r["ticks"],
           "idle_share": 1 - r["leaves"] / (r["ticks"] * C),
           "ms_per_tick": 1e3 * float(np.median([x["seconds"] for x in ns])) / r["ticks"],
           "nuts_leaf_steps_per_s": _spread([x["rate"] for x in ns]),
           "hmc_leapfrog_steps_per_s": _spread([x["rate"] for x in hs])}
    row["nuts_over_hmc"] = (row["nuts_leaf_steps_per_s"]["median"]
                            / row["hmc_leapfrog_steps_per_s"]["median"])
    if P == 2:
        try:
            nuts_run(lp_elementwise)
            es = [nuts_run(lp_elementwise) for _ in range(a.reps)]
            row["elementwise"] = {"kernel": es[0]["kernel"], "mean_depth": es[0]["mean_depth"],
                                  "leaf_steps_per_s": _spread([x["rate"] for x in es])}
        except Exception as e:  # (the model may not plan onto a NUTS kernel: say so)
            row["elementwise"] = {"error": f"{type(e).__name__}: {e}"[:300]}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--chains", type=int, default=256)
    ap.add_argument("--p", type=int, nargs="*", default=[2, 16, 64, 256])
    ap.add_argument("--families", nargs="*", default=["bernoulli", "poisson"])
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--samples", type=int, default=40)
    ap.add_argument("--depth", type=int, default=6)
    ap.add_argument("--leapfrog", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.batch:
        os.environ["MC_GLM_NUTS_BATCH"] = str(a.batch)
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_glm_nuts.py measures on the GPU: no device is visible")
    out = {"batch": a.batch or 32, "rows": []}
    for fam in a.families:
        for P in a.p:
            out["rows"].append(bench(fam, a.n, P, a))
            print(json.dumps(out["rows"][-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
