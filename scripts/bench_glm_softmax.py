#!/usr/bin/env python3
"""Time of softmax regression on the class-packed MFMA gradient kernel
(csrc/glm_softmax.h) against a dense torch statement of the same gradient, and
of the packed program with K = 2 against the Bernoulli-logit program on the same
X (what the cross-lane softmax and the halved chains per block cost).

    python scripts/bench_glm_softmax.py [--n 100000] [--p 16 64 256] [--k 4 8 32]
        [--chains 256] [--reps 5] [--out FILE.json]

The model is Categorical(logits=X @ B + a) with Normal priors: X ~ N(0, 1) /
sqrt(P) in f32, labels from the softmax at a random B.  HMC iterations run
through ChainSet.run_hmc with L = 1 and L = 9 leapfrog steps; a leapfrog step is
one gradient launch and one step launch, so (t9 - t1) / 8 is the time of that
pair ("leapfrog_ms") and t9 the time of an iteration at L = 9 ("hmc_iter_ms").
The torch path forms, for all chains, eta = addmm(a, X, B) over row chunks (256
MiB of logits), log_softmax over the classes, r = onehot - softmax and the
second matmul X^T r: the likelihood's gradient only, no priors and no leapfrog
arithmetic, so it is compared with leapfrog_ms.  Every path is timed by device
events around the enqueued work after a warm-up of the same shape, in turn; the
median and every run of --reps are reported.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ITERS = 4  # HMC iterations per timed call


def _timed(fn):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return float(a.elapsed_time(b))


def torch_grad(X, onehot, Bm, a, K, chunk_bytes=256 << 20):
    """d log likelihood / d (B, a) of C chains: Bm [P, C K], a [C K]."""
    import torch

    CK = Bm.shape[1]
    n = max(1, chunk_bytes // (4 * CK))
    G = torch.zeros_like(Bm)
    ga = torch.zeros_like(a)
    for r in range(0, X.shape[0], n):
        x = X[r:r + n]
        eta = torch.addmm(a, x, Bm).view(x.shape[0], CK // K, K)
        res = (onehot[r:r + n, None, :] - torch.softmax(eta, dim=2)).view(x.shape[0], CK)
        G.addmm_(x.t(), res)
        ga += res.sum(0)
    return G, ga


def hmc_runner(prog, C, L):
    import torch

    from mlx_mcmc_amd import _engine

    chains = _engine.ChainSet(prog, C, np.zeros(prog.D, np.float32), 1e-3)
    state = {"it": 0}

    def run():
        chains.run_hmc(samples=None, iter_begin=state["it"], iter_count=ITERS, chain_offset=0,
                       num_warmup=1 << 30, num_samples=0, sample_begin=0, sample_capacity=0,
                       seed=1, step_size=1e-3, target_accept=0.8, adapt_step_size=False,
                       num_leapfrog_steps=L)
        state["it"] += ITERS
    return run


def time_paths(paths, reps):
    import torch

    for fn in paths.values():
        fn()                                    # warm-up: same shapes, code objects loaded
    torch.cuda.synchronize()
    runs = {k: [] for k in paths}
    for _ in range(reps):                       # in turn: all see the same neighbours
        for k, fn in paths.items():
            runs[k].append(_timed(fn))
    return runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--p", type=int, nargs="+", default=[16, 64, 256])
    ap.add_argument("--k", type=int, nargs="+", default=[4, 8, 32])
    ap.add_argument("--chains", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import mlx_mcmc_amd as m
    import mlx_mcmc_amd.core as mx
    from mlx_mcmc_amd import _lib, _trace

    dev = _lib.require_device()
    N, C = args.n, args.chains
    results = []

    def softmax_program(X, y, P, K):
        def lp(p):
            return (mx.sum(m.Categorical(logits=mx.array(X) @ p["B"] + p["a"]).log_prob(y))
                    + mx.sum(m.Normal(0.0, 2.0).log_prob(p["B"]))
                    + mx.sum(m.Normal(0.0, 5.0).log_prob(p["a"])))
        return _trace.compile_model(lp, {"B": np.zeros((P, K), np.float32),
                                         "a": np.zeros(K, np.float32)})

    def per_leapfrog(runs):
        t1, t9 = float(np.median(runs["L1"])), float(np.median(runs["L9"]))
        return (t9 - t1) / (8 * ITERS), t9 / ITERS

    for P in args.p:
        rng = np.random.default_rng(7 * N + P)
        X = (rng.normal(size=(N, P)) / math.sqrt(P)).astype(np.float32)
        Xd = torch.from_numpy(X).to(dev)
        for K in args.k + [2]:
            eta0 = X @ (2.0 * rng.normal(size=(P, K))).astype(np.float32)
            y = (eta0 + rng.gumbel(size=(N, K))).argmax(1)      # a draw from softmax(eta0)
            prog = softmax_program(X, y, P, K)
            onehot = torch.nn.functional.one_hot(torch.from_numpy(y).to(dev), K).float()
            gen = torch.Generator(device=dev).manual_seed(0)
            Bm = 0.5 * torch.randn((P, C * K), generator=gen, device=dev)
            av = 0.5 * torch.randn((C * K,), generator=gen, device=dev)
            paths = {"L1": hmc_runner(prog, C, 1), "L9": hmc_runner(prog, C, 9),
                     "torch": lambda: torch_grad(Xd, onehot, Bm, av, K)}
            bern = None
            if K == 2:   # the Bernoulli-logit program on the same X, y: a yardstick of the packing
                def blp(p):
                    return (mx.sum(m.Bernoulli(logits=mx.array(X) @ p["w"] + p["a"])
                                   .log_prob(y.astype(np.float32)))
                            + mx.sum(m.Normal(0.0, 2.0).log_prob(p["w"]))
                            + m.Normal(0.0, 5.0).log_prob(p["a"]))
                bern = _trace.compile_model(blp, {"w": np.zeros(P, np.float32), "a": np.float32(0)})
                paths["bL1"], paths["bL9"] = hmc_runner(bern, C, 1), hmc_runner(bern, C, 9)
            runs = time_paths(paths, args.reps)
            leap, it9 = per_leapfrog(runs)
            tms = float(np.median(runs["torch"]))
            rec = {"N": N, "P": P, "K": K, "chains": C, "D": prog.D, "slices": prog.glm_slices(C),
                   "note": prog.kernel_note, "leapfrog_ms": leap, "hmc_iter_ms_L9": it9,
                   "mfma_flops_per_s": 4.0 * N * P * K * C / (leap * 1e-3),
                   "torch_grad_ms": tms, "torch_over_leapfrog": tms / leap, "runs_ms": runs}
            if bern is not None:
                bl, bi = per_leapfrog({"L1": runs["bL1"], "L9": runs["bL9"]})
                rec.update(bernoulli_leapfrog_ms=bl, bernoulli_hmc_iter_ms_L9=bi,
                           softmax_k2_over_bernoulli=leap / bl)
            print(json.dumps(rec), flush=True)
            results.append(rec)
            del prog, bern, paths, onehot, Bm, av
            torch.cuda.empty_cache()
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "command": " ".join(["python", "scripts/bench_glm_softmax.py"] + sys.argv[1:]),
           "results": results}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
