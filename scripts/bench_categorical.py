#!/usr/bin/env python3
"""Throughput of the Categorical likelihood.

    python scripts/bench_categorical.py [--n 100000] [--chains 64] [--reps 5]
        [--affine] [--out FILE.json]

HMC softmax regression with a reference class, K = 3, N observations,
`--chains` chains, L = 10, fixed step size, four broadcast parameters (the lane
planner's limit): chain-leapfrog-steps/s of the kernel alone (device events
around the launches, median of --reps) for

  node          ``Categorical(logits=[0, a1 + b1 * x, a2 + b2 * x])``
  hand_written  the same model from existing ops: one-hot ``mx.where`` masks
                and the naive ``log(1 + exp e1 + exp e2)``, each class logit
                built once with ``mx.add`` / ``mx.multiply`` so that it names
                the predictor once (two masks and two copies of x: 4 N floats
                against the node model's 2 N).  ``--affine`` writes the
                logits with ``+`` / ``*`` instead: the affine form is expanded
                at each of its two uses, x is uploaded four times (6 N floats)
                and at N = 100 K the lane planner declines

with the kernel route of each (the default plan) and the planner's note.  Run it
under scripts/ab_lib.py with another build of the library for that build's
hand-written figure (a build without the Categorical nodes reports the node row
as unavailable).  Replicate throughput is not measured: a Categorical term has
no sampler yet.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F32 = np.float32


def models(n=100_000, seed=71, affine=False):
    """(node model, hand-written model, init) on the same seeded data."""
    import mlx_mcmc_amd as m
    import mlx_mcmc_amd.core as mx

    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 1.0, n).astype(F32)
    eta = np.stack([np.zeros(n), 0.3 + 0.8 * x, -0.4 - 0.6 * x])
    cum = np.cumsum(np.exp(eta) / np.exp(eta).sum(0), axis=0)
    y = (rng.random(n)[None, :] > cum).sum(0).clip(0, 2).astype(F32)
    m1, m2 = (y == 1).astype(F32), (y == 2).astype(F32)
    init = {"a1": F32(0.2), "b1": F32(0.7), "a2": F32(-0.3), "b2": F32(-0.5)}

    def prior(p):
        return sum(m.Normal(0, 5).log_prob(p[k]) for k in init)

    def node(p):
        return prior(p) + mx.sum(m.Categorical(
            logits=[0.0, p["a1"] + p["b1"] * x, p["a2"] + p["b2"] * x]).log_prob(y))

    def hand(p):
        if affine:
            e1, e2 = p["a1"] + p["b1"] * x, p["a2"] + p["b2"] * x
        else:
            e1 = mx.add(p["a1"], mx.multiply(p["b1"], x))
            e2 = mx.add(p["a2"], mx.multiply(p["b2"], x))
        return prior(p) + mx.sum(mx.where(m1, e1, 0.0) + mx.where(m2, e2, 0.0)
                                 - mx.log(1.0 + mx.exp(e1) + mx.exp(e2)))
    return node, hand, init


def _timed(fn):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return float(a.elapsed_time(b))


def hmc_rate(lp, init, chains, reps, L=10, eps=1e-3, iters=20):
    import torch

    from mlx_mcmc_amd import _engine, _lib, _trace

    prog = _trace.compile_model(lp, init)
    cs = _engine.ChainSet(prog, chains, prog.layout.flatten(init), eps, device=torch.device("cuda"))
    samples = torch.empty((chains, 1, prog.D), dtype=torch.float32, device="cuda")
    cfg = dict(chain_offset=0, num_warmup=10 ** 6, num_samples=1, sample_begin=0,
               sample_capacity=1, seed=0, step_size=eps, target_accept=0.8,
               num_leapfrog_steps=L, adapt_step_size=False)
    cs.run_hmc(samples=samples, iter_begin=0, iter_count=2, **cfg)
    torch.cuda.synchronize()
    ms = []
    for r in range(reps):
        ms.append(_timed(lambda: cs.run_hmc(samples=samples, iter_begin=2 + r * iters,
                                            iter_count=iters, **cfg)))
    cs.check_status()
    model = prog.model
    nodes = sum(1 for i in range(model.n_nodes) if model.c_nodes[i].op != 0)
    return {"chain_steps_per_s": chains * iters * L / (float(np.median(ms)) * 1e-3),
            "kernel": prog.slice_kernel, "slices": int(prog.num_slices),
            "jit": int(_lib.load().mc_program_expr_jit(prog.handle)), "nodes": int(model.n_nodes),
            "op_nodes": nodes, "data_floats": int(model.data.size), "note": prog.kernel_note,
            "ms": [round(t, 3) for t in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--chains", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--affine", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    import mlx_mcmc_amd as m

    node, hand, init = models(args.n, affine=args.affine)
    out = {"n": args.n, "chains": args.chains, "affine": args.affine,
           "hand_written": hmc_rate(hand, init, args.chains, args.reps)}
    if hasattr(m, "Categorical"):
        try:
            out["node"] = hmc_rate(node, init, args.chains, args.reps)
            out["ratio"] = out["node"]["chain_steps_per_s"] / out["hand_written"]["chain_steps_per_s"]
        except Exception as e:   # (another build of the library: no Categorical nodes)
            out["node"] = f"unavailable: {e}"
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
