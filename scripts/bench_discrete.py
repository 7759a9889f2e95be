#!/usr/bin/env python3
"""Throughput of the count likelihoods.

    python scripts/bench_discrete.py [--n 100000] [--chains 64] [--draws 256000]
        [--reps 5] [--only hmc|predictive] [--out FILE.json]

1  HMC logistic regression, N observations, `--chains` chains, L = 10, fixed
   step size: chain-leapfrog-steps/s of the kernel alone (device events around
   the launches, median of --reps) for ``Bernoulli(logits=a + b * x)`` and for
   the hand-written ``workloads.logistic_regression`` of the same data, with the
   kernel route of each (the default plan).  Run it under scripts/ab_lib.py with
   another build of the library for that build's hand-written figure (a build
   without the count nodes reports the Bernoulli row as unavailable).
2  Poisson replicates: mc_predictive statistics of ``Poisson(log_rate=a + b *
   x)`` over `--draws` draws x N observations, beside chunked ``torch.poisson``
   of the same rates reduced to the same statistics on the same GPU.  The two
   draw from different streams: `max_mean_diff_se` is the largest difference of
   the predictive means in units of its standard error.
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
    nodes = sum(1 for i in range(prog.model.n_nodes) if prog.model.c_nodes[i].op != 0)
    return {"chain_steps_per_s": chains * iters * L / (float(np.median(ms)) * 1e-3),
            "kernel": prog.slice_kernel, "slices": int(prog.num_slices),
            "jit": int(_lib.load().mc_program_expr_jit(prog.handle)), "op_nodes": nodes,
            "ms": [round(t, 3) for t in ms]}


def bench_hmc(args):
    import mlx_mcmc_amd as m
    import mlx_mcmc_amd.core as mx
    import workloads as W

    x, y = W.logistic_data(args.n)
    init = {"a": np.float32(-0.3), "b": np.float32(1.1)}
    out = {"n": args.n, "chains": args.chains}
    hand, _ = W.logistic_regression(W.ns_product(), args.n)
    out["hand_written"] = hmc_rate(hand, init, args.chains, args.reps)
    if hasattr(m, "Bernoulli"):
        def node(p):
            lp = m.Normal(0, 5).log_prob(p["a"]) + m.Normal(0, 5).log_prob(p["b"])
            return lp + mx.sum(m.Bernoulli(logits=p["a"] + p["b"] * x).log_prob(y))
        try:
            out["bernoulli_logits"] = hmc_rate(node, init, args.chains, args.reps)
            out["ratio"] = (out["bernoulli_logits"]["chain_steps_per_s"]
                            / out["hand_written"]["chain_steps_per_s"])
        except Exception as e:   # (another build of the library: no count nodes)
            out["bernoulli_logits"] = f"unavailable: {e}"
    return out


def torch_poisson_chunked(q, x, y, chunk_bytes=256 << 20):
    """The five statistics and the ties by sampling chunks of draws."""
    import torch

    R_all, N = q.shape[0], x.numel()
    R = max(1, chunk_bytes // (4 * N))
    n, mean, m2, below, equal = 0, None, None, None, None
    for r in range(0, R_all, R):
        rows = q[r:r + R]
        rep = torch.poisson(torch.exp(rows[:, 0:1] + rows[:, 1:2] * x[None, :])).to(torch.float64)
        k = rep.shape[0]
        cm = rep.mean(0)
        c2 = ((rep - cm) ** 2).sum(0)
        cb = (rep < y[None, :]).sum(0).to(torch.float64)
        ce = (rep == y[None, :]).sum(0).to(torch.float64)
        if mean is None:
            n, mean, m2, below, equal = k, cm, c2, cb, ce
        else:
            d = cm - mean
            tot = n + k
            mean = mean + d * (k / tot)
            m2 = m2 + c2 + d * d * (n * k / tot)
            below, equal, n = below + cb, equal + ce, tot
    return n, mean, m2, below, equal


def bench_predictive(args):
    import torch

    import mlx_mcmc_amd as m
    import mlx_mcmc_amd.core as mx
    from mlx_mcmc_amd import _lib, _trace

    rng = np.random.default_rng(0)
    N = args.n
    x = rng.normal(0.0, 1.0, N).astype(np.float32)
    y = rng.poisson(np.exp(0.8 + 0.5 * x)).astype(np.float32)
    C, S = 256, max(1, args.draws // 256)
    q = torch.tensor(np.stack([rng.normal(0.8, 0.05, (C, S)), rng.normal(0.5, 0.05, (C, S))],
                              axis=2).astype(np.float32), device="cuda")
    lay = _trace.layout_of({"a": np.float32(0), "b": np.float32(0)})
    prog = _trace.pointwise_program(
        lambda p: mx.sum(m.Poisson(log_rate=p["a"] + p["b"] * x).log_prob(y)), lay)
    lib = _lib.load()
    nb = lib.mc_predictive_workspace_bytes(prog.handle, C, S, 1)
    _lib.check(min(int(nb), 0))
    st = torch.empty((_lib.MC_PP_COUNT, N), dtype=torch.float64, device="cuda")
    eq = torch.empty(N, dtype=torch.float64, device="cuda")
    ws = torch.empty(max(int(nb), 1), dtype=torch.uint8, device="cuda")

    def ours():
        _lib.check(lib.mc_predictive_eq(prog.handle, C, S, 1, 1234, 0, 0, _lib.ptr(q), _lib.ptr(st),
                                        _lib.ptr(eq), None, _lib.ptr(ws), nb, _lib.stream_handle()))
    xt, yt = torch.tensor(x, device="cuda"), torch.tensor(y, device="cuda")
    flat = q.reshape(C * S, 2)
    res = {}

    def theirs():
        res["t"] = torch_poisson_chunked(flat, xt, yt)
    ours()
    theirs()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(args.reps):
        a.append(_timed(ours))
        b.append(_timed(theirs))
    n, mean, m2, _, _ = res["t"]
    host = st.cpu().numpy()
    var = host[_lib.MC_PP_M2] / (host[_lib.MC_PP_N] - 1)
    se = np.sqrt(2.0 * var / host[_lib.MC_PP_N])
    dz = np.abs(host[_lib.MC_PP_MEAN] - mean.cpu().numpy()) / se
    reps = float(C) * S * N
    return {"n": N, "draws": C * S, "replicates": reps,
            "mc_predictive_ms": float(np.median(a)), "torch_poisson_ms": float(np.median(b)),
            "mc_predictive_replicates_per_s": reps / (float(np.median(a)) * 1e-3),
            "torch_poisson_replicates_per_s": reps / (float(np.median(b)) * 1e-3),
            "speedup": float(np.median(b) / np.median(a)), "max_mean_diff_se": float(dz.max()),
            "nonfinite": float(host[_lib.MC_PP_NONFINITE].sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--chains", type=int, default=64)
    ap.add_argument("--draws", type=int, default=256000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=("hmc", "predictive"))
    ap.add_argument("--out")
    args = ap.parse_args()
    out = {}
    if args.only != "predictive":
        out["hmc_logistic"] = bench_hmc(args)
    if args.only != "hmc":
        out["poisson_replicates"] = bench_predictive(args)
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
