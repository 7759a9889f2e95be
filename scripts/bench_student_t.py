#!/usr/bin/env python3
"""Throughput of the Student-t likelihood.

    python scripts/bench_student_t.py [--n 100000] [--chains 64] [--draws 64000]
        [--reps 5] [--only hmc|predictive] [--out FILE.json]

1  HMC robust regression ``y ~ StudentT(4, a + b x, exp(log_s))``, N
   observations, `--chains` chains, L = 10, fixed step size: chain-leapfrog-
   steps/s of the kernel alone (device events around the launches) for the class
   form and for the hand-written elementary-node form
   ``-(nu + 1) / 2 * log1p(z^2 / nu) - log s + const`` of the same data, taken
   alternately `--reps` times each, with the kernel route of each (the default
   plan).  A tree without the Student-t classes (the parent commit) reports the
   hand-written row alone.
2  Replicates: mc_predictive statistics of that likelihood (the scale a
   parameter) over `--draws` draws x N observations, beside a Normal likelihood
   of the same shape, alternately.
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
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)),
            "ms": [round(t, 3) for t in ms]}


class HmcRun:
    def __init__(self, lp, init, chains, L=10, eps=1e-3, iters=20):
        import torch

        from mlx_mcmc_amd import _engine, _lib, _trace

        self.prog = _trace.compile_model(lp, init)
        self.cs = _engine.ChainSet(self.prog, chains, self.prog.layout.flatten(init), eps,
                                   device=torch.device("cuda"))
        self.samples = torch.empty((chains, 1, self.prog.D), dtype=torch.float32, device="cuda")
        self.cfg = dict(chain_offset=0, num_warmup=10 ** 6, num_samples=1, sample_begin=0,
                        sample_capacity=1, seed=0, step_size=eps, target_accept=0.8,
                        num_leapfrog_steps=L, adapt_step_size=False)
        self.chains, self.L, self.iters, self.at, self.ms = chains, L, iters, 2, []
        self.cs.run_hmc(samples=self.samples, iter_begin=0, iter_count=2, **self.cfg)
        torch.cuda.synchronize()
        self.jit = int(_lib.load().mc_program_expr_jit(self.prog.handle))

    def once(self):
        self.ms.append(_timed(lambda: self.cs.run_hmc(samples=self.samples, iter_begin=self.at,
                                                      iter_count=self.iters, **self.cfg)))
        self.at += self.iters

    def result(self):
        self.cs.check_status()
        m = self.prog.model
        out = _spread(self.ms)
        out.update(chain_steps_per_s=self.chains * self.iters * self.L / (out["median_ms"] * 1e-3),
                   kernel=self.prog.slice_kernel, slices=int(self.prog.num_slices), jit=self.jit,
                   op_nodes=sum(1 for i in range(m.n_nodes) if m.c_nodes[i].op != 0))
        return out


def _data(n):
    rng = np.random.default_rng(0)
    x = rng.normal(0.0, 1.0, n).astype(np.float32)
    y = (0.5 + 0.8 * x + 0.7 * rng.standard_t(4, n)).astype(np.float32)
    return x, y


def bench_hmc(args):
    import math

    import mlx_mcmc_amd as m
    import mlx_mcmc_amd.core as mx

    x, y = _data(args.n)
    init = {"a": np.float32(0.4), "b": np.float32(0.7), "log_s": np.float32(-0.3)}
    c = float(np.float32(math.lgamma(2.5) - math.lgamma(2.0) - 0.5 * math.log(4.0 * math.pi)))

    def prior(p):
        return (m.Normal(0, 5).log_prob(p["a"]) + m.Normal(0, 5).log_prob(p["b"])
                + m.Normal(0, 1).log_prob(p["log_s"]))

    def hand(p):
        s = mx.exp(p["log_s"])
        z = (y - (p["a"] + p["b"] * x)) / s
        return prior(p) + mx.sum(-2.5 * mx.log1p(z * z / 4.0) - mx.log(s) + c)

    def node(p):
        return prior(p) + mx.sum(m.StudentT(4, p["a"] + p["b"] * x,
                                            mx.exp(p["log_s"])).log_prob(y))
    runs = {"hand_written": HmcRun(hand, init, args.chains)}
    if hasattr(m, "StudentT"):
        runs["student_t"] = HmcRun(node, init, args.chains)
    for _ in range(args.reps):
        for r in runs.values():
            r.once()
    out = {"n": args.n, "chains": args.chains}
    out.update({k: r.result() for k, r in runs.items()})
    if "student_t" in out:
        out["ratio"] = out["student_t"]["chain_steps_per_s"] / out["hand_written"]["chain_steps_per_s"]
    return out


def bench_predictive(args):
    import torch

    import mlx_mcmc_amd as m
    import mlx_mcmc_amd.core as mx
    from mlx_mcmc_amd import _lib, _trace

    rng = np.random.default_rng(0)
    N = args.n
    x, y = _data(N)
    C, S = 64, max(1, args.draws // 64)
    q = torch.tensor(np.stack([rng.normal(0.5, 0.05, (C, S)), rng.normal(0.8, 0.05, (C, S)),
                               np.exp(rng.normal(-0.3, 0.05, (C, S)))], axis=2).astype(np.float32),
                     device="cuda")
    lay = _trace.layout_of({"a": np.float32(0), "b": np.float32(0), "s": np.float32(1)})
    liks = {"normal": lambda p: mx.sum(m.Normal(p["a"] + p["b"] * x, p["s"]).log_prob(y))}
    if hasattr(m, "StudentT"):
        liks["student_t"] = lambda p: mx.sum(
            m.StudentT(4, p["a"] + p["b"] * x, p["s"]).log_prob(y))
    lib = _lib.load()
    runs = {}
    for name, lik in liks.items():
        prog = _trace.pointwise_program(lik, lay)
        nb = lib.mc_predictive_workspace_bytes(prog.handle, C, S, 1)
        _lib.check(min(int(nb), 0))
        st = torch.empty((_lib.MC_PP_COUNT, N), dtype=torch.float64, device="cuda")
        ws = torch.empty(max(int(nb), 1), dtype=torch.uint8, device="cuda")

        def run(prog=prog, st=st, ws=ws, nb=nb):
            _lib.check(lib.mc_predictive(prog.handle, C, S, 1, 1234, 0, 0, _lib.ptr(q),
                                         _lib.ptr(st), None, _lib.ptr(ws), nb,
                                         _lib.stream_handle()))
        run()
        runs[name] = (run, st, [], prog)
    torch.cuda.synchronize()
    for _ in range(args.reps):
        for run, _, ms, _ in runs.values():
            ms.append(_timed(run))
    reps = float(C) * S * N
    out = {"n": N, "draws": C * S, "replicates": reps}
    for name, (_, st, ms, _) in runs.items():
        host = st.cpu().numpy()
        r = _spread(ms)
        r.update(replicates_per_s=reps / (r["median_ms"] * 1e-3),
                 nonfinite=float(host[_lib.MC_PP_NONFINITE].sum()),
                 mean_of_means=float(np.nanmean(host[_lib.MC_PP_MEAN])))
        out[name] = r
    if "student_t" in out:
        out["ratio"] = out["student_t"]["median_ms"] / out["normal"]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--chains", type=int, default=64)
    ap.add_argument("--draws", type=int, default=64000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=("hmc", "predictive"))
    ap.add_argument("--out")
    args = ap.parse_args()
    out = {}
    if args.only != "predictive":
        out["hmc_robust_regression"] = bench_hmc(args)
    if args.only != "hmc":
        out["replicates"] = bench_predictive(args)
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
