#!/usr/bin/env python3
"""Throughput of mc_glm_predictive (statistics only) on design-matrix
likelihoods, beside the alternative a user has without it: a chunked torch
statement doing the same work on the same GPU.

    python scripts/bench_glm_predictive.py [--n 100000] [--p 16 256] [--chains 4]
        [--draws 1024] [--families normal bernoulli poisson] [--poisson-shift 0 3]
        [--reps 5] [--out FILE.json]

The likelihood is Family(X @ w + a): X ~ N(0, 1) / sqrt(P) in f32, synthetic
draws [chains, draws, P + 1 (+ 1 for log_sigma)] ~ 0.5 N(0, 1), so |eta| stays
O(1); the Poisson family also runs with a constant added to its offset
(--poisson-shift 3: rates near 20, the PTRS branch instead of the inversion).
The default, 100 K rows x 4096 draws, is 4.1e8 replicates per call.  The torch
path takes a chunk of draws (256 MiB of replicates), forms eta by addmm, draws
torch.normal / torch.bernoulli(sigmoid) / torch.poisson(exp), and reduces the
chunk to the same statistics (moments in f64, Chan's merge over chunks).  Both
paths are timed by device events around the enqueued work after a warm-up of
the same shape, alternating between the two; the median and every run of
--reps are reported.

The two paths draw from different streams, so their statistics agree only
statistically: `max_mean_diff_se` is the largest difference of the two
predictive means over observations in units of the standard error of that
difference, sqrt(2 var / n) (the maximum of 1e5 standard normals in absolute
value is about 4.6).
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


def _timed(fn):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return float(a.elapsed_time(b))


def torch_chunked(family, q, X, off, y, P, gen, chunk_bytes=256 << 20):
    """(n, mean, m2, below) by sampling chunks of draws: [R, N] f32 replicates
    per chunk, reduced in f64 and merged by Chan's update."""
    import torch

    flat = q.reshape(-1, q.shape[-1])
    N = X.shape[0]
    R = max(1, chunk_bytes // (4 * N))
    Xt = X.t()
    mean = m2 = below = None
    n = 0
    for r in range(0, flat.shape[0], R):
        rows = flat[r:r + R]
        eta = torch.addmm(rows[:, P:P + 1] + off, rows[:, :P], Xt)
        if family == "normal":
            rep = torch.normal(eta, torch.exp(rows[:, P + 1:P + 2]).expand_as(eta), generator=gen)
        elif family == "bernoulli":
            rep = torch.bernoulli(torch.sigmoid(eta), generator=gen)
        else:
            rep = torch.poisson(torch.exp(eta), generator=gen)
        cbelow = (rep < y).sum(0)
        rep = rep.double()
        cmean = rep.mean(0)
        cm2 = ((rep - cmean) ** 2).sum(0)
        k = rep.shape[0]
        if mean is None:
            mean, m2, below, n = cmean, cm2, cbelow, k
            continue
        d = cmean - mean
        tot = n + k
        mean = mean + d * (k / tot)
        m2 = m2 + cm2 + d * d * (n * k / tot)
        below = below + cbelow
        n = tot
    return n, mean, m2, below


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--p", type=int, nargs="+", default=[16, 256])
    ap.add_argument("--chains", type=int, default=4)
    ap.add_argument("--draws", type=int, default=1024)
    ap.add_argument("--families", nargs="+", default=["normal", "bernoulli", "poisson"])
    ap.add_argument("--poisson-shift", type=float, nargs="+", default=[0.0, 3.0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import mlx_mcmc_amd as m
    import mlx_mcmc_amd.core as mx
    from mlx_mcmc_amd import _lib, _trace

    dev = _lib.require_device()
    lib = _lib.load()
    N, C, S = args.n, args.chains, args.draws
    results = []
    cases = [(P, f, sh) for P in args.p for f in args.families
             for sh in (args.poisson_shift if f == "poisson" else [0.0])]
    for P, family, shift in cases:
        rng = np.random.default_rng(7 * N + P)
        X = (rng.normal(size=(N, P)) / math.sqrt(P)).astype(np.float32)
        off = np.full(N, shift, np.float32)
        eta0 = X @ rng.normal(size=P).astype(np.float32) + off
        if family == "normal":
            y = (eta0 + 0.7 * rng.normal(size=N)).astype(np.float32)
        elif family == "bernoulli":
            y = (rng.random(N) < 1.0 / (1.0 + np.exp(-eta0))).astype(np.float32)
        else:
            y = rng.poisson(np.exp(eta0)).astype(np.float32)

        def ll(p):
            eta = mx.array(X) @ p["w"] + p["a"] + mx.array(off)
            if family == "normal":
                return mx.sum(m.Normal(eta, mx.exp(p["log_sigma"])).log_prob(mx.array(y)))
            if family == "bernoulli":
                return mx.sum(m.Bernoulli(logits=eta).log_prob(y))
            return mx.sum(m.Poisson(log_rate=eta).log_prob(y))

        shapes = {"w": np.zeros(P, np.float32), "a": 0.0}
        if family == "normal":
            shapes["log_sigma"] = 0.0
        layout = _trace.layout_of(shapes)
        prog = _trace.pointwise_program(ll, layout, require_glm="bench_glm_predictive")
        D = layout.size
        gen = torch.Generator(device=dev).manual_seed(0)
        q = 0.5 * torch.randn((C, S, D), generator=gen, device=dev, dtype=torch.float32)
        st = torch.empty((_lib.MC_PP_COUNT, N), dtype=torch.float64, device=dev)
        nb = lib.mc_glm_predictive_workspace_bytes(prog.handle, C, S, 1)
        if nb < 0:
            _lib.check(int(nb))
        ws = torch.empty(max(int(nb), 1), dtype=torch.uint8, device=dev)

        def kernel():
            _lib.check(lib.mc_glm_predictive(prog.handle, C, S, 1, 1234, 0, 0, _lib.ptr(q),
                                             _lib.ptr(st), None, None, _lib.ptr(ws), nb,
                                             _lib.stream_handle()))

        Xd, od, yd = (torch.from_numpy(v).to(dev) for v in (X, off, y))
        alt = {}

        def torch_path():
            alt["r"] = torch_chunked(family, q, Xd, od, yd, P, gen)

        kernel()                                # warm-up: same shapes, code objects loaded
        torch_path()
        torch.cuda.synchronize()
        k_all, t_all = [], []
        for _ in range(args.reps):              # alternating: both see the same neighbours
            k_all.append(_timed(kernel))
            t_all.append(_timed(torch_path))
        ms, tms = float(np.median(k_all)), float(np.median(t_all))
        _, tmean, tm2, tbelow = alt["r"]
        n = float(C * S)
        var = st[_lib.MC_PP_M2] / (n - 1.0)
        se = torch.sqrt(2.0 * var / n)
        ed = float(N) * C * S
        rec = {"family": family, "poisson_shift": shift, "N": N, "P": P, "D": D, "chains": C,
               "draws": S, "element_draws": ed, "workspace_bytes": int(nb),
               "kernel": "k_glm_predictive<%d, %d>" % (
                   prog.model.glm.family, next(t for t in (1, 2, 4, 8) if 32 * t >= P)),
               "kernel_ms": ms, "kernel_ms_all": k_all,
               "kernel_element_draws_per_s": ed / (ms * 1e-3),
               "kernel_mfma_flops_per_s": 2.0 * ed * P / (ms * 1e-3),
               "torch_ms": tms, "torch_ms_all": t_all,
               "torch_element_draws_per_s": ed / (tms * 1e-3),
               "speedup": tms / ms,
               "max_mean_diff_se": float(((st[_lib.MC_PP_MEAN] - tmean).abs() / se).max().item()),
               "max_rel_diff_var": float(((st[_lib.MC_PP_M2] - tm2).abs() / tm2).max().item()),
               "max_abs_diff_pit": float(((st[_lib.MC_PP_BELOW] - tbelow).abs() / n).max().item()),
               "nonfinite": float(st[_lib.MC_PP_NONFINITE].sum().item())}
        print(json.dumps(rec), flush=True)
        results.append(rec)
        del q, st, ws, prog, Xd
        torch.cuda.empty_cache()
    out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "command": " ".join(["python", "scripts/bench_glm_predictive.py"] + sys.argv[1:]),
           "results": results}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
