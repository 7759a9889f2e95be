#!/usr/bin/env python3
"""Throughput of mc_predictive (statistics only) on the bench models'
likelihoods, beside the alternative a user has without it: chunked torch
sampling of the same Normal likelihood on the same GPU.

    python scripts/bench_predictive.py [--shapes large] [--chains 256]
        [--draws 1000] [--reps 5] [--out FILE.json]

The likelihood is the hierarchical bench model's (workloads.hierarchical):
sum(Normal(theta[group], sigma).log_prob(y)), N observations in G groups, over
synthetic draws [chains, draws, 3 + G].  The default, the large shape with
256 x 1000 draws, is 2.56e10 replicates.  The torch path gathers the
parameters of a chunk of draws, draws theta + sigma * randn, and reduces the
chunk to the same five statistics (moments in f64, Chan's merge).  Both paths
are timed by device events around the enqueued work after a warm-up of the
same shape, alternating between the two; the median of --reps is reported.

The two paths draw from different streams, so their statistics agree only
statistically: `max_mean_diff_se` is the largest difference of the two
predictive means over observations in units of the standard error of that
difference, sqrt(2 var / n) (the maximum of N standard normals in absolute
value is about 4.6 for N = 1e5).
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


def torch_chunked(q, y, group, gen, chunk_bytes=256 << 20):
    """(n, mean, m2, below, nonfinite) by sampling chunks of draws: [R, N] f32
    replicates per chunk, reduced in f64 and merged by Chan's update."""
    import torch

    C, S, D = q.shape
    flat = q.reshape(C * S, D)
    N = y.numel()
    R = max(1, chunk_bytes // (4 * N))
    mean = m2 = below = nonfinite = None
    n = 0
    for r in range(0, C * S, R):
        rows = flat[r:r + R]
        theta = rows[:, 3:][:, group]
        sigma = rows[:, 2:3]
        rep = theta + sigma * torch.randn(theta.shape, generator=gen, device=q.device,
                                          dtype=torch.float32)
        cbelow = (rep < y).sum(0)
        cnf = (~torch.isfinite(rep)).sum(0)
        rep = rep.double()
        cmean = rep.mean(0)
        cm2 = ((rep - cmean) ** 2).sum(0)
        k = rep.shape[0]
        if mean is None:
            mean, m2, below, nonfinite, n = cmean, cm2, cbelow, cnf, k
            continue
        d = cmean - mean
        tot = n + k
        mean = mean + d * (k / tot)
        m2 = m2 + cm2 + d * d * (n * k / tot)
        below = below + cbelow
        nonfinite = nonfinite + cnf
        n = tot
    return n, mean, m2, below, nonfinite


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["large"])
    ap.add_argument("--chains", type=int, default=256)
    ap.add_argument("--draws", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import mlx_mcmc_amd as m
    import mlx_mcmc_amd.core as mx
    import workloads as W
    from mlx_mcmc_amd import _lib, _trace

    dev = _lib.require_device()
    lib = _lib.load()
    results = []
    for shape in args.shapes:
        G, N = W.SHAPES[shape]
        y, group = W.hierarchical_data(G, N)

        def ll(p):
            return mx.sum(m.Normal(p["theta"][group], p["sigma"]).log_prob(y))

        layout = _trace.layout_of({"mu": 0.0, "tau": 1.0, "sigma": 1.0,
                                   "theta": np.zeros(G, np.float32)})
        prog = _trace.pointwise_program(ll, layout)
        C, S, D = args.chains, args.draws, layout.size
        gen = torch.Generator(device=dev).manual_seed(0)
        q = torch.randn((C, S, D), generator=gen, device=dev, dtype=torch.float32)
        q[..., 2] = 0.5 + q[..., 2].abs()              # sigma > 0
        M = prog.num_elements
        st = torch.empty((_lib.MC_PP_COUNT, M), dtype=torch.float64, device=dev)
        nb = lib.mc_predictive_workspace_bytes(prog.handle, C, S, 1)
        if nb < 0:
            _lib.check(int(nb))
        ws = torch.empty(max(int(nb), 1), dtype=torch.uint8, device=dev)

        def kernel():
            _lib.check(lib.mc_predictive(prog.handle, C, S, 1, 1234, 0, 0, _lib.ptr(q),
                                         _lib.ptr(st), None, _lib.ptr(ws), nb,
                                         _lib.stream_handle()))

        yd = torch.from_numpy(y).to(dev)
        gd = torch.from_numpy(group.astype(np.int64)).to(dev)
        alt = {}

        def torch_path():
            alt["r"] = torch_chunked(q, yd, gd, gen)

        kernel()                                # warm-up: same shapes, code objects loaded
        torch_path()
        torch.cuda.synchronize()
        k_all, t_all = [], []
        for _ in range(args.reps):              # alternating: both see the same neighbours
            k_all.append(_timed(kernel))
            t_all.append(_timed(torch_path))
        ms, tms = float(np.median(k_all)), float(np.median(t_all))
        tn, tmean, tm2, tbelow, tnf = alt["r"]
        n = float(C * S)
        var = st[_lib.MC_PP_M2] / (n - 1.0)
        se = torch.sqrt(2.0 * var / n)
        ed = float(M) * C * S
        rec = {"shape": shape, "G": G, "N": N, "D": D, "chains": C, "draws": S,
               "element_draws": ed, "workspace_bytes": int(nb),
               "kernel_ms": ms, "kernel_ms_all": k_all,
               "kernel_element_draws_per_s": ed / (ms * 1e-3),
               "torch_ms": tms, "torch_ms_all": t_all,
               "torch_element_draws_per_s": ed / (tms * 1e-3),
               "speedup": tms / ms,
               "max_mean_diff_se": float(((st[_lib.MC_PP_MEAN] - tmean).abs() / se).max().item()),
               "max_rel_diff_var": float(((st[_lib.MC_PP_M2] - tm2).abs() / tm2).max().item()),
               "max_abs_diff_pit": float(((st[_lib.MC_PP_BELOW] - tbelow).abs() / n).max().item()),
               "nonfinite": [float(st[_lib.MC_PP_NONFINITE].sum().item()),
                             float(tnf.sum().item())]}
        print(json.dumps(rec), flush=True)
        results.append(rec)
        del q, st, ws, prog
        torch.cuda.empty_cache()
    out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "command": " ".join(["python", "scripts/bench_predictive.py"] + sys.argv[1:]),
           "results": results}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
