#!/usr/bin/env python3
"""Throughput of mc_pointwise_stats on the bench models' likelihoods, beside
the alternative a user has without it: chunked torch broadcasting of the same
Normal likelihood on the same GPU.

    python scripts/bench_pointwise.py [--shapes small medium large]
        [--chains 256] [--draws 1000] [--reps 5] [--out FILE.json]

The likelihood is the hierarchical bench model's (workloads.hierarchical):
sum(Normal(theta[group], sigma).log_prob(y)), N observations in G groups, over
synthetic draws [chains, draws, 3 + G] (the kernel does not care where draws
came from).  Both paths are timed by device events around the enqueued work,
after a warm-up of the same shape; the median of --reps is reported.

Counted work per element-draw of this likelihood (divisions and
transcendentals as one operation each): 9 f32 operations of the log density
(difference, square, variance, halving, quotient, log of the scale, two
subtractions, the weight) and 7 f64 operations of the statistics (the shift,
the exponential, its sum, and four of the moments) = 16.  `peak_fraction` is
element-draws/s * 16 over the 157.3 TFLOP/s f32 vector peak (spec); it counts
the f64 operations at the f32 rate and the exponential as one, so it is a
statement about counted work, not about instruction issue.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FLOPS_PER_ELEMENT_DRAW = 16
F32_VECTOR_PEAK = 157.3e12


def _median_ms(fn, reps):
    import torch

    fn()                                    # warm-up: same shape, code objects loaded
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), [float(t) for t in times]


def torch_chunked(q, y, group, chunk_bytes=256 << 20):
    """The six statistics by broadcasting chunks of draws: [R, N] f32 values
    per chunk, merged in f64 (max / rescale, Chan)."""
    import torch

    C, S, D = q.shape
    flat = q.reshape(C * S, D)
    N = y.numel()
    R = max(1, chunk_bytes // (4 * N))
    c0 = -0.5 * float(np.log(2 * np.pi))
    m = s = mean = m2 = None
    n = 0
    for r in range(0, C * S, R):
        rows = flat[r:r + R]
        theta = rows[:, 3:][:, group]
        sigma = rows[:, 2:3]
        ll = (c0 - torch.log(sigma)) - (0.5 * (y - theta) ** 2) / (sigma * sigma)
        ll = ll.double()
        cm = ll.max(0).values
        cmean = ll.mean(0)
        cm2 = ((ll - cmean) ** 2).sum(0)
        k = ll.shape[0]
        if m is None:
            m, s, mean, m2, n = cm, torch.exp(ll - cm).sum(0), cmean, cm2, k
            continue
        mn = torch.maximum(m, cm)
        s = s * torch.exp(m - mn) + torch.exp(ll - mn).sum(0)
        m = mn
        d = cmean - mean
        tot = n + k
        mean = mean + d * (k / tot)
        m2 = m2 + cm2 + d * d * (n * k / tot)
        n = tot
    return m, s, mean, m2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["small", "medium", "large"])
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
        st = torch.empty((_lib.MC_PW_COUNT, M), dtype=torch.float64, device=dev)
        nb = lib.mc_pointwise_workspace_bytes(prog.handle, C, S)
        ws = torch.empty(max(int(nb), 1), dtype=torch.uint8, device=dev)

        def kernel():
            _lib.check(lib.mc_pointwise_stats(prog.handle, C, S, _lib.ptr(q), _lib.ptr(st), None,
                                              _lib.ptr(ws), nb, _lib.stream_handle()))

        yd = torch.from_numpy(y).to(dev)
        gd = torch.from_numpy(group.astype(np.int64)).to(dev)
        ms, all_ms = _median_ms(kernel, args.reps)
        alt = {}

        def torch_path():
            alt["r"] = torch_chunked(q, yd, gd)

        tms, tall = _median_ms(torch_path, args.reps)
        # the two paths computed the same statistics
        tm, ts, tmean, tm2 = alt["r"]
        lppd_k = torch.log(st[_lib.MC_PW_SUMEXP]) + st[_lib.MC_PW_MAX]
        lppd_t = torch.log(ts) + tm
        agree = float((lppd_k - lppd_t).abs().max().item())
        agree_m2 = float(((st[_lib.MC_PW_M2] - tm2).abs() / tm2.abs().clamp_min(1e-30)).max().item())
        ed = float(M) * C * S
        rec = {"shape": shape, "G": G, "N": N, "D": D, "chains": C, "draws": S,
               "element_draws": ed, "workspace_bytes": int(nb),
               "kernel_ms": ms, "kernel_ms_all": all_ms,
               "kernel_element_draws_per_s": ed / (ms * 1e-3),
               "kernel_peak_fraction": ed / (ms * 1e-3) * FLOPS_PER_ELEMENT_DRAW / F32_VECTOR_PEAK,
               "torch_ms": tms, "torch_ms_all": tall,
               "torch_element_draws_per_s": ed / (tms * 1e-3),
               "speedup": tms / ms,
               "max_abs_diff_log_sum_exp": agree, "max_rel_diff_m2": agree_m2}
        print(json.dumps(rec), flush=True)
        results.append(rec)
        del q, st, ws, prog
        torch.cuda.empty_cache()
    out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "command": " ".join(["python", "scripts/bench_pointwise.py"] + sys.argv[1:]),
           "flops_per_element_draw": FLOPS_PER_ELEMENT_DRAW, "f32_vector_peak": F32_VECTOR_PEAK,
           "results": results}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
