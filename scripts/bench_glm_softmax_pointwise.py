#!/usr/bin/env python3
"""Time of the pointwise log-likelihood statistics of softmax regression on the
MFMA kernel (csrc/glm_softmax_pointwise.h, pointwise_kernel="glm") against a
chunked torch statement of the same result.

    python scripts/bench_glm_softmax_pointwise.py [--n 100000] [--draws 4096]
        [--p 16 256] [--k 2 4 8 32] [--reps 3] [--out FILE.json]

The likelihood is Categorical(logits=X @ B + a): X ~ N(0, 1) / sqrt(P) in f32,
labels from the softmax at a random B, draws ~ 0.5 N(0, 1).  The kernel path is
one mc_pointwise_stats call on the [1, R, D] device buffer (its launch, the merge
of the draw blocks and the copy of the six statistics to the host).  The torch
path forms, over row chunks (256 MiB of logits), eta = addmm(a, X, B) for all
draws, log_softmax over the classes, the gather of the label's column and the
same reductions over the draw axis in float64 (max, sum exp(x - max), mean, sum of
squared deviations); its coefficient matrix [P, R K] is laid out before the
clock starts.  Both are timed by device events around the enqueued work after a
warm-up of the same shape, in turn; the median and every run of --reps are
reported, with the largest difference of the two paths' per-observation lppd.
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
    out = fn()
    b.record()
    b.synchronize()
    return float(a.elapsed_time(b)), out


def torch_stats(X, y, Bm, a, K, chunk_bytes=256 << 20):
    """(max, sumexp, mean, m2) [N] float64 of the [N, R] matrix: Bm [P, R K], a [R K]."""
    import torch

    RK = Bm.shape[1]
    R = RK // K
    n = max(1, chunk_bytes // (4 * RK))
    out = torch.empty((4, X.shape[0]), dtype=torch.float64, device=X.device)
    for r in range(0, X.shape[0], n):
        x = X[r:r + n]
        eta = torch.addmm(a, x, Bm).view(x.shape[0], R, K)
        idx = y[r:r + n, None, None].expand(x.shape[0], R, 1)
        ll = torch.log_softmax(eta, dim=2).gather(2, idx)[..., 0].double()
        mx = ll.max(1).values
        mean = ll.mean(1)
        out[0, r:r + n] = mx
        out[1, r:r + n] = torch.exp(ll - mx[:, None]).sum(1)
        out[2, r:r + n] = mean
        out[3, r:r + n] = ((ll - mean[:, None]) ** 2).sum(1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--draws", type=int, default=4096)
    ap.add_argument("--p", type=int, nargs="+", default=[16, 256])
    ap.add_argument("--k", type=int, nargs="+", default=[2, 4, 8, 32])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import mlx_mcmc_amd as m
    import mlx_mcmc_amd.core as mx
    from mlx_mcmc_amd import _lib, _trace, diagnostics

    dev = _lib.require_device()
    N, R = args.n, args.draws
    results = []
    for P in args.p:
        rng = np.random.default_rng(7 * N + P)
        X = (rng.normal(size=(N, P)) / math.sqrt(P)).astype(np.float32)
        Xd = torch.from_numpy(X).to(dev)
        for K in args.k:
            eta0 = X @ (2.0 * rng.normal(size=(P, K))).astype(np.float32)
            y = (eta0 + rng.gumbel(size=(N, K))).argmax(1)      # a draw from softmax(eta0)

            def like(p):
                return mx.sum(m.Categorical(logits=mx.array(X) @ p["B"] + p["a"]).log_prob(y))

            lay = _trace.layout_of({"B": np.zeros((P, K), np.float32),
                                    "a": np.zeros(K, np.float32)})
            prog = _trace.pointwise_program(like, lay, require_glm="pointwise_kernel='glm'",
                                            softmax=True)
            gen = torch.Generator(device=dev).manual_seed(0)
            draws = 0.5 * torch.randn((1, R, lay.size), generator=gen, device=dev)
            Bm = draws[0, :, :P * K].view(R, P, K).permute(1, 0, 2).reshape(P, R * K).contiguous()
            av = draws[0, :, P * K:].reshape(R * K).contiguous()
            yd = torch.from_numpy(y).to(dev)
            paths = {"kernel": lambda: diagnostics._pointwise_launch(prog, draws)[0],
                     "torch": lambda: torch_stats(Xd, yd, Bm, av, K)}
            for fn in paths.values():
                fn()                                # warm-up: same shapes, code objects loaded
            torch.cuda.synchronize()
            runs, last = {k: [] for k in paths}, {}
            for _ in range(args.reps):              # in turn: both see the same neighbours
                for k, fn in paths.items():
                    t, last[k] = _timed(fn)
                    runs[k].append(t)
            ref = last["torch"].cpu().numpy()
            got = last["kernel"]
            lppd_diff = float(np.max(np.abs((np.log(got["sumexp"]) + got["max"])
                                            - (np.log(ref[1]) + ref[0]))))
            kms, tms = float(np.median(runs["kernel"])), float(np.median(runs["torch"]))
            rec = {"N": N, "P": P, "K": K, "draws": R, "D": lay.size, "kernel_ms": kms,
                   "torch_ms": tms, "torch_over_kernel": tms / kms,
                   "mfma_flops_per_s": 2.0 * N * P * K * R / (kms * 1e-3),
                   "max_lppd_diff": lppd_diff, "nonfinite": float(got["nonfinite"].sum()),
                   "runs_ms": runs}
            print(json.dumps(rec), flush=True)
            results.append(rec)
            del prog, paths, draws, Bm, av, last
            torch.cuda.empty_cache()
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "command": " ".join(["python", "scripts/bench_glm_softmax_pointwise.py"] + sys.argv[1:]),
           "results": results}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
