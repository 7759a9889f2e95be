#!/usr/bin/env python3
"""Time of mc_glm_psis_loo on design-matrix likelihoods, its split into the
eight select passes, the gather and the fit, and two yardsticks on the same GPU
and shape: one mc_pointwise_stats pass (k_glm_pointwise: the WAIC pass, the
same GEMM with the f64 exponential and moments a select pass drops), and a
chunked torch statement of the same selection.

    python scripts/bench_glm_loo.py [--n 100000] [--p 16 256] [--chains 4]
        [--draws 1024] [--families normal bernoulli poisson] [--reps 5] [--out FILE.json]

The likelihood is Family(X @ w + a): X ~ N(0, 1) / sqrt(P) in f32, synthetic
draws [chains, draws, P + 1 (+ 1 for log_sigma)] ~ 0.5 N(0, 1).  The torch path
takes a chunk of observations (256 MiB of log densities over all draws), forms
eta by addmm, the family's log density, and torch.topk(k = Mt + 1,
largest=False) over the draw axis: the cutoff and the tail below it, which is
what bench_loo.py holds term models against.  It stops there — no fit, no sums
— so the comparison is with the select and gather stages, and with the whole
loo as an upper bound.  All three are timed by device events around the
enqueued work after a warm-up of the same shape, in turn; the median and every
run of --reps are reported.  The stages come from mc_debug_glm_psis_times
(events between the launches of one call).  `max_cutoff_diff` is the largest
difference between the two paths' cutoffs (two f32 evaluations of eta).
"""
from __future__ import annotations

import argparse
import ctypes
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


def torch_select(family, q, X, off, y, lgam, P, mt, chunk_bytes=256 << 20):
    """(cutoff [N], tail [N, mt] ascending, NaN past each observation's count)."""
    import torch

    flat = q.reshape(-1, q.shape[-1])
    R = flat.shape[0]
    n = max(1, chunk_bytes // (4 * R))
    cut, tails = [], []
    for r in range(0, X.shape[0], n):
        yy = y[r:r + n]
        eta = torch.addmm(flat[:, P:P + 1] + off[r:r + n], flat[:, :P], X[r:r + n].t())
        if family == "normal":
            ls = flat[:, P + 1:P + 2]
            z = (yy - eta) * torch.exp(-ls)
            ll = -0.5 * math.log(2.0 * math.pi) - ls - 0.5 * z * z
        elif family == "bernoulli":
            ll = -torch.nn.functional.softplus(torch.where(yy != 0, -eta, eta))
        else:
            ll = yy * eta - torch.exp(eta) - lgam[r:r + n]
        low = torch.topk(ll, mt + 1, dim=0, largest=False, sorted=True).values
        c = low[mt]
        cut.append(c)
        tails.append(torch.where(low[:mt] < c, low[:mt], torch.nan).t())
    return torch.cat(cut), torch.cat(tails)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--p", type=int, nargs="+", default=[16, 256])
    ap.add_argument("--chains", type=int, default=4)
    ap.add_argument("--draws", type=int, default=1024)
    ap.add_argument("--families", nargs="+", default=["normal", "bernoulli", "poisson"])
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
    mt = int(lib.mc_psis_tail_len(C * S, 1.0))
    results = []
    for P, family in [(P, f) for P in args.p for f in args.families]:
        rng = np.random.default_rng(7 * N + P)
        X = (rng.normal(size=(N, P)) / math.sqrt(P)).astype(np.float32)
        off = np.zeros(N, np.float32)
        eta0 = X @ rng.normal(size=P).astype(np.float32)
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
        prog = _trace.pointwise_program(ll, layout, require_glm="bench_glm_loo")
        D = layout.size
        gen = torch.Generator(device=dev).manual_seed(0)
        q = 0.5 * torch.randn((C, S, D), generator=gen, device=dev, dtype=torch.float32)
        out = torch.empty((_lib.MC_PSIS_COUNT, N), dtype=torch.float64, device=dev)
        tl = torch.empty((N, mt), dtype=torch.float32, device=dev)
        nb = lib.mc_glm_psis_workspace_bytes(prog.handle, C, S, 1.0)
        if nb < 0:
            _lib.check(int(nb))
        ws = torch.empty(max(int(nb), 8), dtype=torch.uint8, device=dev)
        st = torch.empty((_lib.MC_PW_COUNT, N), dtype=torch.float64, device=dev)
        pnb = lib.mc_pointwise_workspace_bytes(prog.handle, C, S)
        pws = torch.empty(max(int(pnb), 1), dtype=torch.uint8, device=dev)
        stages = (ctypes.c_float * 18)()

        def loo():
            _lib.check(lib.mc_glm_psis_loo(prog.handle, C, S, 1.0, _lib.ptr(q), _lib.ptr(out),
                                           _lib.ptr(tl), _lib.ptr(ws), nb, _lib.stream_handle()))

        def waic_pass():
            _lib.check(lib.mc_pointwise_stats(prog.handle, C, S, _lib.ptr(q), _lib.ptr(st), None,
                                              _lib.ptr(pws), pnb, _lib.stream_handle()))

        def staged():
            _lib.check(lib.mc_debug_glm_psis_times(prog.handle, C, S, 1.0, _lib.ptr(q),
                                                   _lib.ptr(out), _lib.ptr(ws), nb,
                                                   _lib.stream_handle(), stages))
            return list(stages)

        Xd, od, yd = (torch.from_numpy(v).to(dev) for v in (X, off, y))
        lgam = torch.lgamma(yd + 1.0)
        alt = {}

        def torch_path():
            alt["r"] = torch_select(family, q, Xd, od, yd, lgam, P, mt)

        loo()                                   # warm-up: same shapes, code objects loaded
        waic_pass()
        torch_path()
        torch.cuda.synchronize()
        l_all, w_all, t_all, s_all = [], [], [], []
        for _ in range(args.reps):              # in turn: all see the same neighbours
            l_all.append(_timed(loo))
            w_all.append(_timed(waic_pass))
            t_all.append(_timed(torch_path))
            s_all.append(staged())
        sm = np.median(np.asarray(s_all, np.float64), axis=0)
        count, pick = sm[0:16:2], sm[1:16:2]
        lms, wms, tms = (float(np.median(v)) for v in (l_all, w_all, t_all))
        tcut, ttail = alt["r"]
        dcut = out[_lib.MC_PSIS_CUTOFF]
        ed = float(N) * C * S
        rec = {"family": family, "N": N, "P": P, "D": D, "chains": C, "draws": S, "tail_len": mt,
               "element_draws": ed, "workspace_bytes": int(nb),
               "kernels": "k_glm_psis_count / k_glm_psis_gather<%d, %d>" % (
                   prog.model.glm.family, next(t for t in (1, 2, 4, 8) if 32 * t >= P)),
               "loo_ms": lms, "loo_ms_all": l_all,
               "count_ms_per_pass": [float(v) for v in count], "pick_ms_per_pass":
               [float(v) for v in pick], "gather_ms": float(sm[16]), "fit_ms": float(sm[17]),
               "count_mfma_flops_per_s": 2.0 * ed * P / (float(np.median(count)) * 1e-3),
               "waic_pass_ms": wms, "waic_pass_ms_all": w_all,
               "count_over_waic_pass": float(np.median(count)) / wms,
               "torch_select_ms": tms, "torch_select_ms_all": t_all,
               "torch_over_loo": tms / lms,
               "torch_over_select_and_gather": tms / float(count.sum() + pick.sum() + sm[16]),
               "max_cutoff_diff": float((dcut - tcut.double()).abs().max().item()),
               "tail_count_mismatches": int(((~torch.isnan(ttail)).sum(1).double()
                                             != out[_lib.MC_PSIS_TAILN]).sum().item()),
               "n_high_k": int((out[_lib.MC_PSIS_KHAT] > 0.7).sum().item())}
        print(json.dumps(rec), flush=True)
        results.append(rec)
        del q, out, tl, ws, pws, prog, Xd, alt
        torch.cuda.empty_cache()
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "command": " ".join(["python", "scripts/bench_glm_loo.py"] + sys.argv[1:]),
           "results": results}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
