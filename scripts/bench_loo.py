#!/usr/bin/env python3
"""Time of PSIS-LOO (mc_psis_loo) on the README workload, split into its
stages, beside WAIC on the same draws and the alternative a user has without
it: chunks of the matrix, torch.topk and a torch restatement of the fit.

    python scripts/bench_loo.py [--shape large] [--chains 256] [--draws 1000]
        [--reps 5] [--parent-lib LIB.so] [--baseline-obs 2000] [--out FILE.json]

The likelihood is the hierarchical bench model's (scripts/bench_pointwise.py):
sum(Normal(theta[group], sigma).log_prob(y)) over synthetic draws
[chains, draws, 3 + G].  Every time is a median of --reps device-event timings
after a warm-up of the same shape.

* ``loo``: the whole launch; ``stages``: its kernels' device time by stage
  (select = the eight k_psis_count / k_psis_pick passes, gather, fit), from
  torch.profiler's kernel records of one further call (null when the profiler
  records no kernels of the library).
* ``waic``: mc_pointwise_stats on this build and, with --parent-lib (a
  libmcmc355.so built from the parent commit, loaded beside this one), on the
  parent's, alternating in the same process: ``waic_ms`` / ``parent_waic_ms``
  with every repetition, so the spread is in the record.  The two builds'
  statistics are compared bit for bit.
* ``baseline``: for the first --baseline-obs observations, the [N, chunk]
  matrix by torch broadcasting, torch.topk of the Mt + 1 smallest per column
  and the fit's grid in torch float64, scaled to all M observations
  (``baseline_ms_scaled``).  khat of the two paths is compared on that chunk.

``evaluations`` is the number of times every (draw, observation) value is
formed: 1 for WAIC, 9 for loo (eight select passes and the gather) plus the
one of its lppd.
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

LOO_EVALUATIONS = 9


def _times_ms(fn, reps):
    import torch

    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(float(a.elapsed_time(b)))
    return times


def _stage_ms(fn):
    """Device time of one call's kernels by stage, or None."""
    import torch
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    out = {"select": 0.0, "gather": 0.0, "fit": 0.0}
    seen = 0
    for ev in prof.events():
        name = ev.name
        us = getattr(ev, "device_time", None)
        if us is None:
            us = getattr(ev, "cuda_time", 0.0)
        for key, stage in (("k_psis_count", "select"), ("k_psis_pick", "select"),
                           ("k_psis_gather", "gather"), ("k_psis_fit", "fit")):
            if key in name:
                out[stage] += us * 1e-3
                seen += 1
    return out if seen else None


def torch_fit(y):
    """Step 5 of the definition on ascending exceedances y [n, K] (float64):
    khat [K]."""
    import torch

    n = y.shape[0]
    m = 30 + int(np.floor(np.sqrt(n)))
    i = torch.arange(1, m + 1, dtype=torch.float64, device=y.device)
    yq = y[int(np.floor(n / 4.0 + 0.5)) - 1]
    b = (1.0 - torch.sqrt(m / (i - 0.5)))[:, None] / (3.0 * yq)[None, :] + 1.0 / y[-1][None, :]
    kap = torch.stack([torch.log1p(-b[k][None, :] * y).mean(0) for k in range(m)])
    ll = n * (torch.log(-b / kap) - kap - 1.0)
    w = 1.0 / torch.exp(ll[None, :, :] - ll[:, None, :]).sum(1)
    w = w / w.sum(0)
    bbar = (w * b).sum(0)
    kbar = torch.log1p(-bbar[None, :] * y).mean(0)
    return (n * kbar + 5.0) / (n + 10.0)


def torch_baseline(q, y, group, mt, obs, chunk):
    """khat of observations [0, obs) by matrix chunks, topk and torch_fit."""
    import torch

    C, S, D = q.shape
    flat = q.reshape(C * S, D)
    c0 = -0.5 * float(np.log(2 * np.pi))
    sigma = flat[:, 2:3]
    logs = torch.log(sigma)
    out = []
    for o in range(0, obs, chunk):
        g = group[o:o + chunk]
        ll = (c0 - logs) - (0.5 * (y[o:o + chunk] - flat[:, 3:][:, g]) ** 2) / (sigma * sigma)
        low = torch.topk(ll, mt + 1, dim=0, largest=False, sorted=True).values.double()
        lmin, cut = low[0], low[mt]
        # (ties at the cutoff are measure zero for these continuous draws)
        t = torch.flip(low[:mt], dims=(0,))
        out.append(torch_fit(torch.exp(lmin - t) - torch.exp(lmin - cut)))
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="large")
    ap.add_argument("--chains", type=int, default=256)
    ap.add_argument("--draws", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--baseline-obs", type=int, default=2000)
    ap.add_argument("--baseline-chunk", type=int, default=250)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import mlx_mcmc_amd as m
    import mlx_mcmc_amd.core as mx
    import workloads as W
    from mlx_mcmc_amd import _lib, _trace

    dev = _lib.require_device()
    lib = _lib.load()
    G, N = W.SHAPES[args.shape]
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
    mt = int(lib.mc_psis_tail_len(C * S, 1.0))

    st = torch.empty((_lib.MC_PW_COUNT, M), dtype=torch.float64, device=dev)
    nb = lib.mc_pointwise_workspace_bytes(prog.handle, C, S)
    ws = torch.empty(max(int(nb), 1), dtype=torch.uint8, device=dev)

    def waic_on(which, stats):
        def run():
            _lib.check(which.mc_pointwise_stats(prog.handle, C, S, _lib.ptr(q), _lib.ptr(stats),
                                                None, _lib.ptr(ws), nb, _lib.stream_handle()))
        return run

    out = torch.empty((_lib.MC_PSIS_COUNT, M), dtype=torch.float64, device=dev)
    pnb = lib.mc_psis_workspace_bytes(prog.handle, C, S, 1.0)
    if pnb < 0:
        _lib.check(int(pnb))
    pws = torch.empty(max(int(pnb), 8), dtype=torch.uint8, device=dev)

    def loo():
        _lib.check(lib.mc_psis_loo(prog.handle, C, S, 1.0, _lib.ptr(q), _lib.ptr(out), None,
                                   _lib.ptr(pws), pnb, _lib.stream_handle()))

    rec = {"shape": args.shape, "G": G, "M": M, "D": D, "chains": C, "draws": S,
           "tail_len": mt, "loo_workspace_bytes": int(pnb), "evaluations": LOO_EVALUATIONS}
    loo_ms = _times_ms(loo, args.reps)
    rec.update(loo_ms=float(np.median(loo_ms)), loo_ms_all=loo_ms, stages_ms=_stage_ms(loo))
    khat = out[_lib.MC_PSIS_KHAT].clone()
    rec.update(khat_min=float(khat.min().item()), khat_max=float(khat.max().item()),
               n_high_k=int((khat > 0.7).sum().item()))

    # WAIC on this build and the parent's, alternating
    parent = None
    if args.parent_lib:
        # (the parent's kernels on this build's program and view: the refactor
        # changed no layout, and the statistics are compared below)
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        parent.mc_pointwise_stats.restype = ctypes.c_int
        parent.mc_pointwise_stats.argtypes = dict(
            (n, a) for n, _, a in _lib.SIGNATURES)["mc_pointwise_stats"]
    st_parent = torch.empty_like(st)
    mine, theirs = [], []
    rounds = 3 if parent is not None else 1
    for _ in range(rounds):
        mine += _times_ms(waic_on(lib, st), args.reps)
        if parent is not None:
            theirs += _times_ms(waic_on(parent, st_parent), args.reps)
    rec.update(waic_ms=float(np.median(mine)), waic_ms_all=mine)
    if parent is not None:
        rec.update(parent_waic_ms=float(np.median(theirs)), parent_waic_ms_all=theirs,
                   parent_stats_bit_equal=bool(torch.equal(
                       st.view(torch.int64), st_parent.view(torch.int64))))
    rec["loo_over_waic"] = rec["loo_ms"] / rec["waic_ms"]

    # the chunked torch baseline on the first observations
    obs = min(args.baseline_obs, M)
    yd = torch.from_numpy(y).to(dev)
    gd = torch.from_numpy(group.astype(np.int64)).to(dev)
    alt = {}

    def baseline():
        alt["khat"] = torch_baseline(q, yd, gd, mt, obs, args.baseline_chunk)

    bms = _times_ms(baseline, max(1, args.reps // 2))
    rec.update(baseline_obs=obs, baseline_ms=float(np.median(bms)), baseline_ms_all=bms,
               baseline_ms_scaled=float(np.median(bms)) * M / obs,
               baseline_khat_max_abs_diff=float((alt["khat"] - khat[:obs]).abs().max().item()))
    rec["speedup_over_baseline"] = rec["baseline_ms_scaled"] / rec["loo_ms"]
    print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
                       "command": " ".join(["python", "scripts/bench_loo.py"] + sys.argv[1:]),
                       "result": rec}, f, indent=1)


if __name__ == "__main__":
    main()
