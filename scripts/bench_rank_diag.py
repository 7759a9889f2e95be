#!/usr/bin/env python3
"""Time of the rank-normalised diagnostics (mc_rank_diag) on a [C, S, D]
buffer of synthetic AR(1) draws, split into its stages, beside the alternative
a user has without it: a chunked torch statement of the same quantities.

    python scripts/bench_rank_diag.py [--shapes 256x1000x1000,4x1000x1000]
        [--reps 5] [--baseline-chunk 32] [--out FILE.json]

Every time is a median of --reps device-event timings after a warm-up of the
same shape.

* ``rank_diag_ms``: the whole launch; ``stages_ms``: its kernels' device time
  by stage (stage = k_rd_stage / k_rd_fold, sort = k_rd_sort_lds or the
  k_rd_ghist / k_rd_gscan / k_rd_gscatter passes, rank = k_rd_rank,
  autocovariance = k_rd_acov / k_rd_final), from torch.profiler's kernel
  records of one further call (null when the profiler records no kernels of
  the library).
* ``baseline_ms``: per chunk of elements, the split draws gathered to
  [chunk, N], torch.sort twice (values, then the order's inverse: ordinal
  ranks — ties are measure zero for these draws) for the bulk and the folded
  ranks, torch.special.ndtri, the autocovariance of z and of the two tail
  indicators by FFT in float64, and the sequence rule on the host (NumPy, all
  elements of the chunk at once).  bulk-ESS of the two paths is compared.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = (("k_rd_stage", "stage"), ("k_rd_fold", "stage"), ("k_rd_sort_lds", "sort"),
          ("k_rd_ghist", "sort"), ("k_rd_gscan", "sort"), ("k_rd_gscatter", "sort"),
          ("k_rd_rank", "rank"), ("k_rd_acov", "autocovariance"),
          ("k_rd_final", "autocovariance"))


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
    out = {"stage": 0.0, "sort": 0.0, "rank": 0.0, "autocovariance": 0.0}
    seen = 0
    for ev in prof.events():
        us = getattr(ev, "device_time", None)
        if us is None:
            us = getattr(ev, "cuda_time", 0.0)
        for key, stage in STAGES:
            if key in ev.name:
                out[stage] += us * 1e-3
                seen += 1
                break
    return out if seen else None


def host_rule(rho, N):
    """The sequence rule for every row of rho [K, n] (rho[:, 0] = 1) at once."""
    K, n = rho.shape
    npair = (n - 3) // 2 + 1            # pairs (0,1), (2,3), ... the loop may read
    P = rho[:, 0:2 * npair:2] + rho[:, 1:2 * npair:2]
    stop = np.argmax(~(P > 0), axis=1)
    stop = np.where((P > 0).all(axis=1), npair - 1, stop)       # the last pair read
    mono = np.minimum.accumulate(P, axis=1)
    idx = np.arange(npair)[None, :]
    total = np.where(idx < stop[:, None], mono, 0.0).sum(axis=1)
    last = rho[np.arange(K), 2 * stop]
    wrote = P[np.arange(K), stop] >= 0
    tau = -1 + 2 * total + np.where((last > 0) | wrote, last, 0.0)
    return N / np.maximum(tau, 1 / np.log10(N))


def torch_ess(y, N):
    """Stan's ESS of y [K, m, n] (float64 device tensor): autocovariance by FFT,
    the rule on the host."""
    import torch

    K, m, n = y.shape
    v = y - y.mean(dim=2, keepdim=True)
    f = torch.fft.rfft(v, n=2 * n, dim=2)
    acov = torch.fft.irfft(f * f.conj(), n=2 * n, dim=2)[:, :, :n] / n
    a = acov.mean(dim=1)
    W = a[:, 0] * n / (n - 1)
    vp = (n - 1) / n * W + y.mean(dim=2).var(dim=1, unbiased=True)
    rho = 1 - (W[:, None] - a) / vp[:, None]
    rho[:, 0] = 1
    return host_rule(rho.cpu().numpy(), N)


def torch_rhat(z):
    K, m, n = z.shape
    W = z.var(dim=2, unbiased=True).mean(dim=1)
    return (((n - 1) / n * W + z.mean(dim=2).var(dim=1, unbiased=True)) / W).sqrt()


def torch_z(v):
    """Normal scores of the ordinal ranks of every row of v [K, N]."""
    import torch

    N = v.shape[1]
    order = torch.sort(v, dim=1).indices
    ranks = torch.sort(order, dim=1).indices.to(torch.float64) + 1.0
    return torch.special.ndtri((ranks - 0.375) / (N + 0.25))


def torch_baseline(x, chunk):
    """bulk-ESS [D] (NumPy) — and, timed with it, every other output."""
    import torch

    C, S, D = x.shape
    n = S // 2
    m, N = 2 * C, 2 * C * n
    ess_bulk = []
    for d0 in range(0, D, chunk):
        xc = x[:, :, d0:d0 + chunk]
        y = torch.stack([xc[:, :n], xc[:, S - n:]], dim=1).reshape(m, n, -1).permute(2, 0, 1)
        y = y.contiguous()                                   # [K, m, n]
        K = y.shape[0]
        flat = y.reshape(K, N)
        z = torch_z(flat).reshape(K, m, n)
        med = flat.median(dim=1).values
        zf = torch_z((flat - med[:, None]).abs()).reshape(K, m, n)
        q = torch.quantile(flat, torch.tensor([0.05, 0.95], device=x.device), dim=1)
        rb, rf = torch_rhat(z), torch_rhat(zf)
        torch.maximum(rb, rf).cpu()
        ess_bulk.append(torch_ess(z, N))
        lo = torch_ess((y <= q[0][:, None, None]).double(), N)
        hi = torch_ess((y <= q[1][:, None, None]).double(), N)
        np.minimum(lo, hi)
    return np.concatenate(ess_bulk)


def synthetic(C, S, D, dev):
    """AR(1) draws, phi cycling over 0, 0.5, 0.9 by element."""
    import torch

    gen = torch.Generator(device=dev).manual_seed(0)
    e = torch.randn((C, S, D), generator=gen, device=dev, dtype=torch.float32)
    phi = torch.tensor([0.0, 0.5, 0.9], device=dev)[torch.arange(D, device=dev) % 3]
    x = torch.empty_like(e)
    x[:, 0] = e[:, 0]
    s = torch.sqrt(1 - phi * phi)
    for t in range(1, S):
        x[:, t] = phi * x[:, t - 1] + s * e[:, t]
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x1000x1000,4x1000x1000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--baseline-chunk", type=int, default=32)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from mlx_mcmc_amd import _lib

    dev = _lib.require_device()
    lib = _lib.load()
    recs = []
    for shape in args.shapes.split(","):
        C, S, D = (int(v) for v in shape.split("x"))
        x = synthetic(C, S, D, dev)
        nb = lib.mc_rank_diag_workspace_bytes(C, S, D)
        if nb < 0:
            _lib.check(int(nb))
        ws = torch.empty(max(int(nb), 8), dtype=torch.uint8, device=dev)
        out = torch.empty((_lib.MC_RD_COUNT, D), dtype=torch.float64, device=dev)

        def run():
            _lib.check(lib.mc_rank_diag(C, S, D, _lib.ptr(x), _lib.ptr(out), None, _lib.ptr(ws),
                                        nb, _lib.stream_handle()))

        ms = _times_ms(run, args.reps)
        rec = {"chains": C, "draws": S, "D": D, "workspace_bytes": int(nb),
               "rank_diag_ms": float(np.median(ms)), "rank_diag_ms_all": ms,
               "stages_ms": _stage_ms(run)}
        host = out.cpu().numpy()
        rec.update(rhat_rank_max=float(np.nanmax(host[_lib.MC_RD_RHAT_RANK])),
                   ess_bulk_min=float(np.nanmin(host[_lib.MC_RD_ESS_BULK])),
                   ess_tail_min=float(np.nanmin(host[_lib.MC_RD_ESS_TAIL])))
        alt = {}

        def baseline():
            alt["ess_bulk"] = torch_baseline(x, args.baseline_chunk)

        bms = _times_ms(baseline, max(1, args.reps // 2))
        rel = np.abs(alt["ess_bulk"] - host[_lib.MC_RD_ESS_BULK]) / host[_lib.MC_RD_ESS_BULK]
        rec.update(baseline_ms=float(np.median(bms)), baseline_ms_all=bms,
                   baseline_ess_bulk_max_rel_diff=float(np.nanmax(rel)))
        rec["speedup_over_baseline"] = rec["baseline_ms"] / rec["rank_diag_ms"]
        print(json.dumps(rec), flush=True)
        recs.append(rec)
        del x, ws, out
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
                       "command": " ".join(["python", "scripts/bench_rank_diag.py"] + sys.argv[1:]),
                       "results": recs}, f, indent=1)


if __name__ == "__main__":
    main()
