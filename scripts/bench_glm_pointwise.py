#!/usr/bin/env python3
"""Throughput of the design-matrix pointwise kernel (csrc/glm_pointwise.h).

    python scripts/bench_glm_pointwise.py [--n 100000] [--chains 4] [--draws 1024]
        [--p 2 16 64 256] [--reps 7] [--chunk 256] [--window-ms 300] [--out FILE.json]

Logistic regression y ~ Bernoulli(logits = a + X beta) over C x S seeded draws,
per P:
 a  mc_pointwise_stats (k_glm_pointwise and, with B > 1 draw blocks, k_pw_merge)
    without the matrix, by device events;
 b  the chunked f32 torch statement of the same computation on the same draws:
    torch.addmm over chunks of `--chunk` draws, the Bernoulli log-density,
    logsumexp and float64 sums and sums of squares accumulated over the chunks.
A single call is milliseconds, so a timed window is one event pair around as
many back-to-back calls as fill `--window-ms` (counted from the warm-up; times
are per call: window / calls).  a and b alternate inside this one run after a
warm-up, `--reps` windows each, and the spread is reported.  "matrix_rate" is
the whole launch's 2 Np R Pp product FLOP over its time as a fraction of the FP32 matrix peak — an end-to-end figure
of (a), not the K loop's own share (that needs a kernel trace of its own).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP32_MATRIX_PEAK = 157.3e12  # MI355X, FLOP/s


def _timed(fn, calls=1):
    """ms per call over one event pair around `calls` back-to-back calls."""
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return float(a.elapsed_time(b)) / calls


def _spread(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def bench_p(N, P, C, S, reps, chunk, window_ms):
    import torch

    import mlx_mcmc_amd as m
    import mlx_mcmc_amd.core as mx
    from mlx_mcmc_amd import _lib, _trace

    rng = np.random.default_rng(1)
    X = (rng.normal(size=(N, P)) / np.sqrt(P)).astype(np.float32)
    y = (rng.random(N) < 1 / (1 + np.exp(-(X @ rng.normal(size=P))))).astype(np.float32)

    def ll(p):
        return mx.sum(m.Bernoulli(logits=p["a"] + X @ p["beta"]).log_prob(y))

    lay = _trace.layout_of({"a": np.float32(0.0), "beta": np.zeros(P, np.float32)})
    prog = _trace.pointwise_program(ll, lay)
    x = torch.as_tensor(rng.standard_normal((C, S, 1 + P)).astype(np.float32)).cuda()
    lib = _lib.load()
    st = torch.empty((_lib.MC_PW_COUNT, N), dtype=torch.float64, device="cuda")
    nb = int(lib.mc_pointwise_workspace_bytes(prog.handle, C, S))
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device="cuda")

    def ours():
        _lib.check(lib.mc_pointwise_stats(prog.handle, C, S, _lib.ptr(x), _lib.ptr(st),
                                          _lib.ptr(None), _lib.ptr(ws), nb,
                                          _lib.stream_handle()))

    Xt, yd = torch.as_tensor(X).cuda().T.contiguous(), torch.as_tensor(y).cuda()
    q = x.reshape(C * S, 1 + P)

    def stmt():
        lse = torch.full((N,), -float("inf"), dtype=torch.float64, device="cuda")
        s1 = torch.zeros(N, dtype=torch.float64, device="cuda")
        s2 = torch.zeros(N, dtype=torch.float64, device="cuda")
        for r in range(0, C * S, chunk):
            b = q[r:r + chunk]
            eta = torch.addmm(b[:, :1], b[:, 1:], Xt)                      # [chunk, N]
            v = -torch.nn.functional.softplus(torch.where(yd != 0, -eta, eta))
            lse = torch.logaddexp(lse, torch.logsumexp(v, 0).double())
            vd = v.double()
            s1 += vd.sum(0)
            s2 += (vd * vd).sum(0)
        R = C * S
        return lse, s1 / R, s2 - s1 * s1 / R

    for f in (ours, stmt):
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    # the two agree (lppd's log-sum-exp and the mean) before anything is timed
    lse, mean, _ = stmt()
    got = st.cpu().numpy()
    np.testing.assert_allclose(np.log(got[_lib.MC_PW_SUMEXP]) + got[_lib.MC_PW_MAX],
                               lse.cpu().numpy(), rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(got[_lib.MC_PW_MEAN], mean.cpu().numpy(), rtol=1e-5, atol=1e-4)
    n_ours = max(1, int(np.ceil(window_ms / _timed(ours, 3))))
    n_stmt = max(1, int(np.ceil(window_ms / _timed(stmt, 3))))
    t_ours, t_stmt = [], []
    for _ in range(reps):
        t_ours.append(_timed(ours, n_ours))
        t_stmt.append(_timed(stmt, n_stmt))
    Np, Pp = (N + 31) // 32 * 32, 32
    while Pp < P:   # (the padded operands the kernel multiplies: plan_glm's Pp)
        Pp *= 2
    mo, mt = float(np.median(t_ours)), float(np.median(t_stmt))
    return {"P": P, "N": N, "C": C, "S": S, "draw_chunk": chunk, "workspace_bytes": nb,
            "calls_per_window": {"pointwise_stats": n_ours, "torch_statement": n_stmt},
            "pointwise_stats": _spread(t_ours), "torch_statement": _spread(t_stmt),
            "torch_over_ours": mt / mo, "entries_per_s": N * C * S / (mo * 1e-3),
            "matrix_rate": 2.0 * Np * C * S * Pp / (mo * 1e-3) / FP32_MATRIX_PEAK}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--chains", type=int, default=4)
    ap.add_argument("--draws", type=int, default=1024)
    ap.add_argument("--p", type=int, nargs="*", default=[2, 16, 64, 256])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_glm_pointwise.py measures on the GPU: no device is visible")
    out = {"rows": [bench_p(a.n, P, a.chains, a.draws, a.reps, a.chunk, a.window_ms)
                    for P in a.p]}
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
