#!/usr/bin/env python3
"""The column-split GLM gradient kernel k_glm_grad_wide (csrc/glm_wide.h) against
k_glm_grad and against the torch statement.

    python scripts/bench_glm_wide.py [--n 100000] [--chains 256] [--L 20] [--reps 7]
        [--out profiles/glm_wide/bench_glm_wide.json]

Logistic regression of scripts/bench_glm.py, one call, HIP events:
 P = 256          mc_logp_grad and mc_hmc_run blocks on glm_kernel="auto" (k_glm_grad)
                  and on glm_kernel="wide", and the f32 torch statement eta = X @ B;
                  R = y - sigmoid(eta); G = X.T @ R, the three alternating `--reps`
                  times after a warm-up; and the largest difference of the two
                  kernels' log p and gradients at the timed points;
 P = 512, 1024    the same for "wide" and the torch statement (k_glm_grad stops at
                  256 columns).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_glm import Hmc, _spread, _timed, logistic  # noqa: E402


class WideHmc(Hmc):
    """bench_glm.Hmc on a program compiled with `glm_kernel`."""

    def __init__(self, lp, init, chains, L, glm_kernel, iters=5, eps=1e-3):
        import torch

        from mlx_mcmc_amd import _engine, _trace

        self.prog = _trace.compile_model(lp, init, glm_kernel=glm_kernel)
        self.cs = _engine.ChainSet(self.prog, chains, self.prog.layout.flatten(init), eps)
        self.samples = torch.empty((chains, 1, self.prog.D), dtype=torch.float32, device="cuda")
        self.cfg = dict(chain_offset=0, num_warmup=10 ** 6, num_samples=1, sample_begin=0,
                        sample_capacity=1, seed=0, step_size=eps, target_accept=0.8,
                        num_leapfrog_steps=L, adapt_step_size=False)
        self.chains, self.L, self.iters, self.at = chains, L, iters, 0
        self.once()


def bench_p(N, P, C, L, reps):
    import torch

    from mlx_mcmc_amd import _engine

    lp, init, X, y = logistic(N, P)
    runs = {k: WideHmc(lp, init, C, L, k) for k in (("auto", "wide") if P <= 256 else ("wide",))}
    q = torch.randn(C, runs["wide"].prog.D, device="cuda")
    Xd, yd = torch.as_tensor(X).cuda(), torch.as_tensor(y).cuda()[:, None]
    B = torch.randn(P, C, device="cuda")

    def stmt():
        R = yd - torch.sigmoid(Xd @ B)
        return Xd.T @ R

    fns = {k: (lambda r=r: _engine.logp_grad(r.prog, q)) for k, r in runs.items()}
    fns["torch_statement"] = stmt
    for f in fns.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    th = {k: [] for k in runs}
    for _ in range(reps):
        for k, f in fns.items():
            t[k].append(_timed(f))
        for k, r in runs.items():
            th[k].append(r.once())
    row = {"P": P, "N": N, "chains": C, "L": L, "slices": runs["wide"].prog.glm_slices(C),
           "note": runs["wide"].prog.kernel_note,
           "torch_statement": _spread(t["torch_statement"])}
    for k, r in runs.items():
        med = float(np.median(th[k]))
        row[k] = {"logp_grad": _spread(t[k]), "hmc_block": _spread(th[k]),
                  "hmc_steps_per_s": r.rate(med), "hmc_us_per_leapfrog": 1e3 * med / r.iters / L}
    if "auto" in runs:
        (la, ga), (lw, gw) = (_engine.logp_grad(runs[k].prog, q) for k in ("auto", "wide"))
        row["auto_vs_wide"] = {
            "max_rel_logp": float(((la - lw).abs() / la.abs().clamp(min=1.0)).max()),
            "max_abs_grad": float((ga - gw).abs().max()), "max_grad": float(ga.abs().max())}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--chains", type=int, default=256)
    ap.add_argument("--L", type=int, default=20)
    ap.add_argument("--p", type=int, nargs="*", default=[256, 512, 1024])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "glm_wide",
                                                  "bench_glm_wide.json"))
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_glm_wide.py measures on the GPU: no device is visible")
    out = {"rows": [bench_p(a.n, P, a.chains, a.L, a.reps) for P in a.p]}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
