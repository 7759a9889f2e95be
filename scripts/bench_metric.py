#!/usr/bin/env python3
"""What a diagonal mass matrix buys NUTS on this engine (csrc/metric.h).

Two models, 64 chains each: the kappa = 1000 Gaussian of the NUTS bench
(config 5, D = 100) and the small hierarchical shape.  Each runs three ways:

  default        identity metric on the kernel the model gets today
  tape_identity  identity metric on the chain-per-workgroup tape (k_nuts)
  tape_adapted   the metric adapted during warmup, on the tape
  lanes_adapted  the metric adapted during warmup, on the lane-resident kernel
                 (k_nuts_lr with MET, mc_nuts_run_metric_lanes)
  lanes_ones     that kernel with a metric of ones, not adapted: the draws of
                 `default`, so its leaf rate against `default`'s is the price
                 of the metric's multiplies and registers on the leaf path

The last two run on the Gaussian only (the hierarchical model has shared
parameters: not register-only).  The variants are interleaved, round after
round on one device, and every variant reports the median over the rounds of:
mean tree depth, leaf-steps/s of the timed sampling phase, and the minimum / median over the parameters of
ESS/s (reference compute_ess per chain and parameter, summed over chains,
divided by the sampling time).  Every run is the same seed: the rounds differ
in timing only.

    python scripts/bench_metric.py [--rounds 3] [--out profiles/mass_matrix]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = ("default", "tape_identity", "tape_adapted")
LANES_VARIANTS = ("lanes_adapted", "lanes_ones")


def one_run(prog, variant, init, eps0, C, Wm, K, depth, slice_mode, seed):
    import torch
    from mlx_mcmc_amd import _engine, diagnostics

    chains = _engine.ChainSet(prog, C, prog.layout.flatten(init), eps0)
    samples = torch.empty((C, K, prog.D), dtype=torch.float32, device=chains.device)
    cfg = dict(chain_offset=0, num_warmup=Wm, num_samples=K, sample_begin=0, sample_capacity=K,
               seed=seed, step_size=eps0, target_accept=0.8, max_tree_depth=depth,
               adapt_step_size=True, slice_mode=slice_mode, samples=samples)
    if variant == "default":
        launch = chains.run_nuts
    else:
        chains.set_metric()
        run = chains.run_nuts_metric_lanes if variant in LANES_VARIANTS else chains.run_nuts_metric
        launch = lambda **kw: run(adapt=variant.endswith("_adapted"), **kw)  # noqa: E731
    launch(iter_begin=0, iter_count=Wm, **cfg)
    torch.cuda.synchronize()
    g0 = chains.scalars()["n_grad"].astype(np.int64)
    t0 = time.perf_counter()
    launch(iter_begin=Wm, iter_count=K, **cfg)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    sc = chains.scalars()
    leaves = int(np.sum(sc["n_grad"].astype(np.int64) - g0))
    ess = diagnostics.ess(samples).sum(axis=0)             # over chains, per parameter
    out = {"seconds": dt, "mean_depth": float(np.mean(sc["depth_sum"] / K)),
           "leaf_steps_per_s": leaves / dt, "ess_per_s_min": float(ess.min() / dt),
           "ess_per_s_median": float(np.median(ess) / dt),
           "step_size_median": float(np.median(sc["step_size"])),
           "finite": bool(torch.isfinite(samples).all().item())}
    if variant != "default":
        out["metric_updates"] = int(chains.metric_scalars()["n_updates"].max())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--chains", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=1000)
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mass_matrix"))
    args = ap.parse_args()

    import mlx_mcmc_amd  # noqa: F401
    import workloads as W
    from mlx_mcmc_amd import _trace

    ns = W.ns_product()
    # (model, initial step size, slice mode): the bench's NUTS settings; the
    # hierarchical model with the f64 slice, which keeps its chains mixing
    # (tests/test_gpu_parity.py test_nuts_lanes_matches_tape_hierarchical)
    cases = {"illcond_d100": (W.illcond_normal(ns, 100), 0.1, 0),
             "hier_small": (W.hierarchical(ns, *W.SHAPES["small"]), 2e-3, 1)}
    os.makedirs(args.out, exist_ok=True)
    for name, ((lp, init), eps0, slice_mode) in cases.items():
        progs = {"default": _trace.compile_model(lp, init)}
        progs["tape_identity"] = progs["tape_adapted"] = _trace.compile_model(lp, init, slices=1)
        variants = VARIANTS
        if progs["default"].nuts_metric_lanes_why(10) == "":
            variants = VARIANTS + LANES_VARIANTS
            progs.update({v: progs["default"] for v in LANES_VARIANTS})
        runs = {v: [] for v in variants}
        for r in range(args.rounds + 1):                    # round 0 warms clocks and caches
            for v in variants:
                res = one_run(progs[v], v, init, eps0, args.chains, args.warmup, args.samples, 10,
                              slice_mode, seed=0)
                if r > 0:
                    runs[v].append(res)
        out = {"model": name, "chains": args.chains, "num_warmup": args.warmup,
               "num_samples": args.samples, "rounds": args.rounds, "max_tree_depth": 10,
               "kernels": {v: progs[v].nuts_kernel(10) for v in variants}, "variants": {}}
        for v in variants:
            keys = [k for k in runs[v][0] if k != "finite"]
            out["variants"][v] = {k: float(np.median([x[k] for x in runs[v]])) for k in keys}
            out["variants"][v]["finite"] = all(x["finite"] for x in runs[v])
            out["variants"][v]["seconds_all"] = [x["seconds"] for x in runs[v]]
        base = out["variants"]["default"]
        for v in variants:
            out["variants"][v]["ess_per_s_min_vs_default"] = (
                out["variants"][v]["ess_per_s_min"] / base["ess_per_s_min"])
        print(json.dumps(out), flush=True)
        with open(os.path.join(args.out, f"{name}.json"), "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
