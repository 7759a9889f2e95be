"""Throughput of gathered-parameter expression models (alpha[g] + beta[g] * x:
grouped expression terms, csrc/lanes.h LrTerm::kb) on the lane-resident
kernels against the chain-per-workgroup tape, N = 100 K, 256 chains: HMC
chain-leapfrog-steps/s (L = 10, three timed launches per line), NUTS
leaf-steps/s at a fixed step size and MH chain-iterations/s on the programs
nuts() / metropolis_hastings() run (_trace.nuts_program / mh_program) against
the compiled program on the tape.  The fused varying-intercept line is the
ceiling.  The record is profiles/r7/expr_gather/bench_gather.log.
    python scripts/bench_gather.py"""
import os
import sys
import time

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import workloads as W  # noqa: E402
from mlx_mcmc_amd import _engine, _lib, _trace  # noqa: E402

LIB = _lib.load()
N, CHAINS = 100000, 256


def hmc_rate(lp, init, slices, iters, L=10, eps=1e-3):
    t0 = time.perf_counter()
    prog = _trace.compile_model(lp, init, slices=slices)
    tb = time.perf_counter() - t0
    cs = _engine.ChainSet(prog, CHAINS, prog.layout.flatten(init), eps, device=torch.device("cuda"))
    smp = torch.empty((CHAINS, 1, prog.D), dtype=torch.float32, device="cuda")
    cfg = dict(chain_offset=0, num_warmup=10 ** 6, num_samples=1, sample_begin=0, sample_capacity=1,
               seed=0, step_size=eps, target_accept=0.8, num_leapfrog_steps=L, adapt_step_size=False)
    cs.run_hmc(samples=smp, iter_begin=0, iter_count=2, **cfg)
    torch.cuda.synchronize()
    out = []
    for rep in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        cs.run_hmc(samples=smp, iter_begin=2 + rep * iters, iter_count=iters, **cfg)
        e1.record()
        torch.cuda.synchronize()
        out.append(CHAINS * iters * L / (e0.elapsed_time(e1) * 1e-3) / 1e6)
    cs.check_status()
    return out, prog, tb


def nuts_rate(prog, init, eps=1e-3, iters=4):
    cs = _engine.ChainSet(prog, CHAINS, prog.layout.flatten(init), eps, device=torch.device("cuda"))
    cfg = dict(chain_offset=0, num_warmup=10 ** 6, num_samples=0, sample_begin=0, sample_capacity=0,
               seed=0, step_size=eps, target_accept=0.8, max_tree_depth=6, adapt_step_size=False,
               slice_mode=0)
    cs.run_nuts(iter_begin=0, iter_count=1, **cfg)
    torch.cuda.synchronize()
    out, it = [], 1
    for rep in range(3):
        g0 = cs.scalars()["n_grad"].astype(np.int64).sum()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        cs.run_nuts(iter_begin=it, iter_count=iters, **cfg)
        e1.record()
        torch.cuda.synchronize()
        it += iters
        out.append((cs.scalars()["n_grad"].astype(np.int64).sum() - g0) / (e0.elapsed_time(e1) * 1e-3) / 1e6)
    cs.check_status()
    return out


def mh_rate(prog, init, iters, scale=2e-3):
    cs = _engine.ChainSet(prog, CHAINS, prog.layout.flatten(init), scale, device=torch.device("cuda"))
    cfg = dict(chain_offset=0, num_warmup=0, num_samples=0, sample_begin=0, sample_capacity=0, seed=0)
    cs.run_mh(proposal_scale=scale, iter_begin=0, iter_count=4, **cfg)
    torch.cuda.synchronize()
    out, it = [], 4
    for rep in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        cs.run_mh(proposal_scale=scale, iter_begin=it, iter_count=iters, **cfg)
        e1.record()
        torch.cuda.synchronize()
        it += iters
        out.append(CHAINS * iters / (e0.elapsed_time(e1) * 1e-3) / 1e6)
    cs.check_status()
    return out


def fmt(v):
    return " ".join("%.3f" % x for x in v)


MODELS = {
    "varying slopes G=1000": lambda: W.varying_slopes(W.ns_product(), 1000, N),
    "varying slopes G=200": lambda: W.varying_slopes(W.ns_product(), 200, N),
    "weighted/indexed G=64": lambda: W.weighted_indexed(W.ns_product(), 64, N),
    "weighted/indexed G=1000": lambda: W.weighted_indexed(W.ns_product(), 1000, N),
    "varying intercept G=1000 (fused)": lambda: W.varying_intercept(W.ns_product(), 1000, N),
}
only = sys.argv[1:]
for name, mk in MODELS.items():
    if only and not any(o in name for o in only):
        continue
    lp, init = mk()
    progs = {}
    for sl, it in ((0, 20), (1, 2)):
        r, prog, tb = hmc_rate(lp, init, sl, it)
        progs[sl] = prog
        print(f"{name} N={N} HMC slices={sl}: {fmt(r)} M chain-steps/s (kernel {prog.slice_kernel}, "
              f"{prog.num_slices} slices, bundle {prog.lane_bundle}, slots {prog.lane_slots}; "
              f"build {tb:.1f} s) {prog.kernel_note}", flush=True)
    np_ = _trace.nuts_program(progs[0], 6)
    for label, p in (("nuts() program", np_), ("tape", progs[1])):
        print(f"{name} N={N} NUTS {label}: {fmt(nuts_rate(p, init))} M leaf-steps/s "
              f"(kernel {p.nuts_kernel(6)})", flush=True)
    mp = _trace.mh_program(progs[0])
    for label, p, it in (("metropolis_hastings() program", mp, 100), ("tape", progs[1], 10)):
        k = "sliced" if LIB.mc_program_mh_sliced(p.handle) == 1 else "tape"
        print(f"{name} N={N} MH {label}: {fmt(mh_rate(p, init, it))} M chain-iterations/s "
              f"(kernel {k})", flush=True)
