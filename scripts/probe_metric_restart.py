#!/usr/bin/env python3
"""When do adapted NUTS chains on the small hierarchical model reach the
step-size clamp?  Prints, for the identity and the adapted run, how many of 64
chains end with eps > 10, the iterations at which that starts (they follow the
metric updates at 150, 250, 450, 950) and one chain's trace around it
(profiles/mass_matrix/probe_hier.log)."""
import sys, os
sys.path.insert(0, os.getcwd())
import numpy as np
import mlx_mcmc_amd as m
import workloads as W
lp, init = W.hierarchical(W.ns_product(), *W.SHAPES["small"])
for adapt in (False, True):
    s, r, info = m.nuts(lp, init, num_samples=200, num_warmup=1000, step_size=2e-3, target_accept=0.8,
                        num_chains=64, key=m.random.key(0), progress=False, return_info=True,
                        return_trace=True, slice_mode="exact", adapt_mass_matrix=adapt, nuts_kernel="tape")
    eps = info.trace["step_size"]; acc = info.trace["accept_stat"]; en = info.trace["energy"]
    first = [int(np.argmax(e > 10)) if (e > 10).any() else -1 for e in eps]
    print("adapt", adapt, "chains run away:", sum(f >= 0 for f in first), "first iteration of eps>10 per chain:", sorted(set(first)))
    c = next((i for i, f in enumerate(first) if f >= 0), None)
    if c is not None:
        f = first[c]
        print(" chain", c, "eps", np.round(eps[c][f-6:f+3], 4), "alpha", np.round(acc[c][f-6:f+3], 3), "H0", en[c][f-6:f+3], "depth", info.trace["tree_depth"][c][f-6:f+3])
    ok = [i for i, f in enumerate(first) if f < 0]
    print(" surviving chains", len(ok), "final eps median", np.median(info.step_size[ok]) if ok else None,
          "mean depth", info.mean_tree_depth[ok].mean() if ok else None)
    if adapt:
        print(" minv chain", ok[0] if ok else 0, np.round(info.extra["inverse_mass_matrix"][ok[0] if ok else 0], 5))
