"""One call that the exchange launchers must split over chain blocks.

Every workgroup of an exchange launch has to be resident at once, so a call
with more chain blocks than the device holds is run as several launches: a
later launch starts at chain block g0 > 0 and on an advanced exchange tag
base (csrc/launch.h run_exchange).  A CU holds at most 4 workgroups of 8
waves, so C = 4 * (CUs // 16) * 8 + 8 chains at 16 slices (520 on 256 CUs)
are more chain blocks than any of these kernels has resident, on each route
that has such a loop: lane-resident HMC, term-interpreter HMC, sliced NUTS,
sliced MH, and lane-resident HMC compiled by the expression JIT.

The draws are keyed by the global chain id, so the call must give, bit for
bit, what the same global chains give as two separate calls (chain_offset),
split at a chain-block boundary: draws, positions and the per-chain scalars
(step sizes and counters)."""
import numpy as np
import pytest
import torch

import workloads as W
from mlx_mcmc_amd import _engine, _lib, _trace

pytestmark = pytest.mark.gpu

WARMUP, KEPT = 2, 2
SPLIT = 256  # a multiple of every route's chains per block (8 or 16)


def _chains():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return 4 * (cus // 16) * 8 + 8


def _run(prog, q0, algo, C, offset):
    cs = _engine.ChainSet(prog, C, q0, 0.01)
    total = WARMUP + KEPT
    smp = torch.empty((C, KEPT, prog.D), dtype=torch.float32, device=cs.device)
    cfg = dict(chain_offset=offset, num_samples=KEPT, sample_begin=0, sample_capacity=KEPT,
               seed=5, iter_begin=0, iter_count=total, samples=smp)
    if algo == "hmc":
        cs.run_hmc(num_warmup=WARMUP, step_size=0.01, target_accept=0.8, num_leapfrog_steps=3,
                   **cfg)
    elif algo == "nuts":
        cs.run_nuts(num_warmup=WARMUP, step_size=0.01, target_accept=0.8, max_tree_depth=3, **cfg)
    else:
        cs.run_mh(proposal_scale=0.01, num_warmup=WARMUP, **cfg)
    torch.cuda.synchronize()
    cs.check_status()
    return smp.cpu().numpy(), cs.positions().cpu().numpy().copy(), cs.scalars()


def _check_split(prog, q0, algo):
    C = _chains()
    assert C > SPLIT
    draws, pos, sc = _run(prog, q0, algo, C, 0)
    assert np.isfinite(draws).all()
    for lo, hi in ((0, SPLIT), (SPLIT, C)):
        d, q, s = _run(prog, q0, algo, hi - lo, lo)
        np.testing.assert_array_equal(draws[lo:hi], d)
        np.testing.assert_array_equal(pos[lo:hi], q)
        assert sc[lo:hi].tobytes() == s.tobytes(), f"{algo}: per-chain scalars of [{lo}, {hi})"
        np.testing.assert_array_equal(sc["step_size"][lo:hi], s["step_size"])


@pytest.mark.parametrize("route", ["lanes", "interpreter", "nuts_sliced", "mh_sliced"])
def test_chain_blocks_split_over_launches(gpu, route):
    lp, init = W.hierarchical(W.ns_product(), *W.SHAPES["medium"])
    kernel = "interpreter" if route == "interpreter" else "auto"
    prog = _trace.compile_model(lp, init, slices=16, slice_kernel=kernel)
    assert prog.num_slices == 16
    if route in ("lanes", "interpreter"):
        assert prog.slice_kernel == route, prog.kernel_note
        algo = "hmc"
    elif route == "nuts_sliced":
        assert prog.nuts_kernel(3) == "sliced"
        algo = "nuts"
    else:
        assert _lib.load().mc_program_mh_sliced(prog.handle) == 1
        algo = "mh"
    _check_split(prog, prog.layout.flatten(init), algo)


def test_chain_blocks_split_over_launches_jit_lanes(gpu):
    """The same on the JIT-compiled k_hmc_lr: the logistic regression's
    expression term on 16 slices (tests/test_gpu_expr_lanes.py's model)."""
    N = 100_000
    lp, _ = W.logistic_regression(W.ns_product(), N)
    start = {"a": np.float32(-0.3), "b": np.float32(1.1)}
    prog = _trace.compile_model(lp, start)
    assert prog.slice_kernel == "lanes" and prog.num_slices >= 2, prog.kernel_note
    _check_split(prog, prog.layout.flatten(start), "hmc")
    assert _lib.load().mc_program_expr_jit(prog.handle) == 1  # (not the tape fall-back)
