"""One chain per workgroup on the dense HMC route (lanes_fast_nc.h k_hmc_lfc NC = 1,
run_lanes.h launch_hmc_dense): while a launch has at most as many chains as
the device has CUs, the 4- and 8-wave dense kernels run a workgroup per chain
in plain f32 instead of a chain pair packed per workgroup.  The chain's
arithmetic, its summation trees and its draws are the pair kernel's, so the
two routes give the same bytes; MC_HMC_DENSE_CHAINS=1|2, read when a program
is compiled, fixes the route of that program.

Models (tests/_ragged.py's hierarchical Normal over explicit run lengths, the
smallest that reach each kernel; step sizes as tests/test_gpu_hmc_dense.py's
and tests/test_gpu_dense_rng.py's):
  g300   G = 300 groups of 10: 4 waves x 2 slots, a lane RNG plan;
  g600   G = 600, ragged runs with an empty and a one-element group: 8 x 2, a
         lane RNG plan (made for a pair: the one-chain kernel reads chain 0's);
  g1024  G = 1024, 128 parameters per wave: 8 x 2, block-wide draws (one
         chain's jobs and half the LDS buffer on the one-chain route).
(The one-wave kernels of g40 / g200 keep their pair form: no case here.)
C = 3 chains, L = 1, 2, 3 and 5, 6 iterations of which 3 are adaptive warmup.

  * samples, q, g, log p, step sizes and accept counts of the forced
    one-chain route byte-equal to the forced pair route (which keeps the
    pair kernel covered: the default at C = 3 is the one-chain route);
  * on the one-chain route: launches of 1 + 2 + 3 iterations byte-identical
    to one launch; chain 2 alone (chain_offset = 2) equal to chain 2 of the
    whole run; a single chain runs and equals chain 0 of the whole run;
  * the forced one-chain run's state against float64 within _ragged.bounds;
  * the rule (no device): one chain per workgroup at and below the CU count,
    a pair above, the override honoured; programs without a dense plan are
    never asked (Program.hmc_dense_chains is None).
"""
import os

import numpy as np
import pytest

import workloads as W
from _ragged import check_state, ragged_hier

C = 3
STEPS = (1, 2, 3, 5)
SPLITS = (1, 2, 3)
_R600 = [0, 1] + [5 + (7 * i) % 11 for i in range(598)]
_R600[-1] += 6000 - sum(_R600)
_R1024 = [(0, 7, 3, 5, 4, 6, 2, 5)[i % 8] for i in range(1024)]
# name -> (run lengths, data order, (dense slices, slots), step size, how it draws)
MODELS = {"g300": ([10] * 300, "sorted", (4, 2), 0.019, "plan"),
          "g600": (_R600, "shuffled", (8, 2), 0.007, "plan"),
          "g1024": (_R1024, "shuffled", (8, 2), 0.008, "block")}
ENV = "MC_HMC_DENSE_CHAINS"
_models, _progs = {}, {}


def _model(name):
    if name not in _models:
        lengths, order = MODELS[name][:2]
        _models[name] = ragged_hier(W.ns_product(), lengths, order=order)
    return _models[name]


def _program(name, chains):
    """The model's program compiled under MC_HMC_DENSE_CHAINS=`chains`."""
    from mlx_mcmc_amd import _trace

    if (name, chains) not in _progs:
        lp, init, _ = _model(name)
        saved = os.environ.pop(ENV, None)
        os.environ[ENV] = str(chains)
        try:
            _progs[name, chains] = _trace.compile_model(lp, init)
        finally:
            os.environ.pop(ENV, None)
            if saved is not None:
                os.environ[ENV] = saved
    prog = _progs[name, chains]
    assert prog.slice_kernel == "lanes" and prog.lanes_fast, prog.kernel_note
    assert prog.hmc_dense == MODELS[name][2], prog.hmc_dense
    assert prog.hmc_dense_rng == MODELS[name][4], prog.hmc_dense_rng
    for n in (1, C, 100000):
        assert prog.hmc_dense_chains(n) == chains, (n, prog.hmc_dense_chains(n))
    return prog


def _hmc_state(prog, q0, splits, L, eps, chains=C, offset=0):
    import torch

    from mlx_mcmc_amd import _engine

    n = sum(splits)
    cfg = dict(chain_offset=offset, num_warmup=n // 2, num_samples=n - n // 2, sample_begin=0,
               sample_capacity=n - n // 2, seed=5, step_size=eps, target_accept=0.8,
               num_leapfrog_steps=L, adapt_step_size=True)
    cs = _engine.ChainSet(prog, chains, q0, eps)
    out = torch.zeros((chains, n - n // 2, prog.D), dtype=torch.float32, device=cs.device)
    it = 0
    for k in splits:
        cs.run_hmc(samples=out, iter_begin=it, iter_count=k, **cfg)
        it += k
    torch.cuda.synchronize()
    cs.check_status()
    sc = cs.scalars()
    return {"samples": out.cpu().numpy(), "q": cs.positions().cpu().numpy(),
            "g": cs.gradients().cpu().numpy(), "logp": sc["logp"].copy(),
            "step_size": sc["step_size"].copy(),
            "n_accept": sc["n_accept"] + sc["warmup_accept"],
            "n_total": sc["n_total"] + sc["warmup_total"]}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(MODELS))
def test_one_chain_route_equals_the_pair_route(gpu, name):
    single, pair = _program(name, 1), _program(name, 2)
    _, init, data = _model(name)
    q0, eps, n = single.layout.flatten(init), MODELS[name][3], sum(SPLITS)
    for L in STEPS:
        w = f"{name} L={L}"
        one = _hmc_state(single, q0, (n,), L, eps)
        print(f"{w}: accepted {one['n_accept'].tolist()} of {n}")
        assert np.all(one["n_total"] == n), w
        assert one["n_accept"].sum() >= 1, w + ": no chain moved"
        ref = _hmc_state(pair, q0, (n,), L, eps)
        for k in one:
            assert one[k].tobytes() == ref[k].tobytes(), f"{w}: {k} differs from the pair route"
        # the state against float64, whatever the rule would choose
        check_state(one["q"], one["g"], one["logp"], data, what=w)
        parts = _hmc_state(single, q0, SPLITS, L, eps)
        for k in one:
            assert one[k].tobytes() == parts[k].tobytes(), f"{w}: {k} differs over splits"
        shard = _hmc_state(single, q0, (n,), L, eps, chains=1, offset=2)
        for k in one:
            assert one[k][2:3].tobytes() == shard[k].tobytes(), \
                f"{w}: {k} of chain 2 differs in its shard"
        solo = _hmc_state(single, q0, (n,), L, eps, chains=1)
        for k in one:
            assert one[k][0:1].tobytes() == solo[k].tobytes(), \
                f"{w}: {k} of chain 0 differs when it runs alone"


@pytest.mark.gpu
def test_default_route_follows_the_rule(gpu):
    import torch

    from mlx_mcmc_amd import _lib, _trace

    lp, init, _ = _model("g300")
    saved = os.environ.pop(ENV, None)
    try:
        prog = _trace.compile_model(lp, init)
        sliced = _trace.compile_model(lp, init, slices=4)
    finally:
        if saved is not None:
            os.environ[ENV] = saved
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rule = _lib.load().mc_debug_hmc_dense_chains
    assert prog.hmc_dense == (4, 2)
    for n in (1, C, cus, cus + 1, 8 * cus):
        assert prog.hmc_dense_chains(n) == rule(n, cus, 0) == (1 if n <= cus else 2), n
    # an explicit slice count runs the exchange kernels: no dense plan to ask about
    assert sliced.hmc_dense is None and sliced.hmc_dense_chains(C) is None


def test_rule_on_the_host():
    from mlx_mcmc_amd import _lib

    lib = _lib.load()
    rule = lib.mc_debug_hmc_dense_chains
    for cus in (1, 64, 256, 304):
        for n in {1, max(1, cus // 2), max(1, cus - 1), cus}:
            assert rule(n, cus, 0) == 1, (n, cus)
        for n in (cus + 1, 2 * cus, 16 * cus):
            assert rule(n, cus, 0) == 2, (n, cus)
        for n in (1, cus, cus + 1, 16 * cus):
            assert rule(n, cus, 1) == 1 and rule(n, cus, 2) == 2, (n, cus)
            assert rule(n, cus, 3) == rule(n, cus, 0) == rule(n, cus, -1), (n, cus)
    assert lib.mc_program_hmc_dense_chains(None, 4) == -1
