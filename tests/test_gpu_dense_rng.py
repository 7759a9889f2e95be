"""Block-wide draws on the dense HMC route (lanes_fast.h k_hmc_lf draw_block):
where a dense plan has no lane RNG plan — a slice needs more (chain, block)
jobs than a wave has lanes — the workgroup draws every Philox block once per
iteration, NBk = ceil(D / 4) momentum blocks per chain and the two accept
draws, and hands the normals out through LDS, the draws of iteration it + 1
made by the last step of iteration it into the buffer of the other parity.

Models (tests/_ragged.py's hierarchical Normal over explicit run lengths):
  g200   G = 200, N = 2000: one wave of 4 slots; 104 jobs looped on 64 lanes;
  g300   G = 300, N = 3000: 4 waves;
  g600   G = 600, N = 6000, ragged with an empty and a one-element group: 8 waves;
  g1024  G = 1024, N = 4096, ragged runs of 0..7 (every eighth group empty):
         8 waves of 128 parameters; D = 1027: 516 jobs on 512 lanes (a second
         trip), and a last block of which 3 of 4 normals are used.
g200 and g1024 are constructed so that the planner makes no lane RNG plan (a
slice holds 124 private parameters or more: 62 momentum jobs and the shared
parameters' and accept draws pass a wave's 64 lanes).  g300 and g600 (75
parameters per wave) have one (Program.hmc_dense_rng == "plan"): their
programs are compiled under MC_LANES_RNG=0, which leaves every plan without,
so that the 4-wave kernel and a ragged 8-wave layout draw block-wide too.

C = 3 chains (a dead chain in the last pair), L = 1, 2 and 5, 7 iterations of
which 3 are warmup.  Samples, positions, gradients, log p, step sizes and
accept counts are byte-equal between
  * the block-wide draws and the per-lane fallback (MC_HMC_DENSE_RNG=0 when
    the program is compiled), whose draws the existing suite ties to the oracle;
  * one launch and launches of 1 + 2 + 4 iterations (the draws made ahead
    across launch edges; with L = 1 the buffer parity alone separates a fast
    wave's writes from a slow wave's reads);
  * chain 2 alone at chain_offset = 2 and chain 2 of the whole run.
g1024's state is also checked against float64 within _ragged.bounds.
"""
import os

import numpy as np
import pytest

import workloads as W
from _ragged import check_state, ragged_hier

pytestmark = pytest.mark.gpu

C = 3
STEPS = (1, 2, 5)
SPLITS = (1, 2, 4)
_R600 = [0, 1] + [5 + (7 * i) % 11 for i in range(598)]
_R600[-1] += 6000 - sum(_R600)
# (the planner deals contiguous parameters of near-equal element counts to the
# slices, and the 8 x 2 plan holds 1024 only at exactly 128 per slice: every 8
# groups hold 32 observations, one of them none)
_R1024 = [(0, 7, 3, 5, 4, 6, 2, 5)[i % 8] for i in range(1024)]
assert sum(_R1024) == 4096
# name -> (run lengths, data order, (dense slices, slots), step size, built without a
# lane RNG plan): step sizes as tests/test_gpu_hmc_dense.py's, about 1.5 / sqrt(2 N)
# (half of that for the short ragged runs)
MODELS = {"g200": ([10] * 200, "sorted", (1, 4), 0.0217, True),
          "g300": ([10] * 300, "sorted", (4, 2), 0.019, False),
          "g600": (_R600, "shuffled", (8, 2), 0.007, False),
          "g1024": (_R1024, "shuffled", (8, 2), 0.008, True)}
ENV = ("MC_LANES_RNG", "MC_HMC_DENSE_RNG")
_models, _progs = {}, {}


def _model(name):
    if name not in _models:
        lengths, order = MODELS[name][:2]
        _models[name] = ragged_hier(W.ns_product(), lengths, order=order)
    return _models[name]


def _compile(name, env):
    from mlx_mcmc_amd import _trace

    key = (name, tuple(sorted(env.items())))
    if key not in _progs:
        lp, init, _ = _model(name)
        saved = {k: os.environ.pop(k, None) for k in ENV}
        os.environ.update(env)
        try:
            _progs[key] = _trace.compile_model(lp, init)
        finally:
            for k in ENV:
                os.environ.pop(k, None)
                if saved[k] is not None:
                    os.environ[k] = saved[k]
    prog = _progs[key]
    assert prog.slice_kernel == "lanes" and prog.lanes_fast, prog.kernel_note
    assert prog.hmc_dense == MODELS[name][2], prog.hmc_dense
    return prog


def _programs(name):
    """(block-wide draws, per-lane fallback) programs of the model."""
    base = _compile(name, {})
    if MODELS[name][4]:
        assert base.hmc_dense_rng == "block", base.hmc_dense_rng
    env = {} if base.hmc_dense_rng == "block" else {"MC_LANES_RNG": "0"}
    blk = _compile(name, env)
    lane = _compile(name, dict(env, MC_HMC_DENSE_RNG="0"))
    assert blk.hmc_dense_rng == "block" and lane.hmc_dense_rng == "lane", \
        (blk.hmc_dense_rng, lane.hmc_dense_rng)
    return blk, lane


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


@pytest.mark.parametrize("name", sorted(MODELS))
def test_block_draws_equal_the_per_lane_draws(gpu, name):
    blk, lane = _programs(name)
    _, init, data = _model(name)
    q0, eps, n = blk.layout.flatten(init), MODELS[name][3], sum(SPLITS)
    for L in STEPS:
        w = f"{name} L={L}"
        one = _hmc_state(blk, q0, (n,), L, eps)
        print(f"{w}: accepted {one['n_accept'].tolist()} of {n}")
        assert np.all(one["n_total"] == n), w
        assert one["n_accept"].sum() >= 1, w + ": no chain moved"
        if name == "g1024":
            check_state(one["q"], one["g"], one["logp"], data, what=w)
        ref = _hmc_state(lane, q0, (n,), L, eps)
        for k in one:
            assert one[k].tobytes() == ref[k].tobytes(), f"{w}: {k} differs from the per-lane draws"
        parts = _hmc_state(blk, q0, SPLITS, L, eps)
        for k in one:
            assert one[k].tobytes() == parts[k].tobytes(), f"{w}: {k} differs over splits"
        shard = _hmc_state(blk, q0, (n,), L, eps, chains=1, offset=2)
        for k in one:
            assert one[k][2:3].tobytes() == shard[k].tobytes(), \
                f"{w}: {k} of chain 2 differs in its shard"
