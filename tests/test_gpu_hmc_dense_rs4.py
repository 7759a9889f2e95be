"""The one-chain dense HMC step's four-value record (lanes_fast_nc.h lf_rs4,
k_hmc_lfc NC = 1): a chain's four wave totals — log p and the three shared
cotangents — are reduce-scattered into one register, travel as one float per
(slice, value) of the LDS line and are read with one load per lane; the shared
slots' holders are the lanes 16, 32, 48 (the rows of that register), which
hand the own priors' log p to the pair route's lanes on the last step; the
own prior's gradient is formed behind the step's LDS read.  Every summation tree is the pair kernel's (lanes_fast.h k_hmc_lf,
untouched), so the forced one-chain route (MC_HMC_DENSE_CHAINS=1, read when a
program is compiled) must give the bytes of the forced pair route (=2), which
is the reference here.

Models (tests/_ragged.py's hierarchical Normal over explicit run lengths; the
smallest shapes that reach each corner of the layout):
  g257   G = 257 groups of 7: 4 waves x 2 slots, 65 parameters per wave — slot
         1 holds a single lane, every other lane of it is empty (the Z-form
         inputs of an intermediate step, empty lanes' selected zeros).  (Groups
         of 6 make a program of 1802 elements, fewer than the 2048 below which
         the automatic plan stays unsliced and makes no dense plan: program.hip
         auto_slices; 7 is the shortest run that reaches the kernel);
  g513   G = 513, ragged runs with an empty and a one-element group: 8 x 2,
         slot 1 nearly empty in every wave;
  g1024  G = 1024, runs (0, 7, 3, 5, 4, 6, 2, 5) repeated: 8 x 2, all 128
         parameters of every wave, block-wide draws.
L = 1 (the only-step kind), 2 (no intermediate step), 3 and 4 (the aligning
and the trailing parity step), 20 (the workload's own); C = 3 chains, so chain
1 is an odd chain with its hand-up; 6 iterations of which 3 are adaptive
warmup.

  * every array (samples, q, g, log p, step sizes, accept counts) of the
    one-chain route byte-equal to the pair route's;
  * launches of 1 + 2 + 3 iterations byte-equal to one launch;
  * the one-chain state against float64 within _ragged.bounds (check_state);
  * on the pair route's result: at least one proposal accepted in every case
    (the step sizes below were checked with oracle/samplers.py's HMC on the
    same models and seed on the CPU: of the 18 proposals of a case it accepts
    6 at g1024 with L = 4 and 14 .. 18 in every other case).
"""
import os

import numpy as np
import pytest

import workloads as W
from _ragged import check_state, ragged_hier

C = 3
STEPS = (1, 2, 3, 4, 20)
SPLITS = (1, 2, 3)
SEED = 5
_R513 = [0, 1] + [4 + (5 * i) % 9 for i in range(511)]
_R1024 = [(0, 7, 3, 5, 4, 6, 2, 5)[i % 8] for i in range(1024)]
# name -> (run lengths, data order, (dense slices, slots), step size)
MODELS = {"g257": ([7] * 257, "sorted", (4, 2), 0.019),
          "g513": (_R513, "shuffled", (8, 2), 0.007),
          "g1024": (_R1024, "shuffled", (8, 2), 0.008)}
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
    assert prog.hmc_dense_chains(C) == chains, prog.hmc_dense_chains(C)
    return prog


def _hmc_state(prog, q0, splits, L, eps):
    import torch

    from mlx_mcmc_amd import _engine

    n = sum(splits)
    cfg = dict(chain_offset=0, num_warmup=n // 2, num_samples=n - n // 2, sample_begin=0,
               sample_capacity=n - n // 2, seed=SEED, step_size=eps, target_accept=0.8,
               num_leapfrog_steps=L, adapt_step_size=True)
    cs = _engine.ChainSet(prog, C, q0, eps)
    out = torch.zeros((C, n - n // 2, prog.D), dtype=torch.float32, device=cs.device)
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
@pytest.mark.parametrize("L", STEPS)
@pytest.mark.parametrize("name", sorted(MODELS))
def test_four_value_record_equals_the_pair_route(gpu, name, L):
    single, pair = _program(name, 1), _program(name, 2)
    _, init, data = _model(name)
    q0, eps, n = single.layout.flatten(init), MODELS[name][3], sum(SPLITS)
    w = f"{name} L={L}"
    ref = _hmc_state(pair, q0, (n,), L, eps)
    print(f"{w}: the pair route accepted {ref['n_accept'].tolist()} of {n}")
    assert np.all(ref["n_total"] == n), w
    assert ref["n_accept"].sum() >= 1, w + ": no proposal accepted on the pair route"
    one = _hmc_state(single, q0, (n,), L, eps)
    for k in ref:
        assert one[k].tobytes() == ref[k].tobytes(), f"{w}: {k} differs from the pair route"
    parts = _hmc_state(single, q0, SPLITS, L, eps)
    for k in one:
        assert one[k].tobytes() == parts[k].tobytes(), f"{w}: {k} differs over splits"
    check_state(one["q"], one["g"], one["logp"], data, what=w)
