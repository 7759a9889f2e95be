"""The fast-form kernel's step loop (csrc/lanes_fast.h, k_hmc_lf): the
intermediate leapfrog steps run two per loop trip (record-line parity 0 then
1), after one aligning step when a trajectory's tags start on the other
parity and before one trailing step when their count is odd.

L = 1 .. 6 gives 0, 0, 1, 2, 3, 4 intermediate steps, so the aligning step,
the trailing step and the paired body each run alone and together.  A launch
reserves iter_count * L + 1 tags, so launches of uneven length (1 + 2 + 3
iterations) start trajectories on both parities whatever L is.  For every L:

  * one launch of 6 iterations, six launches of 1 and launches of 1 + 2 + 3
    give byte-identical draws, positions, gradients, log p, step sizes and
    accept counts — on the compile-time hierarchical form and on the run-time
    form (mc_debug_lanes_forms(0)); the two forms sum the shared parameters'
    kinetic terms in different orders (role order / ordinal order), so no
    existing test holds them bit-identical: between them the accept counts
    are equal and positions agree to the sliced tests' rtol 1e-3 / atol 1e-4
    (tests/test_gpu_sliced.py);
  * on the small hierarchical model at 2 and at 16 slices with 4 chains, as
    the planner lays it out (its 7 parameters replicated over lane groups,
    LrCtx::rep > 1: launch constants read at run time) and with MC_LANES_REP=1
    (one lane per parameter: the instantiation with the launch constants
    compiled in, the bench's).

Two more cases put the run-time-constant paths against other kernels at the
existing tolerances: the replicated layout against the term interpreter
(test_gpu_sliced.py: decisions and step sizes equal, positions rtol 1e-3),
and the reparameterised model (transformed shared parameters) against the
tape kernel (the interpreter declines transforms; test_gpu_transform.py).
"""
import numpy as np
import pytest

import workloads as W

pytestmark = pytest.mark.gpu

C = 4
NIT = 6            # 3 warmup + 3 stored iterations
SPLITS = {"one": [6], "each": [1] * 6, "uneven": [1, 2, 3]}
_progs = {}
_runs = {}


def _program(model, slices, rep1, monkeypatch):
    from mlx_mcmc_amd import _trace

    key = (model, slices, rep1)
    if key not in _progs:
        if rep1:
            monkeypatch.setenv("MC_LANES_REP", "1")   # (read when the lanes are planned)
        fn = {"hier": W.hierarchical, "reparam": W.hierarchical_reparam}[model]
        lp, init = fn(W.ns_product(), *W.SHAPES["small"])
        prog = _trace.compile_model(lp, init, slices=slices, slice_kernel="lanes")
        assert prog.slice_kernel == "lanes" and prog.lanes_fast and prog.num_slices == slices
        _progs[key] = (prog, prog.layout.flatten(init))
    return _progs[key]


def _run(prog, q0, L, split, forms=True):
    """Everything a run leaves behind, as bytes-comparable arrays."""
    import torch

    from mlx_mcmc_amd import _engine, _lib

    cfg = dict(chain_offset=0, num_warmup=3, num_samples=3, sample_begin=0, sample_capacity=3,
               seed=5, step_size=0.02, target_accept=0.8, num_leapfrog_steps=L,
               adapt_step_size=True)
    lib = _lib.load()
    if not forms:
        lib.mc_debug_lanes_forms(0)
    try:
        cs = _engine.ChainSet(prog, C, q0, 0.02)
        out = torch.zeros((C, 3, prog.D), dtype=torch.float32, device=cs.device)
        it = 0
        for n in SPLITS[split]:
            cs.run_hmc(samples=out, iter_begin=it, iter_count=n, **cfg)
            it += n
        assert it == NIT
        torch.cuda.synchronize()
        cs.check_status()
    finally:
        if not forms:
            lib.mc_debug_lanes_forms(1)
    sc = cs.scalars()
    return {"samples": out.cpu().numpy(), "q": cs.positions().cpu().numpy(),
            "g": cs.gradients().cpu().numpy(), "logp": sc["logp"].copy(),
            "step_size": sc["step_size"].copy(), "n_accept": sc["n_accept"].copy(),
            "n_total": sc["n_total"].copy(), "warmup_accept": sc["warmup_accept"].copy(),
            "warmup_total": sc["warmup_total"].copy()}


def _cached(model, slices, rep1, L, split, forms, monkeypatch):
    key = (model, slices, rep1, L, split, forms)
    if key not in _runs:
        prog, q0 = _program(model, slices, rep1, monkeypatch)
        _runs[key] = _run(prog, q0, L, split, forms)
    return _runs[key]


def _same_bytes(a, b, what):
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k)
        assert a[k].tobytes() == b[k].tobytes(), f"{what}: {k} differs"


@pytest.mark.parametrize("L", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("rep1", [False, True], ids=["replicated", "one_lane"])
@pytest.mark.parametrize("slices", [2, 16])
def test_step_loop_launch_splits_identical(gpu, monkeypatch, slices, rep1, L):
    one = _cached("hier", slices, rep1, L, "one", True, monkeypatch)
    assert np.all(one["n_total"] + one["warmup_total"] == NIT)
    assert np.all(np.isfinite(one["samples"])) and np.all(np.isfinite(one["logp"]))
    for split in ("each", "uneven"):
        _same_bytes(_cached("hier", slices, rep1, L, split, True, monkeypatch), one,
                    f"S={slices} L={L} {split}")
    # the run-time form: the same loop, its own summation order
    rt = _cached("hier", slices, rep1, L, "one", False, monkeypatch)
    for split in ("each", "uneven"):
        _same_bytes(_cached("hier", slices, rep1, L, split, False, monkeypatch), rt,
                    f"run-time form S={slices} L={L} {split}")
    np.testing.assert_array_equal(rt["n_accept"] + rt["warmup_accept"],
                                  one["n_accept"] + one["warmup_accept"])
    np.testing.assert_array_equal(rt["step_size"], one["step_size"])
    np.testing.assert_allclose(rt["samples"], one["samples"], rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(rt["q"], one["q"], rtol=1e-3, atol=1e-4)


def _hmc(lp, init, **kw):
    import mlx_mcmc_amd as m

    return m.hmc(lp, init, num_samples=10, num_warmup=10, step_size=0.02, num_leapfrog_steps=7,
                 key=m.random.key(3), num_chains=C, progress=False, return_info=True,
                 return_trace=True, **kw)


def test_replicated_layout_matches_interpreter(gpu):
    """rep > 1 (the small shape as planned): launch constants read at run
    time, against the term interpreter on the same slices."""
    lp, init = W.hierarchical(W.ns_product(), *W.SHAPES["small"])
    a, _, ia = _hmc(lp, init, num_slices=2, slice_kernel="interpreter")
    b, _, ib = _hmc(lp, init, num_slices=2, slice_kernel="lanes")
    np.testing.assert_array_equal(ia.trace["accepted"], ib.trace["accepted"])
    np.testing.assert_array_equal(ia.trace["step_size"], ib.trace["step_size"])
    for k in a:
        np.testing.assert_allclose(b[k], a[k], rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(ib.trace["energy"], ia.trace["energy"], rtol=1e-4, atol=1e-3)


def test_reparam_matches_tape(gpu, monkeypatch):
    """Transformed shared parameters (has_xf): the run-time path, 2 slices,
    against the tape kernel; launch splits byte-identical there too."""
    lp, init = W.hierarchical_reparam(W.ns_product(), *W.SHAPES["small"])
    a, _, ia = _hmc(lp, init, num_slices=1)
    b, _, ib = _hmc(lp, init, num_slices=2)
    assert ia.extra["kernel"] == "unsliced" and ib.extra["kernel"] == "lanes"
    np.testing.assert_array_equal(ia.trace["accepted"], ib.trace["accepted"])
    np.testing.assert_array_equal(ia.trace["step_size"], ib.trace["step_size"])
    for k in a:
        np.testing.assert_allclose(b[k], a[k], rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(ib.trace["energy"], ia.trace["energy"], rtol=1e-4, atol=1e-3)
    for L in (3, 4):
        one = _cached("reparam", 2, False, L, "one", True, monkeypatch)
        _same_bytes(_cached("reparam", 2, False, L, "uneven", True, monkeypatch), one,
                    f"reparam L={L} uneven")
