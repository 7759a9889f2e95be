"""Every fused-term path of csrc/eval.h eval_term (strided_uscale's twelve
codes, strided_generic, seg_normal_uscale<., 0 / 1>, seg_generic) and what
csrc/program.hip plans on top (waves per chain, split or whole runs, passes,
wave tasks, barriers) against the float64 reference of tests/_fused_terms.py,
within its derived bounds, on every evaluator that runs them:

  * the interpreter tape (mc_logp_grad): every case of the table at 16 points,
    the support-edge points included (log p -inf, the outside element's
    cotangent exactly 0, every other entry within its bound), twice, the two
    launches bit-identical (every path is atomics-free: a difference is a race);
  * the running kernel of a static build (k_hmc): per path label the case with
    the most parameter operands, 3 iterations of 2 leapfrog steps on 4 chains
    at a step size at which the float64 restatement's energy error stays below
    1e-3 (chosen and checked on the CPU, _fused_terms.hmc_step_size), then
    positions, gradients and log p at the final position against float64 (the
    initialisation kernel's gradient is the interpreter's: only a state after
    a leapfrog step is k_hmc's own, and every chain must have accepted once);
  * the compiled build: the same cases plus a minimal expression term, so that
    the JIT compiles k_hmc with only that case's path (MC_JIT_SU / MC_JIT_PATHS
    / MC_JIT_DISTS, tests/test_fused_terms_reference.py): the state against
    float64 by the same bound, draws and trace bit-identical to the interpreter
    build's (mc_debug_expr_jit(0)), mc_program_expr_jit == 1.  A path that
    jit.hip fused_paths did not name evaluates to nothing there: this test
    fails if fused_paths and eval_term ever disagree;
  * the value-only pass (k_mh): 10 Metropolis-Hastings iterations, log p at
    the final position;
  * the sliced evaluators at 2 slices, the term interpreter (sliced.h) and the
    lane-resident kernel's generic path (lanes.h): every case with exactly one
    per-element parameter operand, no vector transform and a non-Normal
    distribution, and the Normal with a per-element scale.

k_nuts instantiates the same eval_lp_grad template as k_hmc and is not run
separately.

Declined by a planner (asserted, not skipped): the lane kernel declines
su11_ps ("more than 256 private parameters in a slice"); two slices of
sg_normal_vscale_wpc8 (16385 elements) are refused for both kernels ("exceeds
the LDS budget"); both decline sg_identity_pvec ("identity terms over them,
run on the chain-per-workgroup kernels").

A gather's writes count as the whole parameter vector in the barrier plan
(program.hip, "conservative"): a term gathering over a range disjoint from the
previous term's still gets a barrier — pinned as barrier_gather_disjoint
(tests/test_fused_terms_reference.py holds the plan).

What the measurement found (MI355X): no defect.  Every case on every evaluator
is within its bound, every repeated launch bit-identical, and the compiled
kernels' draws equal the interpreter build's bit for bit.  The worst measured
|error| / bound per path is MEASURED below (the interpreter tape over the
whole table); the running kernels (k_hmc static and compiled, k_mh, the two
sliced evaluators) stay below 0.29 (gradient) and 0.10 (log p).
  path              gradient  log p      path              gradient  log p
  su0               0.106     0.126      su9               0.082     0.048
  su1               0.043     0.084      su10              0.031     0.055
  su2               0.272     0.089      su11              0.228     0.081
  su3               0.126     0.087      strided_generic   0.580     0.084
  su4               0.038     0.085      seg_normal_pv0    0.213     0.075
  su5               0.283     0.072      seg_normal_pv1    0.208     0.068
  su6               0.301     0.079      seg_generic       0.567     0.081
  su7               0.295     0.089      two / three terms 0.291     0.064
  su8               0.278     0.055
(the 0.58 / 0.57: the affine loc's cases, whose bound is mostly the loc's own
two roundings)

Mutations tried, each failing a new test: in csrc/program.hip sync_before
forced to 0 (test_host_plan_is_the_tables: barrier_overlap,
barrier_gather_disjoint, barrier_task_between) and a clashing operand kept in
pass 0 instead of a further pass (the same test: pass_random_walk,
pass_random_walk_wpc4, pass_tree, pass_three); in csrc/jit.hip fused_paths the
MC_PATH_SEG_NORMAL bit never set (test_jit_defines_name_the_cases_path:
seg_normal_pv0, seg_normal_pv1).  Not tried on the device: a removed MC_SU case
(its term would add nothing to log p or the gradient: test_interpreter_tape's
case of that code compares them with float64), and the same mutations' effect
on the kernels (a race has no guaranteed symptom; the host plan is held
instead, and the repeated launches must agree in bits).
"""
import numpy as np
import pytest

import _fused_terms as F

pytestmark = pytest.mark.gpu

CASES = F.cases()
IDS = [c.name for c in CASES]

# Worst measured |error| / bound per path (gradient, log p), MI355X, the
# interpreter tape over the whole table.
MEASURED = {"su0": (0.106, 0.126), "su1": (0.043, 0.084), "su2": (0.272, 0.089),
            "su3": (0.126, 0.087), "su4": (0.038, 0.085), "su5": (0.283, 0.072),
            "su6": (0.301, 0.079), "su7": (0.295, 0.089), "su8": (0.278, 0.055),
            "su9": (0.082, 0.048), "su10": (0.031, 0.055), "su11": (0.228, 0.081),
            "strided_generic": (0.580, 0.084), "seg_normal_pv0": (0.213, 0.075),
            "seg_normal_pv1": (0.208, 0.068), "seg_generic": (0.567, 0.081),
            "barrier": (0.291, 0.064)}

_worst = {}


def _note(path, wg, wl):
    a = _worst.setdefault(path, [0.0, 0.0])
    a[0], a[1] = max(a[0], wg), max(a[1], wl)
    print(f"worst so far [{path}]: gradient {a[0]:.3f}, log p {a[1]:.3f}")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_interpreter_tape(gpu, case):
    from mlx_mcmc_amd import _engine

    prog = F.build(case)
    try:
        assert prog.wpc == case.wpc
        pts = F.points(case)
        lp, g = _engine.logp_grad(prog, pts)
        lp, g = lp.cpu().numpy(), g.cpu().numpy()
        lp2, g2 = _engine.logp_grad(prog, pts)
        assert np.array_equal(lp.view(np.uint32), lp2.cpu().numpy().view(np.uint32))
        assert np.array_equal(g.view(np.uint32), g2.cpu().numpy().view(np.uint32)), \
            "two launches differ: a race"
        if case.edge is not None:
            assert np.isneginf(lp[-1]) and g[-1, case.edge[0]] == 0.0
            assert np.all(np.isfinite(lp[:-1]))
        wg, wl = F.check_points(case, pts, lp, g, f"tape {case.name}")
        _note(case.path, wg, wl)
    finally:
        prog.close()


# ---- the running kernels ---------------------------------------------------------
CHAINS, ITERS, LEAPFROGS, SEED = 4, 3, 2, 11


def _starts(case):
    q0 = F.points(case)[:CHAINS]
    eps = min(F.hmc_step_size(case, q, L=LEAPFROGS) for q in q0)
    return q0, eps


def _hmc(prog, q0, eps):
    import torch

    from mlx_mcmc_amd import _engine

    cs = _engine.ChainSet(prog, CHAINS, q0, eps)
    smp = torch.zeros((CHAINS, ITERS, prog.D), dtype=torch.float32, device=cs.device)
    tr = _engine.make_trace(CHAINS, 0, ITERS, cs.device)
    cs.run_hmc(samples=smp, trace=tr, iter_begin=0, iter_count=ITERS, chain_offset=0,
               num_warmup=0, num_samples=ITERS, sample_begin=0, sample_capacity=ITERS, seed=SEED,
               step_size=eps, target_accept=0.8, num_leapfrog_steps=LEAPFROGS,
               adapt_step_size=False)
    torch.cuda.synchronize()
    cs.check_status()
    sc = cs.scalars()
    return {"q": cs.positions().cpu().numpy(), "g": cs.gradients().cpu().numpy(),
            "logp": sc["logp"].copy(), "n_accept": sc["n_accept"] + sc["warmup_accept"],
            "samples": smp.cpu().numpy(), "trace": tr.numpy()}


def _check_state(case, r, q0, what, extra_depth=0):
    assert np.all(r["n_accept"] >= 1), f"{what}: every chain must have moved off k_init's state"
    assert np.all(np.any(r["q"] != q0, axis=1))
    return F.check_points(case, r["q"], r["logp"], r["g"], what, extra_depth=extra_depth)


def _on_tape(prog):
    """An explicit single slice keeps the chain-per-workgroup kernels."""
    from mlx_mcmc_amd import _lib

    lib = _lib.load()
    _lib.check(lib.mc_program_set_slices(prog.handle, 1))
    assert lib.mc_program_slice_kernel(prog.handle) == 0
    assert lib.mc_program_num_slices(prog.handle) <= 1


@pytest.mark.parametrize("label", F.labels())
def test_running_kernel_static(gpu, label):
    case = F.label_case(label)
    q0, eps = _starts(case)
    prog = F.build(case)
    try:
        _on_tape(prog)
        _check_state(case, _hmc(prog, q0, eps), q0, f"k_hmc {case.name}")
    finally:
        prog.close()


@pytest.mark.parametrize("label", F.labels())
def test_running_kernel_compiled(gpu, label):
    from mlx_mcmc_amd import _lib

    lib = _lib.load()
    case = F.label_case(label).with_expr()
    q0, eps = _starts(case)
    runs = {}
    for jit in (1, 0):
        lib.mc_debug_expr_jit(jit)
        try:
            prog = F.build(case)
            try:
                _on_tape(prog)
                runs[jit] = _hmc(prog, q0, eps)
                assert lib.mc_program_expr_jit(prog.handle) == jit, \
                    (lib.mc_program_kernel_note(prog.handle) or b"").decode()[:2000]
            finally:
                prog.close()
        finally:
            lib.mc_debug_expr_jit(-1)
    _check_state(case, runs[1], q0, f"compiled k_hmc {case.name}")
    for k in ("q", "g", "logp", "samples"):
        assert np.array_equal(runs[1][k].view(np.uint32), runs[0][k].view(np.uint32)), k
    for k, v in runs[0]["trace"].items():
        np.testing.assert_array_equal(v, runs[1]["trace"][k], err_msg=k)


@pytest.mark.parametrize("label", F.labels())
def test_value_only_pass(gpu, label):
    import torch

    from mlx_mcmc_amd import _engine

    case = F.label_case(label)
    q0 = F.points(case)[:CHAINS]
    n = 10
    prog = F.build(case)
    try:
        _on_tape(prog)
        cs = _engine.ChainSet(prog, CHAINS, q0, 0.01)
        smp = torch.zeros((CHAINS, n, prog.D), dtype=torch.float32, device=cs.device)
        tr = _engine.make_trace(CHAINS, 0, n, cs.device)
        cs.run_mh(proposal_scale=0.01, samples=smp, trace=tr, chain_offset=0, num_warmup=0,
                  num_samples=n, iter_begin=0, iter_count=n, sample_begin=0, sample_capacity=n,
                  seed=SEED)
        torch.cuda.synchronize()
        cs.check_status()
        q, lp = cs.positions().cpu().numpy(), cs.scalars()["logp"].copy()
        assert tr.numpy()["accepted"].sum() >= CHAINS, "the walk moved"
        assert np.all(np.any(q != q0, axis=1))
        F.check_points(case, q, lp, None, f"k_mh {case.name}", need_grad=False)
    finally:
        prog.close()


# ---- the sliced evaluators -------------------------------------------------------
def _sliceable(c):
    if len(c.terms) != 1:
        return False
    t = c.terms[0]
    ops = [o for o in t.ops + [t.slope, t.x] if o is not None]
    if len([o for o in ops if o.kind in ("pvec", "gather")]) != 1 or \
            any(o.xf for o in ops if o.vec):
        return False
    return t.dist != F.NORMAL or (t.scale.vec and not t.affine)


SLICED = [c for c in CASES if _sliceable(c)]
# (case, kernel) -> the planner's reason; kernel 1 the term interpreter, 2 the lanes
DECLINED = {("su11_ps", 2): "more than 256 private parameters in a slice",
            ("sg_normal_vscale_wpc8", 1): "exceeds the LDS budget",
            ("sg_normal_vscale_wpc8", 2): "exceeds the LDS budget",
            ("sg_identity_pvec", 1): "identity terms over them, run on the chain-per-workgroup",
            ("sg_identity_pvec", 2): "identity terms over them, run on the chain-per-workgroup"}


@pytest.mark.parametrize("kernel", [1, 2], ids=["interp", "lanes"])
@pytest.mark.parametrize("case", SLICED, ids=[c.name for c in SLICED])
def test_sliced_evaluators(gpu, case, kernel):
    from mlx_mcmc_amd import _lib

    lib = _lib.load()
    q0, eps = _starts(case)
    prog = F.build(case)
    try:
        why = DECLINED.get((case.name, kernel))
        try:
            _lib.check(lib.mc_program_set_slices(prog.handle, 2))
            _lib.check(lib.mc_program_set_slice_kernel(prog.handle, kernel))
        except _lib.EngineError as e:
            assert why is not None and why in str(e), (case.name, kernel, str(e))
            return
        assert why is None, f"{case.name}: expected the planner to decline ({why})"
        assert lib.mc_program_num_slices(prog.handle) == 2
        assert lib.mc_program_slice_kernel(prog.handle) == kernel
        _check_state(case, _hmc(prog, q0, eps), q0, f"sliced[{kernel}] {case.name}",
                     extra_depth=2)
    finally:
        prog.close()
