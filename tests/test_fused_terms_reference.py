"""The fused-term case table of tests/_fused_terms.py, on the CPU: its float64
reference against torch float64 autograd, every case's host plan
(mc_debug_term_plan, mc_program_waves_per_chain) against what the table
states, the table's completeness, the expression JIT's pruning defines
(jit.hip fused_paths) against a Python restatement of eval_term's dispatch,
and the sharpness of the derived bounds (mutants of a float32 restatement).
tests/test_gpu_fused_terms.py runs the same table on the device."""
import ctypes
import re

import numpy as np
import pytest

import _fused_terms as F

CASES = F.cases()
IDS = [c.name for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_reference_equals_torch_autograd(case):
    """The closed form equals torch float64 autograd of the same formulas at
    rtol 1e-12 (a gradient entry: of the largest entry, the two sum in
    different orders), at every point, the support edge included."""
    for q in F.points(case):
        rl, rg = F.ref_logp_grad(case, q)
        tl, tg = F.torch_logp_grad(case, q)
        if np.isneginf(tl):
            assert np.isneginf(rl)
        else:
            assert abs(rl - tl) <= 1e-12 * abs(tl), (rl, tl)
        np.testing.assert_allclose(rg, tg, rtol=1e-12, atol=1e-12 * max(1.0, np.max(np.abs(tg))))
    if case.edge is not None:
        q = F.points(case)[-1]
        rl, rg = F.ref_logp_grad(case, q)
        assert np.isneginf(rl) and rg[case.edge[0]] == 0.0
        assert np.isfinite(F.ref_logp_grad(case, F.points(case)[0])[0])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_host_plan_is_the_tables(case):
    """Every case builds host-only, and the planner gives each term the
    primary, passes, masks, wave task, split, barrier and waves per chain the
    table states; the path label is the one eval_term's dispatch (restated)
    gives the term, and the tiling restated in _fused_terms.seg_plan agrees."""
    p = F.build(case, host_only=True)
    try:
        assert p.wpc == case.wpc
        for pos, ti in enumerate(case.order):
            t, pl = case.terms[ti], case.plans[pos]
            got = p.plan(pos)
            masks = pl.masks if pl.masks is not None else [F.default_masks(t)]
            assert len(masks) == pl.npass
            want = {"dist": t.dist, "n": t.n, "primary": pl.primary, "npass": pl.npass,
                    "pass_masks": sum(m << (4 * i) for i, m in enumerate(masks)),
                    "sync_before": pl.sync}
            assert {k: got[k] for k in want} == want, (case.name, pos)
            assert (got["wave_task"] >= 0) == pl.task, (case.name, pos, got)
            assert (got["ncomb"] > 0) == pl.split, (case.name, pos, got)
            assert t.primary() == pl.primary
            if pl.primary >= 0:
                sp = F.seg_plan(t, case.wpc)
                assert (sp["split"], sp["ntiles"], len(sp["virt"])) == \
                    (pl.split, got["ntiles"], got["nvirt"]), (case.name, got)
        if case.path != "barrier":
            assert F.path_of(case.terms[0]) == case.path
        out = (ctypes.c_int32 * 10)()
        from mlx_mcmc_amd import _lib

        lib = _lib.load()
        for bad in (-1, len(case.terms)):
            assert lib.mc_debug_term_plan(p.handle, bad, out, 10) == _lib.MC_ERR_INVALID
        assert lib.mc_debug_term_plan(p.handle, 0, out, 9) == _lib.MC_ERR_INVALID
    finally:
        p.close()


def test_completeness():
    """Every (path label, attribute) pair the table must hold is there, and
    every size, wave count and weight: a deleted case cannot shrink the
    coverage silently."""
    have = {(c.path, a) for c in CASES for a in c.attrs}
    assert [r for r in F.REQUIRED if r not in have] == []
    every = set().union(*[c.attrs for c in CASES])
    assert [g for g in F.REQUIRED_GEOMETRY if g not in every] == []
    assert {c.path for c in CASES} >= set(F.labels())
    # thread-count tails (n mod 64 wpc != 0) at every wave count
    for wpc in (1, 4, 8):
        assert any(c.wpc == wpc and c.terms[0].n % (64 * wpc) for c in CASES), wpc
    # a wave task's twin at n = 65
    tasks = [c for c in CASES if "task" in c.attrs and len(c.terms) == 1]
    assert tasks and all(c.terms[0].n <= 64 for c in tasks)
    # one support-edge point per support-restricted distribution
    assert {c.terms[0].dist for c in CASES if c.edge is not None} == \
        {F.HALFNORMAL, F.EXPONENTIAL, F.GAMMA, F.BETA}
    for lab in F.labels():
        assert F.label_case(lab) is not None, lab


# ---- the JIT's pruning defines ---------------------------------------------------
def _source(h):
    from mlx_mcmc_amd import _lib

    lib = _lib.load()
    n = lib.mc_debug_expr_jit_source(h, None, 0)
    buf = ctypes.create_string_buffer(n + 1)
    lib.mc_debug_expr_jit_source(h, buf, n + 1)
    return buf.value.decode()


def _defines(src):
    return tuple(int(re.search(r"#define %s (\d+)u" % k, src).group(1))
                 for k in ("MC_JIT_PATHS", "MC_JIT_SU", "MC_JIT_DISTS"))


# compiled here without a device: every one (a compilation costs a second or two)
COMPILED = set(F.labels())


@pytest.mark.parametrize("label", F.labels())
def test_jit_defines_name_the_cases_path(label):
    """One case of the label plus a minimal expression term: the generated
    source names exactly that case's path and distribution (the expectation
    from _fused_terms.path_of, eval_term's dispatch restated, not from
    jit.hip), and compiles into k_hmc."""
    from mlx_mcmc_amd import _lib

    lib = _lib.load()
    case = F.label_case(label).with_expr()
    p = F.build(case, host_only=True)
    try:
        want = F.jit_defines(case.terms)
        assert _defines(_source(p.handle)) == want
        paths, su, dists = want
        assert bin(paths).count("1") + bin(su).count("1") == 1 and bin(dists).count("1") == 1
        assert (su == 1 << int(label[2:])) if label.startswith("su") else (su == 0)
        if label in COMPILED:
            kernel = f"mc::k_hmc<{case.wpc}, true, true>"
            rc = lib.mc_debug_expr_jit_compile(p.handle, kernel.encode())
            assert rc == 0, (lib.mc_last_error() or b"").decode()[:3000]
    finally:
        p.close()


def test_jit_defines_union_over_terms():
    """Two fused terms of different paths and distributions: both named."""
    a, b = F.by_name("su11_ps"), F.by_name("sx_gamma_beta")
    terms = [a.terms[0], b.terms[0]]     # (both over parameters from 0 on)
    case = F.Case("union", max(a.D, b.D), terms, "barrier").with_expr()
    p = F.build(case, host_only=True)
    try:
        assert _defines(_source(p.handle)) == (4, 1 << 11, (1 << F.HALFNORMAL) | (1 << F.GAMMA))
    finally:
        p.close()


# ---- sharpness ------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_bounds_are_sharp(case):
    """The float32 restatement stays within bounds() at every point; with one
    element dropped (the one of the largest log density), with any one pass's
    cotangents not deposited, and with one virtual segment left out of the
    split combination, it does not."""
    pts = F.points(case)
    for q in pts:
        lp, g = F.f32_logp_grad(case, q)
        assert F.within(case, q, lp, g)
    for q in (pts[0], pts[9]):
        l, _ = F.term_parts(case.terms[0], q, np.float64)
        i = int(np.argmax(np.abs(l)))
        assert not F.within(case, q, *F.f32_logp_grad(case, q, drop=i)), "dropped element"
        plan = case.plans[0]
        for ps in range(plan.npass if plan.npass > 1 else 0):
            assert not F.within(case, q, *F.f32_logp_grad(case, q, skip_pass=ps)), ("pass", ps)
        if plan.split:
            sp = F.seg_plan(case.terms[0], case.wpc)
            _, first, count = max(sp["groups"], key=lambda x: x[2])
            assert count > 1
            for vi in (first, first + count - 1):
                assert not F.within(case, q, *F.f32_logp_grad(case, q, skip_virtual=vi)), vi
