"""The second moment from per-run constants (lanes_fast.h lf_moments,
plan_lanes.hip lane_moments), emulated in numpy float32 against float64
(tests/_lf_second_moment.py derives the bound), on the run patterns of
tests/_lf_first_moment.py as they are and shifted by +1e3 and +1e5, at
positions 0.5 and 1.5 on either side of each run's mean:

  * |M2_new - M2_64| <= 2^-22 (Q + n d^2 + 2 |R d|);
  * two mutants — the 2 d R term dropped, and negated — leave that bound on
    the shifted data (there R, the residual of the rounded centre, is large
    enough to count; a run whose mean is a float32 has R = 0 and cannot tell
    them apart, so the assertion is on most runs of two or more elements);
  * the host planner's table (mc_debug_lane_moments) against the emulation:
    c, R and n bit-equal, Q within one float32 ulp of the float64 sum (a host
    compiler may contract its square-and-add), at one lane per parameter and
    at a planned rep > 1, where a lane's run is its part of its parameter's.
"""
import ctypes

import numpy as np
import pytest

import workloads as W
from _lf_first_moment import PATTERNS, SHIFTS, run_consts, runs_of, shifted_hier
from _lf_second_moment import OFFSETS, bound_m2, m2_f64, m2_new, q_const


def _runs(name, order, shift):
    _, _, data = shifted_hier(W.ns_oracle(), PATTERNS[name], order=order, shift=shift)
    return runs_of(data)


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_closed_form_within_its_bound(name, shift):
    worst = 0.0
    for order in ("sorted", "shuffled"):
        for g, x in enumerate(_runs(name, order, shift)):
            if len(x) == 0:
                assert m2_new(x, 1.0) == 0.0
                continue
            mean = float(np.mean(x.astype(np.float64)))
            for off in OFFSETS:
                th = np.float32(mean + off)
                err = abs(float(m2_new(x, th)) - m2_f64(x, th))
                b = bound_m2(x, th)
                assert err <= b, (name, order, shift, g, off, err, b)
                worst = max(worst, err / b)
    print(f"{name} +{shift:g}: worst |err| / bound {worst:.3f}")


@pytest.mark.parametrize("factor", [0.0, -2.0], ids=["dropped", "negated"])
def test_mutants_leave_the_bound_on_shifted_data(factor):
    for shift in SHIFTS:
        out = total = 0
        for name in ("bench", "short", "r6_exact"):
            for x in _runs(name, "sorted", shift):
                if len(x) < 2:
                    continue
                mean = float(np.mean(x.astype(np.float64)))
                for off in OFFSETS:
                    th = np.float32(mean + off)
                    total += 1
                    out += abs(float(m2_new(x, th, factor)) - m2_f64(x, th)) > bound_m2(x, th)
        print(f"2 d R x {factor:g}, +{shift:g}: {out} of {total} out of the bound")
        if shift == 1e3:
            assert out > total // 2, (factor, out, total)


def _host_table(lp, init, S):
    """(table [S, 4, 64, 4], rep) of the model's host-only lane plan on S slices."""
    from mlx_mcmc_amd import _lib, _trace

    model = _trace.trace(lp, init)
    lib = _lib.load()
    h = ctypes.c_void_p()
    data = np.ascontiguousarray(model.data, np.float32)
    index = np.ascontiguousarray(model.index, np.int32)
    lib.mc_debug_program_host_only(1)
    try:
        _lib.check(lib.mc_program_create_expr(
            model.c_terms, len(model.terms), model.c_affines, model.n_affines, model.c_exprs,
            model.n_exprs, model.c_nodes, model.n_nodes, model.layout.size, model.lp_const,
            data.ctypes.data_as(ctypes.c_void_p), data.size,
            index.ctypes.data_as(ctypes.c_void_p), index.size, ctypes.byref(h)))
    finally:
        lib.mc_debug_program_host_only(0)
    try:
        assert lib.mc_debug_lane_plan_host(h, S) == 0, (lib.mc_last_error() or b"").decode()
        n = lib.mc_debug_lane_moments(h, None, 0)
        assert n == S * 4 * 64 * 4, n
        out = np.zeros(n, np.float32)
        assert lib.mc_debug_lane_moments(h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                         n) == n
        return out.reshape(S, 4, 64, 4), int(lib.mc_program_lane_rep(h))
    finally:
        lib.mc_program_destroy(h)


def _check_table(table, parts):
    """The table's non-empty entries are the parts' constants, as multisets."""
    got = table.reshape(-1, 4)
    got = got[got[:, 3] > 0]
    assert np.all(table.reshape(-1, 4)[table.reshape(-1, 4)[:, 3] == 0] == 0)
    want = []
    for x in parts:
        if len(x) == 0:
            continue
        c, R = run_consts(x)
        want.append((float(len(x)), c, R, q_const(x, c)))
    assert len(got) == len(want), (len(got), len(want))
    key = lambda r: (r[0], r[1], r[2])  # noqa: E731
    got = sorted(((float(r[3]), r[0], r[1], r[2]) for r in got), key=key)
    want = sorted(want, key=key)
    for a, b in zip(got, want):
        assert a[0] == b[0], (a, b)
        assert np.float32(a[1]).tobytes() == np.float32(b[1]).tobytes(), (a, b)
        assert np.float32(a[2]).tobytes() == np.float32(b[2]).tobytes(), (a, b)
        q32 = np.float32(b[3])
        assert abs(float(a[3]) - b[3]) <= float(np.spacing(q32)), (a, b)


@pytest.mark.parametrize("name,shift", [("bench", 0.0), ("short", 1e3), ("r6_exact", 1e5)])
def test_host_table_one_lane_per_parameter(monkeypatch, name, shift):
    monkeypatch.setenv("MC_LANES_REP", "1")
    lp, init, data = shifted_hier(W.ns_product(), PATTERNS[name], order="shuffled", shift=shift)
    table, rep = _host_table(lp, init, 1)
    assert rep == 1
    _check_table(table, runs_of(data))


def test_host_table_at_a_planned_rep():
    G, N = W.SHAPES["small"]
    lp, init = W.hierarchical(W.ns_product(), G, N)
    y, group = W.hierarchical_data(G, N)
    table, rep = _host_table(lp, init, 2)
    assert rep > 1, rep
    parts = []
    for x in runs_of({"y": np.asarray(y, np.float32), "group": np.asarray(group), "G": G}):
        n, f = len(x), 0
        for k in range(rep):   # near-equal contiguous chunks over the lane group
            ln = n // rep + (1 if k < n % rep else 0)
            parts.append(x[f:f + ln])
            f += ln
    _check_table(table, parts)
