"""The first moment from per-run constants (lanes_fast.h lf_run_consts /
lf_m1), emulated in numpy float32 against float64 (tests/_lf_first_moment.py
has both forms), on the run patterns of tests/_lf_ends.py and
tests/_lf_rounds.py and one with every run under 16 elements, as they are and
with the observations shifted by +1e3 and +1e5:

  * |M1_new - M1_64| <= 2^-23 (n |c - theta| + |R|): one rounding each for
    c - theta, the fma and R;
  * that bound is never above the serial sum's share of _ragged.bounds,
    gamma(n + 1) sum |x - theta| (tighter than the gamma(n + 1 + C_GRAD_LOC)
    the gradient's bound allows it), and the old serial form is inside its own;
  * an uncentred (float) sum x - n theta is out of the new form's bound on
    the shifted data: the shifted cases can fail it;
  * the float32 gradient with the new M1 in it passes _ragged.check_state on
    the inputs of tests/test_gpu_lf_first_moment.py.
"""
import numpy as np
import pytest

import workloads as W
from _lf_first_moment import (PATTERNS, SHIFTS, bound_new, bound_serial, fma32, m1_f64, m1_new,
                              m1_serial, m1_uncentred, run_consts, runs_of, shifted_hier)
from _ragged import check_state, f32_logp_grad, perturbed_points

GPU_CASES = [("bench", "sorted", 0.0), ("r1_rem3", "shuffled", 0.0), ("r2_tail3", "sorted", 0.0),
             ("r6_exact", "shuffled", 0.0), ("short", "sorted", 0.0), ("bench", "sorted", 1e3)]


def _points(name, order, shift):
    _, init, data = shifted_hier(W.ns_oracle(), PATTERNS[name], order=order, shift=shift)
    return data, perturbed_points(init, n=4)


def test_fma32_rounds_once():
    # 2^24 + 1 is a tie of float32: the product's low bits decide it
    one, eps = np.float32(1.0), np.float32(2.0 ** -30)
    big = np.float32(2.0 ** 24)
    assert fma32(one, one, big) == big                       # tie to even
    assert fma32(np.float32(1.0) + np.float32(2.0 ** -23), one, big) == big + np.float32(2.0)
    assert fma32(eps, eps, one) == one
    assert fma32(np.float32(3.0), np.float32(5.0), np.float32(-15.0)) == 0.0


def test_run_consts_of_an_empty_and_a_single_run():
    assert run_consts(np.zeros(0, np.float32)) == (0.0, 0.0)
    c, R = run_consts(np.array([1234.5678], np.float32))
    assert c == np.float32(1234.5678) and R == 0.0
    assert m1_new(np.zeros(0, np.float32), 3.0) == 0.0


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_new_form_within_its_bound_and_the_serial_one(name, shift):
    worst = worst_rel = 0.0
    for order in ("sorted", "shuffled"):
        data, pts = _points(name, order, shift)
        runs = runs_of(data)
        for q in pts:
            for g, x in enumerate(runs):
                th = q[3 + g]
                ref = m1_f64(x, th)
                bn, bs = bound_new(x, th), bound_serial(x, th)
                en = abs(float(m1_new(x, th)) - ref)
                assert en <= bn, (name, order, shift, g, en, bn)
                assert bn <= bs, (name, order, shift, g, bn, bs)
                assert abs(float(m1_serial(x, th)) - ref) <= bs, (name, order, shift, g)
                if bn > 0:
                    worst = max(worst, en / bn)
                    worst_rel = max(worst_rel, bn / bs)
    print(f"{name} +{shift:g}: worst |err| / bound {worst:.3f}, worst bound / serial bound "
          f"{worst_rel:.3f}")


@pytest.mark.parametrize("shift", [s for s in SHIFTS if s])
def test_shifted_data_fail_an_uncentred_sum(shift):
    out = total = 0
    for name in ("bench", "r6_exact", "round6"):
        data, pts = _points(name, "sorted", shift)
        for q in pts:
            for g, x in enumerate(runs_of(data)):
                if len(x) == 0:
                    continue
                th = q[3 + g]
                total += 1
                out += abs(float(m1_uncentred(x, th)) - m1_f64(x, th)) > bound_new(x, th)
    print(f"+{shift:g}: {out} of {total} uncentred sums out of the bound")
    assert out > total // 2


@pytest.mark.parametrize("name,order,shift", GPU_CASES)
def test_gradient_with_the_new_form_inside_ragged_bounds(name, order, shift):
    """The float32 closed form with the new M1 in theta's gradient, within
    _ragged.bounds at the GPU test's inputs."""
    data, pts = _points(name, order, shift)
    runs = runs_of(data)
    for q in pts:
        lp, g = f32_logp_grad(data, q)
        mu, tau, sigma = q[0], q[1], q[2]
        iv = np.float32(1.0) / np.float32(sigma * sigma)
        it = np.float32(1.0) / np.float32(tau * tau)
        for k, x in enumerate(runs):
            th = q[3 + k]
            g[3 + k] = np.float32(m1_new(x, th) * iv) - np.float32(np.float32(th - mu) * it)
        check_state(q, g, lp, data, what=f"{name} {order} +{shift:g} new form")
