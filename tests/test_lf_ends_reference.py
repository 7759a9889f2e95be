"""tests/_lf_ends.py checked on the CPU (as tests/test_lf_rounds_reference.py
checks _lf_rounds.ROUNDS): each pattern has the run lengths its name stands
for, together they reach every case of the sweep's end, and the float64 check
of tests/test_gpu_lf_sweep_end.py can see one observation on each.

The derived log p bound (_ragged.bounds) at the model's init must stay below
one observation's contribution, log(2 pi) / 2 + log sigma = 0.919 at sigma = 1
(N is at most 1206, below _lf_rounds' round6, whose bound is 0.103).  This is
a condition on the patterns, not a measurement of any kernel: if a pattern
changes, it is re-checked here.
"""
import numpy as np
import pytest

import workloads as W
from _lf_ends import CASES, ENDS, NAMES, ORDERS, SET_GROUPS
from _ragged import (HALF_LOG_2PI, bounds, check_state, f32_logp_grad, perturbed_points,
                     ragged_hier, ref_logp_grad)


@pytest.mark.parametrize("name", NAMES)
def test_pattern_is_what_its_name_says(name):
    lengths, lmin4, rounds, rem, lmax = ENDS[name]
    nz = [x for x in lengths if x > 0]
    assert len(lengths) == 12 and len(nz) >= 11
    assert min(nz) // 4 == lmin4 and max(nz) == lmax
    assert lmin4 // 4 == rounds and lmin4 % 4 == rem
    for order in ORDERS[name]:
        _, _, data = ragged_hier(W.ns_oracle(), lengths, order=order)
        np.testing.assert_array_equal(np.bincount(data["group"], minlength=12), lengths)


def test_patterns_reach_every_end():
    P = ENDS.values()
    assert {p[2] for p in P} == {1, 2, 3, 4, 5, 6}          # full rounds: 0 / 1 / 2 trips, both parities
    assert {p[3] for p in P} == {0, 1, 2, 3}                # whole groups past the last round
    tails = {p[4] - 4 * p[1] for p in P}                    # elements past the shortest run's groups
    assert {0, 1, 3, 4, 8} <= tails
    # more groups past the last round than a register set of four holds, at
    # both parities of the round count (set A or set B idle over the last round)
    over = {p[2] % 2 for p in P if p[2] >= 2 and -(-p[4] // 4) - 4 * p[2] > SET_GROUPS}
    assert over == {0, 1}
    # and runs that end with the last round: nothing follows it in the tile
    assert any(p[4] == 16 * p[2] for p in P)
    assert any(min(x for x in p[0] if x > 0) % 4 for p in P)    # a shortest run not divisible by 4
    assert any(0 in p[0] for p in P)                            # an empty group
    assert {o for _, o in CASES} == {"sorted", "shuffled"}
    assert sorted(set(ENDS["bench"][0])) == [100, 101] and set(ORDERS["bench"]) == {"sorted", "shuffled"}


@pytest.mark.parametrize("name", NAMES)
def test_bound_is_below_one_observation(name):
    lengths = ENDS[name][0]
    _, init, data = ragged_hier(W.ns_oracle(), lengths)
    q0 = perturbed_points(init, n=1)[0]
    assert q0[2] == 1.0     # sigma at the init: an observation contributes log(2 pi) / 2
    bl, _ = bounds(data, q0)
    print(f"{name}: log p bound at the init {bl:.3f}")
    assert bl < HALF_LOG_2PI


@pytest.mark.parametrize("name,order", CASES)
def test_bounds_see_one_element(name, order):
    """A float32 evaluation that drops or doubles the last observation of a
    group — the end of a lane's run: a group not summed, summed twice, or an
    element masked wrongly — is out of bounds, in log p alone already; the
    unmutated one is in."""
    lengths = ENDS[name][0]
    _, init, data = ragged_hier(W.ns_oracle(), lengths, order=order)
    for q in perturbed_points(init, n=3):
        lp, g = f32_logp_grad(data, q)
        check_state(q, g, lp, data, what=f"{name} {order} float32")
        bl, _ = bounds(data, q)
        rl, _ = ref_logp_grad(data, q)
        for grp in np.nonzero(np.asarray(lengths) > 0)[0]:
            last = np.nonzero(data["group"] == grp)[0][-1]
            for mult in (0, 2):
                w = np.ones(len(data["y"]), np.float32)
                w[last] = mult
                mlp, mg = f32_logp_grad(data, q, weights=w)
                assert abs(float(mlp) - float(rl)) > bl, (name, grp, mult)
                with pytest.raises(AssertionError):
                    check_state(q, mg, mlp, data, what=f"{name} group {grp} x{mult}")
