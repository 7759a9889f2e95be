"""tests/_lf_rounds.py checked on the CPU (as tests/test_ragged_reference.py
checks _ragged.PATTERNS): each pattern has the run lengths its name stands
for, and the float64 check of tests/test_gpu_lf_sweep_pipeline.py can see one
observation on it.

The derived log p bound (_ragged.bounds) at the model's init must stay below
one observation's contribution, log(2 pi) / 2 + log sigma = 0.919 at sigma = 1.
At _ragged.SEED = 0 it is 0.034 (round3), 0.049 (round4), 0.086 (round5) and
0.103 (round6).  This is a condition on the patterns, not a measurement of any
kernel: if a pattern changes, it is re-checked here.
"""
import numpy as np
import pytest

import workloads as W
from _lf_rounds import NAMES, ROUNDS
from _ragged import (HALF_LOG_2PI, bounds, check_state, f32_logp_grad, perturbed_points,
                     ragged_hier, ref_logp_grad)


@pytest.mark.parametrize("name", NAMES)
def test_pattern_is_what_its_name_says(name):
    lengths, lmin4, rounds, lmax, n = ROUNDS[name]
    nz = [x for x in lengths if x > 0]
    assert len(lengths) == 12 and len(nz) >= 11
    assert min(nz) // 4 == lmin4 and lmin4 // 4 == rounds and max(nz) == lmax and sum(nz) == n
    # every remainder of whole groups the pattern can have past the last full
    # round (0 and 1), and every tail length 0 .. 7 past the shortest run
    assert {x // 4 - lmin4 for x in nz} == {0, 1}
    assert {x - 4 * lmin4 for x in nz} == set(range(8))
    _, _, data = ragged_hier(W.ns_oracle(), lengths, order="shuffled")
    np.testing.assert_array_equal(np.bincount(data["group"], minlength=12), lengths)


@pytest.mark.parametrize("name", NAMES)
def test_bound_is_below_one_observation(name):
    lengths = ROUNDS[name][0]
    _, init, data = ragged_hier(W.ns_oracle(), lengths)
    q0 = perturbed_points(init, n=1)[0]
    assert q0[2] == 1.0     # sigma at the init: an observation contributes log(2 pi) / 2
    bl, _ = bounds(data, q0)
    print(f"{name}: log p bound at the init {bl:.3f}")
    assert bl < HALF_LOG_2PI


@pytest.mark.parametrize("name", NAMES)
def test_bounds_see_one_element(name):
    """A float32 evaluation that drops or doubles the last observation of a
    group is out of bounds, in log p alone already; the unmutated one is in."""
    lengths = ROUNDS[name][0]
    _, init, data = ragged_hier(W.ns_oracle(), lengths)
    for q in perturbed_points(init, n=3):
        lp, g = f32_logp_grad(data, q)
        check_state(q, g, lp, data, what=f"{name} float32")
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
