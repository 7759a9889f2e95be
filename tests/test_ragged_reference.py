"""tests/_ragged.py checked on the CPU: the closed-form float64 reference
against autograd, and the derived bounds against mutants.

  * ref_logp_grad agrees with torch float64 autograd of the oracle-namespace
    model (oracle/ns.py with its constants and operands kept in float64) to
    1e-10 — relative to the sum of the terms' magnitudes, the only scale a sum
    that cancels (the gradient at a group mean) has — on every pattern, sorted
    and shuffled, with and without the scalar_mix terms;
  * the bounds are sharp enough to see one element: for every pattern and
    every non-empty group, a float32 evaluation that drops the group's last
    observation, counts it twice, or drops the last float4 of its run fails
    check_state, while the unmutated float32 evaluation passes.  A mutant
    moves log p by at least log(2 pi) / 2 + log sigma, above the log p bound
    at every pattern's N; the group's own gradient component sees it as well
    unless the dropped residual is ~0, so the test also asserts that
    component alone is out of its bound (runs of up to 128 elements).  Checked at _ragged.SEED = 0 (data)
    with the points of perturbed_points(seed=7): every group of every pattern
    holds.
"""
import numpy as np
import pytest

import workloads as W
from _ragged import (PATTERNS, bounds, check_state, f32_logp_grad, perturbed_points, ragged_hier,
                     ref_logp_grad, _evaluate)

EXTRAS = [None, "scalar_mix"]


@pytest.fixture
def ns64(monkeypatch):
    """The oracle namespace with its tensors in float64 (the same formulas)."""
    import torch

    from oracle import ns

    def _t(x):
        if isinstance(x, torch.Tensor):
            return x.double()
        return torch.as_tensor(np.asarray(x, dtype=np.float64))

    monkeypatch.setattr(ns, "_t", _t)
    return W.ns_oracle()


@pytest.mark.parametrize("extra", EXTRAS, ids=["plain", "scalar_mix"])
@pytest.mark.parametrize("order", ["sorted", "shuffled"])
@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_reference_matches_autograd(ns64, name, order, extra):
    import torch

    lp_fn, init, data = ragged_hier(ns64, PATTERNS[name], order=order, extra=extra)
    assert len(data["y"]) == sum(PATTERNS[name]) and data["G"] == len(PATTERNS[name])
    np.testing.assert_array_equal(np.bincount(data["group"], minlength=data["G"]),
                                  PATTERNS[name])
    for q in perturbed_points(init, n=3):
        x = torch.tensor(q.astype(np.float64), requires_grad=True)
        params, o = {}, 0
        for k, v in init.items():
            n = int(np.size(v))
            params[k] = x[o:o + n].reshape(np.shape(v))
            o += n
        lp = lp_fn(params)
        assert lp.dtype == torch.float64
        (g,) = torch.autograd.grad(lp, x)
        rl, rg = ref_logp_grad(data, q, extra)
        ml, mg = _evaluate(data, q, extra, np.float64, mags=True)
        assert abs(float(lp.detach()) - float(rl)) <= 1e-10 * float(ml)
        assert np.all(np.abs(g.numpy() - rg) <= 1e-10 * mg)


def test_shuffle_is_one_permutation():
    _, _, a = ragged_hier(W.ns_oracle(), PATTERNS["skew"])
    _, _, b = ragged_hier(W.ns_oracle(), PATTERNS["skew"], order="shuffled")
    assert np.any(np.diff(b["group"]) < 0), "unsorted"
    ka = sorted(zip(a["group"].tolist(), a["y"].tolist()))
    kb = sorted(zip(b["group"].tolist(), b["y"].tolist()))
    assert ka == kb


def _mutants(data, g):
    """Per-observation multiplicities of the three mutants of group g."""
    idx = np.nonzero(data["group"] == g)[0]          # the run, in element order
    n = len(idx)
    drop = np.ones(len(data["y"]), np.float32)
    drop[idx[-1]] = 0
    twice = np.ones(len(data["y"]), np.float32)
    twice[idx[-1]] = 2
    f4 = np.ones(len(data["y"]), np.float32)
    f4[idx[4 * ((n - 1) // 4):]] = 0
    return {"drop_last": drop, "count_twice": twice, "drop_float4": f4}


@pytest.mark.parametrize("extra", EXTRAS, ids=["plain", "scalar_mix"])
@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_bounds_see_one_element(name, extra):
    lp_fn, init, data = ragged_hier(W.ns_oracle(), PATTERNS[name], extra=extra)
    nsc = 4 if extra == "scalar_mix" else 3
    pts = perturbed_points(init, n=3)
    for k, q in enumerate(pts):
        lp, g = f32_logp_grad(data, q, extra)
        check_state(q, g, lp, data, extra, what=f"{name} float32")
        bl, bg = bounds(data, q, extra)
        rl, rg = ref_logp_grad(data, q, extra)
        for grp in np.nonzero(np.asarray(PATTERNS[name]) > 0)[0]:
            for kind, w in _mutants(data, int(grp)).items():
                mlp, mgr = f32_logp_grad(data, q, extra, weights=w)
                with pytest.raises(AssertionError):
                    check_state(q, mgr, mlp, data, extra, what=f"{name} {kind} group {grp}")
                # each of log p and the group's own gradient sees it alone: the
                # gradient away from row 0 (the group means, where the only
                # residual of a one-observation group is exactly 0) and on runs
                # of up to 128 elements (its bound grows with the run length
                # squared: ~1e-3 there, 0.03 at 700, where a residual below it
                # is no longer rare; log p still sees those)
                assert abs(float(mlp) - float(rl)) > bl, (name, kind, grp, "log p")
                j = nsc + int(grp)
                if k == 0 or PATTERNS[name][grp] > 128:
                    continue
                assert abs(float(mgr[j]) - float(rg[j])) > bg[j], (name, kind, grp, "gradient")
