"""The reference side of tests/test_gpu_expr_lane_gather.py, on the CPU: the
float64 closed form (_lane_gather.glm_eval) equals float64 autograd of the same
log density, and the state test's bounds (_lane_gather.glm_bounds) are sharp
enough to see one observation: on the ragged varying-slopes data set, dropping
or doubling any single observation of any group moves log p, or that group's
alpha / beta gradient, by more than the bound the GPU test allows."""
import numpy as np
import pytest

import workloads as W
from _lane_gather import (HALF_LOG_2PI, glm_bounds, glm_eval, layout_of, poly_slopes, poly_spec,
                          ragged_slopes, slopes_spec, weighted_spec, weighted_start)

SPECS = {
    "slopes72": (lambda ns: ragged_slopes(ns, 72), lambda off, D: slopes_spec(72, off, D)),
    "poly3": (lambda ns: poly_slopes(ns, 40, 2600, nvec=3),
              lambda off, D: poly_spec(40, 2600, off, D, nvec=3)),
    "weighted": (lambda ns: (W.weighted_indexed(ns, 64, 2600)[0], weighted_start(64, 2600)),
                 lambda off, D: weighted_spec(64, 2600, off, D)),
}


def _point(name, seed=2):
    from mlx_mcmc_amd import _trace

    build, spec = SPECS[name]
    lp, init = build(W.ns_product())
    off, D = layout_of(lp, init)
    q = _trace.trace(lp, init).layout.flatten(init).astype(np.float32)
    q = q + np.random.default_rng(seed).normal(0.0, 0.05, D).astype(np.float32)
    return spec(off, D), q


def _torch_logp(spec, q):
    """The same log density written out in torch float64 (autograd)."""
    import torch

    t = lambda a: torch.tensor(np.asarray(a, np.float64))
    g = torch.tensor(spec["group"].astype(np.int64))
    G = spec["G"]
    m = torch.zeros(len(spec["y"]), dtype=torch.float64)
    for off, f in spec["vec"]:
        m = m + q[off:off + G][g] * t(f)
    for idx, f in spec["sh_mean"]:
        m = m + q[idx] * t(f)
    if spec["scale"][0] == "param":
        s = q[spec["scale"][1]]
    else:
        _, ils, ic, zf = spec["scale"]
        s = torch.exp(q[ils] + q[ic] * t(zf))
    lp = torch.sum(t(spec["w"]) * torch.distributions.Normal(m, s).log_prob(t(spec["y"])))
    for kind, off, n, loc, sc in spec["priors"]:
        x = q[off:off + n]
        if kind == "normal":
            mu = t(loc[1]) if loc[0] == "c" else q[loc[1]]    # (float64 constants)
            lp = lp + torch.sum(torch.distributions.Normal(mu, t(sc)).log_prob(x))
        else:
            lp = lp + torch.sum(np.log(2.0) - 0.5 * (x / sc) ** 2 - np.log(sc) - HALF_LOG_2PI)
    return lp


@pytest.mark.parametrize("name", list(SPECS))
def test_closed_form_equals_f64_autograd(name):
    import torch

    spec, q = _point(name)
    lp, g = glm_eval(spec, q)
    x = torch.tensor(q.astype(np.float64), requires_grad=True)
    tl = _torch_logp(spec, x)
    (tg,) = torch.autograd.grad(tl, x)
    assert abs(lp - tl.item()) <= 1e-11 * abs(tl.item())
    np.testing.assert_allclose(g, tg.numpy(), rtol=1e-10, atol=1e-10)
    # the magnitudes bound the values
    mlp, mg = glm_eval(spec, q, mags=True)
    assert mlp >= abs(lp) and np.all(mg >= np.abs(g) * (1 - 1e-12))


@pytest.mark.parametrize("times", [0, 2], ids=["dropped", "doubled"])
def test_bounds_see_one_observation(times):
    spec, q = _point("slopes72")
    N, G = len(spec["y"]), spec["G"]
    lp, g = glm_eval(spec, q)
    bl, bg = glm_bounds(spec, q)
    oa, ob = spec["vec"][0][0], spec["vec"][1][0]
    worst = np.inf
    seen = np.zeros(G, bool)
    for i in range(N):
        w = np.ones(N)
        w[i] = times
        lp2, g2 = glm_eval(spec, q, weights=w)
        k = spec["group"][i]
        ratio = max(abs(lp2 - lp) / bl, abs(g2[oa + k] - g[oa + k]) / bg[oa + k],
                    abs(g2[ob + k] - g[ob + k]) / bg[ob + k])
        worst = min(worst, ratio)
        seen[k] = True
        assert ratio > 1.0, (i, int(k), ratio)
    assert seen.sum() == np.count_nonzero(np.bincount(spec["group"], minlength=G))
    print(f"one observation {times}x: the least visible moves a checked quantity by "
          f"{worst:.1f} bounds")
