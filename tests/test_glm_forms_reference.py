"""tests/_glm_forms.py without a device: its closed form against float64
autograd, the mc_glm record every form traces to, and the float32 closed form
inside the GPU gate at every input of tests/test_gpu_glm_forms.py."""
import numpy as np
import pytest

import _glm
import _glm_forms as F
from mlx_mcmc_amd import _lib, _trace

ALL_SHAPES = F.SHAPES + [F.WIDE]


def autograd64(f, d, q):
    import torch

    lay, _ = F.layout(f)
    lp_fn, _ = F.model(F.ns_torch64(), f, d)
    lps, gs = [], []
    for row in np.asarray(q, np.float64):
        t = torch.tensor(row, requires_grad=True)
        lp = lp_fn({k: (t[o:o + n] if f.shapes[k] else t[o]) for k, (o, n) in lay.items()})
        lp.backward()
        lps.append(lp.item())
        gs.append(t.grad.numpy())
    return np.array(lps), np.array(gs)


@pytest.mark.parametrize("N,P,C,S", ALL_SHAPES)
@pytest.mark.parametrize("family,name", F.CASES)
def test_closed_form_is_float64_autograd(family, name, N, P, C, S):
    f, d = F.form(name, family, P), F.data(family, N, P)
    q = F.points(f, min(C, 7))
    lp, g = F.closed_form(f, d, q)
    alp, ag = autograd64(f, d, q)
    np.testing.assert_allclose(lp, alp, rtol=1e-10)
    np.testing.assert_allclose(g, ag, rtol=1e-10, atol=1e-12)
    if name == "sliced":
        u = F.layout(f)[0]["u"][0]
        assert np.all(g[:, u] == 0.0) and np.all(ag[:, u] == 0.0)


@pytest.mark.parametrize("kind,level", F.SATURATION)
def test_closed_form_is_float64_autograd_when_saturated(kind, level):
    f, d, q = F.saturated(kind, level, 33, 3, 5)
    lp, g = F.closed_form(f, d, q)
    alp, ag = autograd64(f, d, q)
    np.testing.assert_allclose(lp, alp, rtol=1e-10)
    np.testing.assert_allclose(g, ag, rtol=1e-10, atol=1e-12 * np.abs(ag).max())


def test_plain_is_the_form_of_glm_py():
    for family in _glm.FAMILIES:
        d = _glm.data(family, 33, 3)
        f = F.form("plain", family, 3)
        q = F.points(f, 5)
        for a, b in zip(F.closed_form(f, d, q), _glm.closed_form(d, q)):
            np.testing.assert_allclose(a, b, rtol=1e-12)


NONE, CONST, PSC = _lib.MC_OP_NONE, _lib.MC_OP_CONST, _lib.MC_OP_PSCALAR
# form: intercept (kind, parameter offset), beta_offset, offset pool on (normal,
# bernoulli, poisson), priors (+ 1 on the normal family's log_sigma where marked),
# the normal family's scale (kind, transform, parameter offset); P = 3
RECORDS = {
    "bare": ((NONE, 0), 0, (0, 0, 0), 1, 0, (CONST, _lib.MC_XF_NONE, 0)),
    "const": ((CONST, 0), 0, (1, 1, 1), 1, 0, (CONST, _lib.MC_XF_NONE, 0)),
    "const_nooff": ((CONST, 0), 0, (0, 0, 0), 1, 0, None),
    "sliced": ((PSC, 6), 2, (0, 0, 1), 4, 1, (PSC, _lib.MC_XF_EXP, 8)),
    "rawscale": ((PSC, 0), 1, (0, 0, 0), 3, 0, (PSC, _lib.MC_XF_NONE, 4)),
    "priors_a": ((PSC, 0), 1, (0, 0, 1), 8, 0, (PSC, _lib.MC_XF_EXP, 4)),
    "priors_b": ((PSC, 6), 0, (0, 0, 0), 7, 0, (PSC, _lib.MC_XF_NONE, 3)),
}


@pytest.mark.parametrize("family,name", F.CASES)
def test_every_form_traces_to_its_glm_record(family, name):
    f, d = F.form(name, family, 3), F.data(family, 33, 3)
    model = _trace.trace(*F.model(F.ns_product(), f, d))
    g = model.c_glm
    icpt, boff, off, n_priors, on_sigma, scale = RECORDS[name]
    k = _glm.FAMILIES.index(family)
    assert g.family == _trace.GLM_FAMILIES[family.capitalize()] and (g.n, g.p) == (33, 3)
    assert g.intercept.kind == icpt[0] and g.beta_offset == boff
    if icpt[0] == PSC:
        assert (g.intercept.param_offset, g.intercept.transform) == (icpt[1], _lib.MC_XF_NONE)
    if icpt[0] == CONST:
        assert g.intercept.value == np.float32(F.A_CONST)
    assert g.offset_pool == (132 if off[k] else -1)
    if off[k]:
        np.testing.assert_array_equal(model.data[132:165], d.off)
    assert len(model.terms) == n_priors + (on_sigma if family == "normal" else 0)
    assert model.n_exprs == 0 and model.layout.size == F.layout(f)[1]
    if family == "normal":
        assert g.scale.kind == scale[0]
        if scale[0] == PSC:
            assert (g.scale.transform, g.scale.param_offset) == scale[1:]
        else:
            assert g.scale.value == np.float32(F.SIGMA_CONST)


def test_the_prior_forms_cover_the_prior_table():
    """priors_a and priors_b between them: every dist from Normal to Identity,
    the EXP and LOG value transforms, a weight other than 1, a prior on a
    sub-range of beta, two priors on the same elements."""
    terms = []
    for name in ("priors_a", "priors_b"):
        f, d = F.form(name, "bernoulli", 3), F.data("bernoulli", 33, 3)
        model = _trace.trace(*F.model(F.ns_product(), f, d))
        boff = model.c_glm.beta_offset
        terms += [(t.dist, t.value.transform, t.weight, t.value.param_offset - boff, t.n)
                  for t in model.terms]
    assert {t[0] for t in terms} == set(range(_lib.MC_DIST_NORMAL, _lib.MC_DIST_IDENTITY + 1))
    assert {t[1] for t in terms} == {_lib.MC_XF_NONE, _lib.MC_XF_EXP, _lib.MC_XF_LOG}
    assert {0.5, 2.0, 0.25, -1.0} <= {t[2] for t in terms}
    assert (_lib.MC_DIST_NORMAL, 0, 0.5, 1, 2) in terms
    assert (_lib.MC_DIST_NORMAL, 0, 1.0, 0, 3) in terms
    assert sum(1 for t in terms if t[3:] == (0, 1)) == 2


@pytest.mark.parametrize("family,bad", [("bernoulli", 0.5), ("poisson", 2.5), ("poisson", -1.0)])
def test_an_observation_outside_the_support_traces(family, bad):
    """The tracer takes such a y (the kernels give log p = -inf and no residual:
    tests/test_gpu_glm_forms.py), and the closed form says the same."""
    f, d = F.form("plain", family, 3), _glm.data(family, 33, 3)
    d.y[7] = bad
    model = _trace.trace(*F.model(F.ns_product(), f, d))
    assert model.c_glm.family == _trace.GLM_FAMILIES[family.capitalize()]
    assert model.data[99 + 7] == np.float32(bad)
    lp, g = F.closed_form(f, d, F.points(f, 5))
    assert np.all(lp == -np.inf) and np.isfinite(g).all()


def test_float32_closed_form_is_inside_the_gpu_gate(capsys):
    """Every input of tests/test_gpu_glm_forms.py: the form matrix at its three
    shapes and the saturated inputs at two.  Prints the worst fractions of the
    bound, which the GPU tests' docstrings quote."""
    worst = {}

    def hold(key, f, d, q):
        rlp, rg = F.closed_form(f, d, q)
        lp, g = F.closed_form(f, d, q, np.float32)
        assert lp.dtype == np.float32 and g.dtype == np.float32
        flp, fg = F.gate_fractions(lp, g, rlp, rg)
        assert flp < 1.0 and fg < 1.0, (key, flp, fg)
        a, b = worst.get(key, (0.0, 0.0))
        worst[key] = (max(a, flp), max(b, fg))

    for family, name in F.CASES:
        for N, P, C, S in ALL_SHAPES:
            f = F.form(name, family, P)
            hold("forms", f, F.data(family, N, P), F.points(f, C))
    for N, P, C in ((33, 3, 290), (97, 33, 290), (33, 129, 290)):
        for family in _glm.FAMILIES:
            f = F.form("sliced", family, P)
            hold("chunks", f, F.data(family, N, P), F.points(f, C))
    for kind, level in F.SATURATION:
        for N, P, C, S in F.SHAPES:
            hold(f"{kind} {level:g}", *F.saturated(kind, level, N, P, C))
    with capsys.disabled():
        for key, (flp, fg) in worst.items():
            print(f"\nfloat32 closed form, {key}: worst lp {flp:.3f} of the bound, "
                  f"worst gradient {fg:.3f}", end="")
        print()
