"""The per-op table of tests/_expr_ops.py held to something independent of it
(CPU only): its float64 values and VJPs agree with torch float64 autograd of
the same op on the bulk domain, and its builders trace — without a device —
into programs whose expression term ends in the intended op over the intended
leaf kinds.  tests/test_gpu_expr_ops.py then holds the kernels to the table."""
import numpy as np
import pytest
import torch

import _expr_ops as X

TORCH = X.torch_ops()

# The table's deliberate departures from autograd: (op, argument) -> reason.
# These cotangents are not compared.
SKIPS = {
    ("gamma_lp", 1): "the shape's gammaln normaliser is a host constant of the current value "
                     "(gamma.py:48-59): log b + log v, no digamma",
    ("beta_lp", 1): "log B(a, b) is a host constant (beta.py:45-57): log v, no digamma",
    ("beta_lp", 2): "log B(a, b) is a host constant (beta.py:45-57): log(1 - v), no digamma",
}
# pow's exponent cotangent is the documented v log x; torch masks it where
# x == 0 (and returns NaN-free values for x < 0 with integer y).  The two
# differ only off the bulk domain (x > 0 there), so the bulk comparison keeps
# it; the edge behaviour is the GPU test's.


def _lg(a):
    return np.abs(torch.lgamma(torch.tensor(a)).numpy())


# rtol 1e-12 holds each figure to autograd's.  Where a formula is a difference
# of larger float64 terms, the float64 rounding of those terms (4 eps of their
# magnitudes' sum) is an absolute floor: 1 - v^2 of a saturated tanh, and a
# log density whose summands cancel.  name -> that sum (of float64 inputs).
_L = lambda t: np.abs(np.log(t))   # noqa: E731
TERMS = {
    "tanh": lambda x: np.ones_like(x),
    "normal_lp": lambda v, m, s: 1.0 + _L(s) + ((v - m) / s) ** 2,
    "halfnormal_lp": lambda v, s: 1.0 + _L(s) + (v / s) ** 2,
    "exponential_lp": lambda v, r: _L(r) + r * v,
    "gamma_lp": lambda v, a, b: a * _L(b) + _lg(a) + np.abs(a - 1) * _L(v) + b * v,
    "beta_lp": lambda v, a, b: (np.abs(a - 1) * _L(v) + np.abs(b - 1) * _L(1 - v) + _lg(a) + _lg(b)
                                + _lg(a + b)),
}


@pytest.mark.parametrize("name", X.OPS)
def test_table_matches_float64_autograd(name):
    args = X.bulk(name)
    diff = X.diff_args(name)
    t = [torch.tensor(np.asarray(a, np.float64), requires_grad=(i in diff))
         for i, a in enumerate(args)]
    out = TORCH[name](*t)
    grads = torch.autograd.grad(out.sum(), [t[i] for i in diff])
    floor = 0.0
    if name in TERMS:
        floor = 4 * np.finfo(np.float64).eps * TERMS[name](*[np.asarray(a, np.float64) for a in args])
    fwd = X.fwd64(name, *args)
    assert np.all(np.abs(fwd - out.detach().numpy()) <= 1e-12 * np.abs(fwd)
                  + (0.0 if name == "tanh" else floor)), name
    vj = X.vjp64(name, *args, round_v=False)
    assert len(vj) == len(diff)
    for j, i in enumerate(diff):
        if (name, i) in SKIPS:
            continue
        ref = grads[j].numpy()
        assert np.all(np.abs(vj[j] - ref) <= 1e-12 * np.abs(ref)
                      + (floor if name == "tanh" else 0.0)), (name, i)


def test_skipped_cotangents_are_the_documented_ones():
    """What SKIPS leaves uncompared is stated here instead: the shape
    cotangents are autograd's plus the digamma terms autograd adds."""
    v, a, b = X.bulk("gamma_lp")
    a64 = torch.tensor(np.asarray(a, np.float64))
    np.testing.assert_allclose(X.vjp64("gamma_lp", v, a, b)[1],
                               np.log(np.float64(b)) + np.log(np.float64(v)), rtol=1e-15)
    v, a, b = X.bulk("beta_lp")
    t = [torch.tensor(np.asarray(x, np.float64), requires_grad=True) for x in (v, a, b)]
    g = torch.autograd.grad(TORCH["beta_lp"](*t).sum(), t)
    dg = lambda x: torch.digamma(x).numpy()   # noqa: E731
    a64, b64 = t[1].detach(), t[2].detach()
    vj = X.vjp64("beta_lp", v, a, b)
    np.testing.assert_allclose(vj[1], g[1].numpy() + dg(a64) - dg(a64 + b64), rtol=1e-9)
    np.testing.assert_allclose(vj[2], g[2].numpy() + dg(b64) - dg(a64 + b64), rtol=1e-9)


def test_float32_evaluation_follows_the_reference():
    """fwd32 / vjp32 are the same formulas kept in float32: float32 results,
    equal to the rounded reference for the single-operation ops, and on the
    bulk domain within 8 ulp (in `units`) of the reference everywhere: a
    handful of float32 roundings."""
    for name in X.OPS:
        args = X.bulk(name, 256)
        if name in X.EXACT:
            np.testing.assert_array_equal(X.fwd32(name, *args),
                                          X.fwd64(name, *args).astype(np.float32))
        assert X.fwd32(name, *args).dtype == np.float32
        uf, ug = X.units(name, *args)
        assert np.all(np.abs(X.fwd32(name, *args) - X.fwd64(name, *args)) <= 8 * uf), name
        slack = X.vjp_slack(name, args, 8.0)
        for g32, g64, u, sl in zip(X.vjp32(name, *args), X.vjp64(name, *args), ug, slack):
            assert np.all(np.abs(g32 - g64) <= 8 * u + sl), name
        assert all(g.dtype == np.float32 for g in X.vjp32(name, *args))


def test_bulk_domains_are_fixed_and_legal():
    for name in X.OPS:
        a, b = X.bulk(name), X.bulk(name)
        assert len(a) == X.arity(name)
        for x, y in zip(a, b):
            assert x.dtype == np.float32 and x.shape == (X.P_BULK,)
            np.testing.assert_array_equal(x, y)
        v = X.fwd64(name, *a)
        assert np.all(np.isfinite(v)), name
        f = np.abs(v[v != 0])
        assert np.all((f > 1e-37) & (f < 1e37)), name
        for g in X.vjp64(name, *a):
            assert np.all(np.isfinite(g)), name
        e = X.edges(name)
        assert len(e) == X.arity(name) and len({len(c) for c in e}) == 1


@pytest.mark.parametrize("name", X.OPS)
def test_builders_trace_to_the_intended_root(name):
    """The host tables of each form, and with them the path it takes: the
    engine picks the path from these tables alone.  A term of n <= 64
    elements in one pass without a parameter-vector leaf is a wave task
    (csrc/program.hip, "small terms ... run as wave tasks"): form S, n = 1
    over PSCALAR leaves.  A term of at most 16 nodes runs eval_expr_n's
    NMAX = 16 instantiation, a larger one NMAX = 32 (csrc/eval.h): forms V
    and V32.  The library has no query for the path a launch took."""
    from mlx_mcmc_amd import _lib

    k, diff = X.arity(name), X.diff_args(name)
    data = [np.linspace(0.1, 0.9, X.N_VEC).astype(np.float32)] * k
    if name != "where":
        m = X.traced(X.build_S(name))        # (asserts the root)
        assert m.terms[0].n == 1 and m.layout.size == k
        assert X.leaf_kinds(m) == [_lib.MC_OP_PSCALAR] * k
    m = X.traced(X.build_V(name, data))
    assert m.terms[0].n == X.N_VEC and m.layout.size == len(diff) * X.N_VEC
    kinds = X.leaf_kinds(m)
    assert kinds.count(_lib.MC_OP_PVEC) == len(diff) and kinds.count(_lib.MC_OP_DATA) == k - len(diff)
    assert len(X.node_ops(m)) <= 16
    m32 = X.traced(X.build_V(name, data, "V32"))
    ops32 = X.node_ops(m32)
    assert 16 < len(ops32) <= _lib.MC_EXPR_MAX_NODES and ops32.count(_lib.MC_EX_MUL) >= 17
    assert X.leaf_kinds(m32).count(_lib.MC_OP_CONST) == 1
    mf = X.traced(X.build_V(name, data, "VF"))
    assert X.node_ops(mf)[-1] == _lib.MC_EX_MUL and mf.layout.size == (len(diff) + 1) * X.N_VEC


def test_op_codes_are_the_header_s():
    from mlx_mcmc_amd import _lib

    for name in X.OPS:
        assert X.code(name) == getattr(_lib, "MC_EX_" + name.upper())
    assert sorted(X.code(n) for n in X.OPS) == list(range(1, 25))
