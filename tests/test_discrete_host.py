"""Bernoulli / Binomial / Poisson without a device: the float64 node table
against torch autograd, op codes, the tracer's lowering, the ABI's validation,
the host samplers (mc_predictive_draw_discrete, csrc/predictive.h) against the
NumPy restatement and scipy.stats, and the merge of partials with ``equal``."""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy import special as spsp
from scipy import stats as sps

import _discrete as DS
import _predictive as PP
from mlx_mcmc_amd import _lib, _trace, diagnostics as D
from test_abi import _expr_program
from test_predictive_host import _triples

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
L = _lib.MC_EX_LEAF


# ---- the node table -----------------------------------------------------------------
@pytest.mark.parametrize("name", list(DS.OP))
def test_node_table_equals_torch_autograd(name):
    import torch

    rng = np.random.default_rng(3)
    P = 512
    eta = DS.X._logu(rng, P, 1e-3, 15.0 if name == "poisson" else 30.0, True)
    if name == "bernoulli":
        y, n = rng.integers(0, 2, P).astype(F32), np.zeros(P, F32)
    elif name == "binomial":
        n = rng.integers(0, 40, P).astype(F32)
        y = np.floor(rng.random(P) * (n + 1)).astype(F32)
    else:
        y, n = rng.integers(0, 30, P).astype(F32), np.zeros(P, F32)
    te = torch.tensor(eta.astype(np.float64), requires_grad=True)
    val = DS.torch_node(name)(torch.tensor(y.astype(np.float64)),
                              torch.tensor(n.astype(np.float64)), te)
    val.sum().backward()
    np.testing.assert_allclose(DS.fwd64(name, y, n, eta), val.detach().numpy(), rtol=1e-12,
                               atol=1e-300)
    # (y - sigma cancels where sigma is near y: absolute in units of the terms)
    np.testing.assert_allclose(DS.vjp64(name, y, n, eta), te.grad.numpy(), rtol=1e-11,
                               atol=1e-13 * (1.0 + float(np.abs(n).max())))


def test_out_of_support_and_edges_of_the_table():
    inf, nan = np.inf, np.nan
    assert DS.fwd64("bernoulli", 2.0, None, 0.3) == -inf and DS.vjp64("bernoulli", 2.0, None, 0.3) == 0
    assert DS.fwd64("binomial", 8.0, 7.0, 0.3) == -inf and DS.fwd64("binomial", 2.5, 7.0, 0.3) == -inf
    assert DS.fwd64("binomial", 1.0, 6.5, 0.3) == -inf and DS.fwd64("binomial", 0.0, 0.0, 0.3) == 0
    assert DS.fwd64("poisson", -1.0, None, 0.3) == -inf and DS.fwd64("poisson", 2.5, None, 0.3) == -inf
    # the classes the header states for infinite arguments
    assert DS.fwd32("bernoulli", 1.0, None, inf) == 0 and DS.fwd32("bernoulli", 0.0, None, inf) == -inf
    assert np.isnan(DS.fwd32("binomial", 3.0, 7.0, inf)) and np.isnan(DS.fwd32("binomial", 0.0, 7.0, -inf))
    assert DS.fwd32("binomial", 3.0, 7.0, -inf) == -inf
    assert DS.fwd32("poisson", 0.0, None, -inf) == 0 and DS.fwd32("poisson", 3.0, None, -inf) == -inf
    assert DS.fwd32("poisson", 0.0, None, inf) == -inf and np.isnan(DS.fwd32("poisson", 3.0, None, inf))
    for name in DS.OP:
        assert np.isnan(DS.fwd32(name, 1.0, 7.0, nan))
    # no 0 * -inf at saturation, where the hand-written form has it
    assert np.isfinite(DS.fwd32("bernoulli", 1.0, None, 90.0))
    assert DS.fwd32("bernoulli", 0.0, None, 90.0) == F32(-90.0)


def test_op_codes_equal_the_header():
    text = open(os.path.join(ROOT, "include", "mcmc355.h")).read()
    for name, code in (("MC_EX_BERNOULLI_LOGIT_LP", 25), ("MC_EX_BINOMIAL_LOGIT_LP", 26),
                       ("MC_EX_POISSON_LOG_LP", 27)):
        assert re.search(rf"\b{name}\s*=\s*{code}\b", text), name
        assert getattr(_lib, name) == code
    assert DS.OP == {"bernoulli": 25, "binomial": 26, "poisson": 27}
    for k, name in enumerate(("BERNOULLI", "BINOMIAL", "POISSON")):
        assert re.search(rf"\bMC_DISCRETE_{name}\s*=\s*{k}\b", text)
        assert getattr(_lib, f"MC_DISCRETE_{name}") == k
    assert re.search(r"#define\s+MC_ABI_VERSION\s+2\b", text)


# ---- the tracer -----------------------------------------------------------------------
def _nodes(lp, init):
    model = _trace.trace(lp, init, keep_order=True)
    assert len(model.terms) == 1 and model.terms[0].dist == _lib.MC_DIST_EXPR
    return model, [(model.c_nodes[i].op, model.c_nodes[i].leaf.kind) for i in range(model.n_nodes)]


def test_tracer_natural_parameterisations():
    import mlx_mcmc_amd as m
    import mlx_mcmc_amd.core as mx

    d = DS.data()
    init = {"a": F32(0.1), "b": F32(0.2)}
    model, nodes = _nodes(lambda p: mx.sum(m.Bernoulli(logits=p["a"] + p["b"] * d.x).log_prob(d.yb)),
                          init)
    ops = [o for o, _ in nodes]
    assert ops[-1] == 25 and ops.count(25) == 1              # root: the node itself
    root = model.c_nodes[model.n_nodes - 1]
    assert nodes[root.a] == (L, _lib.MC_OP_DATA)              # y: a data leaf
    model, nodes = _nodes(lambda p: mx.sum(m.Poisson(log_rate=p["a"] + p["b"] * d.x).log_prob(d.yp)),
                          init)
    root = model.c_nodes[model.n_nodes - 1]
    assert root.op == _lib.MC_EX_ADD and model.c_nodes[root.a].op == 27
    assert nodes[root.b] == (L, _lib.MC_OP_DATA)              # the normaliser leaf
    np.testing.assert_array_equal(
        model.data[model.c_nodes[root.b].leaf.pool_offset:][:d.N],
        (-spsp.gammaln(d.yp.astype(np.float64) + 1)).astype(F32))
    assert nodes[model.c_nodes[root.a].a] == (L, _lib.MC_OP_DATA)
    init = {"alpha": np.zeros(d.G, F32), "b": F32(0.2)}
    model, nodes = _nodes(lambda p: mx.sum(
        m.Binomial(d.nt, logits=p["alpha"][d.g] + p["b"] * d.x).log_prob(d.ybin)), init)
    root = model.c_nodes[model.n_nodes - 1]
    node = model.c_nodes[root.a]
    assert root.op == _lib.MC_EX_ADD and node.op == 26
    assert nodes[node.a] == (L, _lib.MC_OP_DATA) and nodes[node.b] == (L, _lib.MC_OP_DATA)
    ny, nn = d.ybin.astype(np.float64), d.nt.astype(np.float64)
    want = spsp.gammaln(nn + 1) - spsp.gammaln(ny + 1) - spsp.gammaln(nn - ny + 1)
    np.testing.assert_array_equal(model.data[model.c_nodes[root.b].leaf.pool_offset:][:d.N],
                                  want.astype(F32))
    # scalar data: CONST leaves, the normaliser among them
    model, nodes = _nodes(lambda p: m.Poisson(log_rate=p["a"]).log_prob(3.0), {"a": F32(0.1)})
    root = model.c_nodes[model.n_nodes - 1]
    assert nodes[root.b] == (L, _lib.MC_OP_CONST)
    assert model.c_nodes[root.b].leaf.value == F32(-spsp.gammaln(4.0))
    assert nodes[model.c_nodes[root.a].a] == (L, _lib.MC_OP_CONST)
    # outside the support the leaf is 0 (the node gives -inf)
    z = _trace.discrete_norm("Poisson", np.array([2.0, -1.0, 2.5], F32))
    np.testing.assert_array_equal(z, np.array([-spsp.gammaln(3.0), 0.0, 0.0], F32))
    z = _trace.discrete_norm("Binomial", np.array([2.0, 8.0], F32), np.array([7.0, 7.0], F32))
    assert z[1] == 0 and z[0] == F32(np.log(21.0))


def _eval(root, values):
    """The traced expression on the host in float32 with the table's nodes."""
    E = _trace.Expr

    def ev(e):
        if e.op == L:
            return values[e.leaf.name] if isinstance(e.leaf, _trace.Param) else np.asarray(e.leaf, F32)
        a = [None if x is None else ev(x) for x in e.args]
        if e.op in DS.OP.values():
            name = {v: k for k, v in DS.OP.items()}[e.op]
            return DS.fwd32(name, a[0], a[1] if name == "binomial" else None, a[-1])
        with np.errstate(all="ignore"):
            return {_lib.MC_EX_ADD: lambda: a[0] + a[1], _lib.MC_EX_SUB: lambda: a[0] - a[1],
                    _lib.MC_EX_NEG: lambda: -a[0], _lib.MC_EX_LOG: lambda: np.log(a[0]),
                    _lib.MC_EX_LOG1P: lambda: np.log1p(a[0]),
                    _lib.MC_EX_GT: lambda: (a[0] > a[1]).astype(F32),
                    _lib.MC_EX_LT: lambda: (a[0] < a[1]).astype(F32),
                    _lib.MC_EX_WHERE: lambda: np.where(a[0] != 0, a[1], a[2]).astype(F32)}[e.op]()
    assert isinstance(root, E)
    return ev(root)


def test_tracer_probs_and_rate_lowering():
    import mlx_mcmc_amd as m

    y = np.array([1.0, 0.0, 1.0], F32)
    n = np.array([4.0, 4.0, 4.0], F32)
    P = _trace.Param("p", 0, ())
    for dist, yy in ((m.Bernoulli(probs=P), y), (m.Binomial(n, probs=P), y)):
        root = dist.log_prob(yy).terms[0].expr
        assert root.op == _lib.MC_EX_WHERE
        for bad in (0.0, 1.0, -0.1, 1.5):
            assert np.all(_eval(root, {"p": F32(bad)}) == -np.inf), bad
        got = _eval(root, {"p": F32(0.3)})
        ref = (sps.bernoulli(0.3).logpmf(yy) if isinstance(dist, m.Bernoulli)
               else sps.binom(4, 0.3).logpmf(yy))
        np.testing.assert_allclose(got, ref, rtol=2e-6)
    R = _trace.Param("r", 0, ())
    root = m.Poisson(rate=R).log_prob(np.array([0.0, 3.0], F32)).terms[0].expr
    for bad in (0.0, -2.0):
        assert np.all(_eval(root, {"r": F32(bad)}) == -np.inf)
    np.testing.assert_allclose(_eval(root, {"r": F32(2.5)}), sps.poisson(2.5).logpmf([0, 3]),
                               rtol=2e-6)


def test_tracer_rejects_traced_counts_and_bad_parameterisations():
    import mlx_mcmc_amd as m

    P = _trace.Param("p", 0, ())
    with pytest.raises(_trace.TraceError):
        m.Poisson(log_rate=0.3).log_prob(P)
    with pytest.raises(_trace.TraceError):
        m.Bernoulli(logits=P).log_prob(P)
    with pytest.raises(_trace.TraceError):
        m.Binomial(P, logits=0.2).log_prob(1.0)
    for make in (lambda: m.Bernoulli(), lambda: m.Bernoulli(probs=0.2, logits=0.1),
                 lambda: m.Binomial(3), lambda: m.Binomial(3, probs=0.2, logits=0.1),
                 lambda: m.Poisson(), lambda: m.Poisson(rate=1.0, log_rate=0.0)):
        with pytest.raises(ValueError):
            make()
    assert set(("Bernoulli", "Binomial", "Poisson")) <= set(m.__all__)
    assert repr(m.Poisson(rate=3.0)) == "Poisson(rate=3.000)"
    assert repr(m.Binomial(10, probs=0.25)) == "Binomial(total_count=10.000, probs=0.250)"
    np.testing.assert_allclose(m.Binomial(10, probs=0.25).mean(), 2.5)
    np.testing.assert_allclose(m.Binomial(10, probs=0.25).variance(), 1.875)
    np.testing.assert_allclose(m.Bernoulli(logits=0.0).mean(), 0.5)
    np.testing.assert_allclose(m.Poisson(log_rate=0.0).variance(), 1.0)
    s = m.Poisson(rate=4.0).sample(m.random.key(3), (500,))
    assert s.dtype == F32 and s.shape == (500,) and abs(s.mean() - 4.0) < 0.5
    s = m.Binomial(12, logits=0.0).sample(m.random.key(3), (500,))
    assert np.all((s >= 0) & (s <= 12) & (s == np.floor(s))) and abs(s.mean() - 6.0) < 0.5
    s = m.Bernoulli(probs=0.2).sample(m.random.key(3), (500,))
    assert set(np.unique(s)) <= {0.0, 1.0}


# ---- the ABI ------------------------------------------------------------------------------
P0 = {"kind": _lib.MC_OP_PSCALAR, "param_offset": 0}
P1 = {"kind": _lib.MC_OP_PSCALAR, "param_offset": 1}
DATA = {"kind": _lib.MC_OP_DATA, "pool_offset": 0}


@pytest.mark.parametrize("nodes,code,msg", [
    # a parameter leaf as y / as n
    ([(L, -1, -1, -1, P0), (L, -1, -1, -1, P1), (25, 0, 1, -1, None)], _lib.MC_ERR_UNSUPPORTED,
     b"Bernoulli node's count y"),
    ([(L, -1, -1, -1, P0), (L, -1, -1, -1, P1), (27, 0, 1, -1, None)], _lib.MC_ERR_UNSUPPORTED,
     b"Poisson node's count y"),
    ([(L, -1, -1, -1, DATA), (L, -1, -1, -1, P0), (L, -1, -1, -1, P1), (26, 0, 1, 2, None)],
     _lib.MC_ERR_UNSUPPORTED, b"Binomial node's total n"),
    ([(L, -1, -1, -1, P0), (L, -1, -1, -1, DATA), (L, -1, -1, -1, P1), (26, 0, 1, 2, None)],
     _lib.MC_ERR_UNSUPPORTED, b"Binomial node's count y"),
    # arity
    ([(L, -1, -1, -1, DATA), (L, -1, -1, -1, P0), (25, 0, 1, 1, None)], _lib.MC_ERR_INVALID,
     b"bad arguments"),
    ([(L, -1, -1, -1, DATA), (L, -1, -1, -1, P0), (26, 0, 1, -1, None)], _lib.MC_ERR_INVALID,
     b"bad arguments"),
    ([(L, -1, -1, -1, DATA), (27, 0, -1, -1, None)], _lib.MC_ERR_INVALID, b"bad arguments"),
    ([(L, -1, -1, -1, P0), (28, 0, -1, -1, None)], _lib.MC_ERR_INVALID, b"unknown op"),
])
def test_node_validation(nodes, code, msg):
    rc, err = _expr_program(nodes)
    assert rc == code and msg in err, (rc, err)


def test_new_functions_are_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "mcmc355.h")).read()
    lib = _lib.load()
    bound = {name: (res, args) for name, res, args in _lib.SIGNATURES}
    for name, nargs in (("mc_discrete_log_prob", 10), ("mc_predictive_draw_discrete", 8),
                        ("mc_predictive_eq", 14), ("mc_program_num_count_terms", 1)):
        assert re.search(rf"\b{name}\(", text), name
        fn = getattr(lib, name)
        assert fn.restype is bound[name][0] and list(fn.argtypes) == bound[name][1]
        assert len(bound[name][1]) == nargs
    assert len(bound["mc_predictive"][1]) == 13 and _lib.MC_PP_COUNT == 5
    out = ctypes.c_float()
    assert lib.mc_predictive_draw_discrete(3, 0.0, 0.0, 0, 0, 0, 0, ctypes.byref(out)) \
        == _lib.MC_ERR_INVALID
    assert lib.mc_predictive_draw_discrete(0, 0.0, 0.0, 0, 0, 0, 0, None) == _lib.MC_ERR_INVALID
    assert lib.mc_discrete_log_prob(7, 1, None, 1, None, 1, None, 1, None, None) == _lib.MC_ERR_INVALID
    # mc_predictive_draw keeps refusing expression terms
    assert lib.mc_predictive_draw(_lib.MC_DIST_EXPR, 0.0, 1.0, 0, 0, 0, 0,
                                  ctypes.byref(out)) == _lib.MC_ERR_UNSUPPORTED


def _host_program(log_likelihood, shapes):
    lib = _lib.load()
    init = {k: np.ones(s, F32) for k, s in shapes.items()}
    lib.mc_debug_program_host_only(1)
    try:
        return _trace.Program(_trace.trace(log_likelihood, init, keep_order=True))
    finally:
        lib.mc_debug_program_host_only(0)


def test_sampler_descriptors_recorded_at_program_creation():
    """mc_program_num_count_terms on host-only programs: one per count term
    stated with logits = / log_rate =; none for the hand-written logistic, for
    the probs = / rate = lowering (a where root); a fused term beside two
    count terms does not count."""
    import _pointwise as PW
    import mlx_mcmc_amd as m
    import mlx_mcmc_amd.core as mx

    lib = _lib.load()
    count = lambda prog: lib.mc_program_num_count_terms(prog.handle)   # noqa: E731
    for name in DS.OP:
        model = DS.likelihood(name)
        prog = _host_program(model.log_likelihood, model.shapes)
        assert prog.num_elements == DS.N_OBS and count(prog) == 1, name
    hand = PW.logistic()
    assert count(_host_program(hand.log_likelihood, hand.shapes)) == 0
    d = DS.data()
    sh = {"a": (), "b": ()}
    assert count(_host_program(
        lambda p: mx.sum(m.Poisson(rate=mx.exp(p["a"] + p["b"] * d.x)).log_prob(d.yp)), sh)) == 0
    assert count(_host_program(
        lambda p: mx.sum(m.Bernoulli(probs=mx.sigmoid(p["a"] + p["b"] * d.x)).log_prob(d.yb)),
        sh)) == 0
    z = np.linspace(-1, 1, 13).astype(F32)
    mixed = _host_program(
        lambda p: (mx.sum(m.Normal(p["a"], 1.5).log_prob(z))
                   + mx.sum(m.Poisson(log_rate=p["a"] + p["b"] * d.x).log_prob(d.yp))
                   + mx.sum(m.Bernoulli(logits=p["b"] * d.x).log_prob(d.yb))), sh)
    assert mixed.num_elements == 13 + 2 * DS.N_OBS and count(mixed) == 2
    assert lib.mc_program_num_count_terms(ctypes.c_void_p(0)) == _lib.MC_ERR_INVALID


# ---- the host samplers ----------------------------------------------------------------------
def test_bernoulli_equals_the_numpy_restatement_bit_for_bit():
    chain, it, obs = _triples()
    rng = np.random.default_rng(8)
    eta = (rng.standard_normal(chain.size) * 3.0).astype(F32)
    eta[:6] = [0.0, np.inf, -np.inf, 20.0, -20.0, np.nan]
    seed = 0x1234567890ABCDEF
    got = DS.host_draws(DS.BERNOULLI, 0.0, eta, seed, chain, it, obs)
    want = DS.bernoulli_draw(eta, seed, chain, it, obs)
    assert got.tobytes() == want.tobytes()
    assert got[1] == 1 and got[2] == 0 and np.isnan(got[5])
    assert set(np.unique(got[~np.isnan(got)])) == {0.0, 1.0}


CHI_N = 20000
CHI_CAP = 1e-4
BERN = [-4.0, 0.0, 2.5]
BINOM = [(1, 0.3), (12, 0.5), (40, 0.02), (200, 0.3), (1000, 0.9)]
POIS = [0.05, 3.0, 9.99, 10.0, 250.0, 1e4]


def _chi2(x, dist):
    """Chi-square goodness of fit p-value of integer draws against a scipy
    discrete distribution, neighbouring outcomes pooled to an expected count
    of at least 5."""
    x = np.asarray(x, np.int64)
    lo, hi = int(min(x.min(), dist.ppf(1e-9))), int(max(x.max(), dist.ppf(1 - 1e-9)))
    ks = np.arange(lo, hi + 1)
    e = dist.pmf(ks) * x.size
    e[0] += dist.cdf(lo - 1) * x.size
    e[-1] += dist.sf(hi) * x.size
    o = np.bincount(x - lo, minlength=ks.size).astype(np.float64)
    eo, oo, ce, co = [], [], 0.0, 0.0
    for a, b in zip(e, o):
        ce += a
        co += b
        if ce >= 5.0:
            eo.append(ce)
            oo.append(co)
            ce = co = 0.0
    if eo:
        eo[-1] += ce
        oo[-1] += co
    else:
        eo, oo = [ce], [co]
    if len(eo) < 2:
        return 1.0 if oo[0] == x.size else 0.0
    eo, oo = np.array(eo), np.array(oo)
    return float(sps.chi2.sf(np.sum((oo - eo) ** 2 / eo), len(eo) - 1))


def _grid(case):
    it, obs = np.divmod(np.arange(CHI_N), 200)
    return 2000 + case, it, obs


def _check(label, x, dist, seed):
    assert np.all(np.isfinite(x)) and np.all(x == np.floor(x))
    p = _chi2(x, dist)
    own = _chi2(dist.rvs(CHI_N, random_state=np.random.default_rng(seed)), dist)
    print(f"{label}: chi-square p = {p:.4g} (scipy's own rvs: {own:.4g})")
    assert own > CHI_CAP
    assert p > CHI_CAP


@pytest.mark.parametrize("case", range(len(BERN)))
def test_bernoulli_chi_square(case):
    eta = BERN[case]
    seed, it, obs = _grid(case)
    x = DS.host_draws(DS.BERNOULLI, 0.0, eta, seed, 1, it, obs)
    _check(f"Bernoulli(logit {eta})", x, sps.bernoulli(1.0 / (1.0 + np.exp(-float(F32(eta))))), seed)


@pytest.mark.parametrize("case", range(len(BINOM)))
def test_binomial_chi_square(case):
    n, p = BINOM[case]
    eta = F32(np.log(p) - np.log1p(-p))
    seed, it, obs = _grid(10 + case)
    x = DS.host_draws(DS.BINOMIAL, n, eta, seed, 2, it, obs)
    assert np.all((x >= 0) & (x <= n))
    _check(f"Binomial({n}, {p})", x, sps.binom(n, 1.0 / (1.0 + np.exp(-float(eta)))), seed)


@pytest.mark.parametrize("case", range(len(POIS)))
def test_poisson_chi_square(case):
    lam = POIS[case]
    theta = F32(np.log(lam))
    if lam == 10.0:
        # the inversion / PTRS threshold itself: exp(theta) on either side of 10
        assert float(np.exp(np.float64(np.nextafter(theta, F32(0))))) < 10.0
    seed, it, obs = _grid(20 + case)
    x = DS.host_draws(DS.POISSON, 0.0, theta, seed, 3, it, obs)
    assert np.all(x >= 0)
    _check(f"Poisson({lam})", x, sps.poisson(float(np.exp(np.float64(theta)))), seed)


def test_invalid_and_over_range_parameters_give_nan():
    nan, inf = float("nan"), float("inf")
    d = lambda k, n, e: DS.host_draw(k, n, e, 7, 1, 2, 3)   # noqa: E731
    assert np.isnan(d(DS.BERNOULLI, 0, nan))
    for theta in (nan, inf, 16.0, 88.0):                     # exp(16) > 2^23
        assert np.isnan(d(DS.POISSON, 0, theta)), theta
    assert d(DS.POISSON, 0, -inf) == 0 and d(DS.POISSON, 0, -800.0) == 0
    assert np.isfinite(d(DS.POISSON, 0, 15.9))
    for n in (-1.0, 2.5, nan, inf, 2.0 ** 23):
        assert np.isnan(d(DS.BINOMIAL, n, 0.3)), n
    assert np.isnan(d(DS.BINOMIAL, 5, nan))
    assert d(DS.BINOMIAL, 0, 0.3) == 0
    assert d(DS.BINOMIAL, 9, inf) == 9 and d(DS.BINOMIAL, 9, -inf) == 0
    assert np.isfinite(d(DS.BINOMIAL, 2.0 ** 23 - 1, 0.3))
    assert np.isfinite(d(DS.BINOMIAL, 2.0 ** 23 - 1, -14.0))


@pytest.mark.parametrize("kind,n,eta", [(DS.BERNOULLI, 0, 0.1), (DS.BINOMIAL, 1000, 0.3),
                                        (DS.BINOMIAL, 30, -2.0), (DS.POISSON, 0, 1.0),
                                        (DS.POISSON, 0, 6.0)])
def test_every_counter_field_changes_the_draw(kind, n, eta):
    """Counts tie often: a field changes the draw when a run of 64 draws along
    another field changes."""
    obs = np.arange(64)
    base = dict(seed=11, chain=2, it=5)
    x0 = DS.host_draws(kind, n, eta, base["seed"], base["chain"], base["it"], obs)
    for k, v in (("seed", 12), ("seed", 11 + 2 ** 32), ("chain", 3), ("it", 6)):
        b = dict(base, **{k: v})
        assert not np.array_equal(DS.host_draws(kind, n, eta, b["seed"], b["chain"], b["it"], obs),
                                  x0), k
    assert not np.array_equal(DS.host_draws(kind, n, eta, 11, 2, 5, obs + 64), x0)
    assert np.array_equal(DS.host_draws(kind, n, eta, 11, 2, 5, obs), x0)


# ---- merging -----------------------------------------------------------------------------------
def test_merge_predictive_with_and_without_equal():
    rng = np.random.default_rng(4)
    x = rng.poisson(3.0, (53, 9)).astype(F32)
    x[17, 4] = np.nan
    v = rng.poisson(3.0, 9).astype(np.float64)
    whole = DS.stats_of(x, v)
    assert whole["equal"].sum() > 0
    parts = [DS.stats_of(s, v) for s in np.split(x, (5, 31), axis=0)]
    got = D.merge_predictive(parts)
    assert sorted(got) == sorted(PP.FIELDS + ("equal",))
    for f in got:
        np.testing.assert_allclose(got[f], whole[f], rtol=1e-12, atol=0, err_msg=f)
    # one part without it: exactly the five fields, as before
    del parts[1]["equal"]
    got = D.merge_predictive(parts)
    assert sorted(got) == sorted(PP.FIELDS)
    for f in got:
        np.testing.assert_allclose(got[f], whole[f], rtol=1e-12, atol=0, err_msg=f)
    assert "equal" in parts[0]          # the inputs are left as they were
