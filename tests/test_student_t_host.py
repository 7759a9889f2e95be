"""StudentT / Cauchy / HalfStudentT / HalfCauchy without a device: the op codes
and bindings, the float64 node table against scipy.stats and central
differences, the tracer's lowering and its refusals, the ABI's validation, and
the host sampler mc_predictive_draw_student_t (csrc/predictive.h) — its purity,
its location-scale bits, its NaN rules and its distribution."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
from scipy import stats as sps

import _student_t as ST
from mlx_mcmc_amd import _lib, _trace
from test_abi import _expr_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
L = _lib.MC_EX_LEAF


# ---- codes, exports, bindings ------------------------------------------------------------
def test_op_codes_equal_the_header():
    text = open(os.path.join(ROOT, "include", "mcmc355.h")).read()
    for name, code in (("MC_EX_STUDENT_T_LP", 32), ("MC_EX_HALF_STUDENT_T_LP", 33)):
        assert re.search(rf"\b{name}\s*=\s*{code}\b", text), name
        assert getattr(_lib, name) == code
    assert ST.OP == {"student_t": 32, "half_student_t": 33}
    assert re.search(r"#define\s+MC_ABI_VERSION\s+2\b", text)
    assert _lib.MC_EX_PICK == 30 and _lib.MC_EXPR_MAX_NODES == 32


def test_classes_are_exported():
    import mlx_mcmc_amd as m
    from mlx_mcmc_amd import distributions

    for name in ("StudentT", "Cauchy", "HalfStudentT", "HalfCauchy"):
        assert name in m.__all__ and name in distributions.__all__
        assert issubclass(getattr(m, name), m.Distribution)
    assert m.Cauchy(0.5, 2.0).df == 1.0 and m.HalfCauchy(2.0).df == 1.0
    assert repr(m.StudentT(4, 0.5, 2.0)) == "StudentT(df=4.000, loc=0.500, scale=2.000)"
    assert repr(m.Cauchy(0.5, 2.0)) == "Cauchy(loc=0.500, scale=2.000)"
    assert repr(m.HalfStudentT(3, 2.0)) == "HalfStudentT(df=3.000, scale=2.000)"
    assert repr(m.HalfCauchy(5.0)) == "HalfCauchy(scale=5.000)"


def test_new_functions_are_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "mcmc355.h")).read()
    lib = _lib.load()
    bound = {name: (res, args) for name, res, args in _lib.SIGNATURES}
    for name, nargs in (("mc_student_t_log_prob", 11), ("mc_predictive_draw_student_t", 9)):
        assert re.search(rf"\b{name}\(", text), name
        fn = getattr(lib, name)
        assert fn.restype is bound[name][0] and list(fn.argtypes) == bound[name][1]
        assert len(bound[name][1]) == nargs
    assert lib.mc_predictive_draw_student_t(4.0, 0.0, 1.0, 0, 0, 0, 0, 0, None) \
        == _lib.MC_ERR_INVALID
    for df in (0.0, -1.0, math.nan, math.inf):
        assert lib.mc_student_t_log_prob(df, 0, 1, None, 1, None, 1, None, 1, None, None) \
            == _lib.MC_ERR_INVALID, df
    assert b"degrees of freedom" in lib.mc_last_error()
    # the discrete entry points are what they were
    assert len(bound["mc_predictive_draw_discrete"][1]) == 8 and _lib.MC_DISCRETE_POISSON == 2


# ---- the node table -----------------------------------------------------------------------
def _points(rng, P, half):
    v = ST.X._logu(rng, P, 1e-3, 30.0, not half)
    m = ST.X._logu(rng, P, 1e-3, 30.0, True)
    s = ST.X._logu(rng, P, 1e-2, 30.0)
    return v, m, s


@pytest.mark.parametrize("nu", [0.7, 1.0, 4.0, 30.0])
def test_table_plus_normaliser_equals_scipy(nu):
    rng = np.random.default_rng(5)
    v, m, s = _points(rng, 512, False)
    nu32 = float(F32(nu))
    want = sps.t.logpdf(v.astype(np.float64), nu32, loc=m.astype(np.float64),
                        scale=s.astype(np.float64))
    got = ST.fwd64("student_t", nu, v, m, s) + ST.norm64(nu, False)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)
    v = np.abs(v)
    got = ST.fwd64("half_student_t", nu, v, None, s) + ST.norm64(nu, True)
    want = math.log(2.0) + sps.t.logpdf(v.astype(np.float64), nu32, scale=s.astype(np.float64))
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)
    if nu == 1.0:
        np.testing.assert_allclose(got, sps.halfcauchy.logpdf(v.astype(np.float64),
                                                              scale=s.astype(np.float64)),
                                   rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("name", ST.NODES)
@pytest.mark.parametrize("nu", [1.0, 4.0, 30.0])
def test_table_vjp_equals_central_differences(name, nu):
    rng = np.random.default_rng(6)
    v, m, s = _points(rng, 256, ST.is_half(name))
    a = {"v": v.astype(np.float64), "m": m.astype(np.float64), "s": s.astype(np.float64)}
    g = ST.vjp64(name, nu, v, m, s)

    def f(**kw):
        b = dict(a, **kw)
        return ST._fwd(name, nu, b["v"], b["m"], b["s"])
    for k in ST.diff_names(name):
        h = 1e-6 * np.maximum(np.abs(a[k]), 1e-2)
        if ST.is_half(name) and k == "v":
            h = np.minimum(h, 0.5 * a[k])         # (stay inside the support)
        fp, fm = f(**{k: a[k] + h}), f(**{k: a[k] - h})
        fd = (fp - fm) / (2 * h)
        # (truncation h^2 f''' / 6 ~ 1e-12 relative; the difference of two values
        # of size |f| carries their float64 rounding over 2 h)
        tol = 2e-6 * np.abs(fd) + 8 * np.finfo(np.float64).eps * (np.abs(fp) + 1.0) / h
        assert np.all(np.abs(g[k] - fd) <= tol), (k, float(np.max(np.abs(g[k] - fd) - tol)))
    assert set(g) == set(ST.diff_names(name))


def test_edge_classes_of_the_table():
    inf, nan = np.inf, np.nan
    f, g = ST.fwd32, ST.vjp32
    # q = inf: -inf and zero cotangents (the formulas would give inf / inf, or -1 / s)
    for v in (inf, -inf, 3e19, -3e19):
        assert f("student_t", 4.0, v, 0.0, 1.0) == -inf
        assert all(x == 0 for x in g("student_t", 4.0, v, 0.0, 1.0).values())
    assert np.isfinite(ST.fwd64("student_t", 4.0, 3e19, 0.0, 1.0))   # (float64 has the range)
    # NaN arguments; s <= 0 and s = inf as MC_EX_NORMAL_LP
    for args in ((nan, 0.0, 1.0), (0.3, nan, 1.0), (0.3, 0.0, nan), (0.3, 0.0, -1.0),
                 (0.3, 0.0, 0.0), (0.3, 0.3, 0.0)):
        assert np.isnan(f("student_t", 4.0, *args)), args
        assert np.isnan(ST.X.fwd32("normal_lp", *[np.array([t], F32) for t in args])[0]), args
    assert f("student_t", 4.0, 0.3, 0.0, inf) == -inf
    # the half form: ex_halfnormal's convention
    for v in (-1.0, nan, -inf):
        assert f("half_student_t", 1.0, v, None, 1.3) == -inf
        assert all(x == 0 for x in g("half_student_t", 1.0, v, None, 1.3).values())
    assert f("half_student_t", 1.0, -0.0, None, 1.3) == -np.log(F32(1.3))
    assert g("half_student_t", 1.0, -0.0, None, 1.3)["s"] == F32(-1.0) / F32(1.3)


# ---- the tracer -----------------------------------------------------------------------------
def _nodes(lp, init):
    model = _trace.trace(lp, init, keep_order=True)
    assert len(model.terms) == 1 and model.terms[0].dist == _lib.MC_DIST_EXPR
    return model, [(model.c_nodes[i].op, model.c_nodes[i].leaf.kind) for i in range(model.n_nodes)]


def test_tracer_lowers_to_add_of_node_and_constant():
    import mlx_mcmc_amd as m
    import mlx_mcmc_amd.core as mx

    d = ST.data()
    init = {"a": F32(0.1), "b": F32(0.2), "s": F32(1.5)}
    model, nodes = _nodes(
        lambda p: mx.sum(m.StudentT(4, p["a"] + p["b"] * d.x, p["s"]).log_prob(d.y)), init)
    # y, a, b, x, s leaves; MUL, ADD; the node; the constant; ADD
    assert model.n_nodes == 10, nodes
    root = model.c_nodes[model.n_nodes - 1]
    node = model.c_nodes[root.a]
    assert root.op == _lib.MC_EX_ADD and node.op == 32
    assert nodes[root.b] == (L, _lib.MC_OP_CONST)
    want = math.lgamma(2.5) - math.lgamma(2.0) - 0.5 * math.log(4.0 * math.pi)
    assert model.c_nodes[root.b].leaf.value == F32(want)
    assert node.leaf.value == 4.0 and node.leaf.kind == _lib.MC_OP_NONE
    assert nodes[node.a] == (L, _lib.MC_OP_DATA) and nodes[node.c] == (L, _lib.MC_OP_PSCALAR)
    assert model.c_nodes[node.b].op == _lib.MC_EX_ADD
    # the hand-written form of the same density: twice the nodes
    def hand(p):
        z = (d.y - (p["a"] + p["b"] * d.x)) / p["s"]
        return mx.sum(-2.5 * mx.log1p(z * z / 4.0) - mx.log(p["s"]) + F32(want))
    hmodel, _ = _nodes(hand, init)
    assert hmodel.n_nodes >= 18
    # the half form: no loc argument, log 2 in the constant; Cauchy classes are df = 1
    model, nodes = _nodes(lambda p: m.HalfCauchy(2.0).log_prob(mx.exp(p["s"])), {"s": F32(0.1)})
    root = model.c_nodes[model.n_nodes - 1]
    node = model.c_nodes[root.a]
    assert root.op == _lib.MC_EX_ADD and node.op == 33 and node.b == -1 and node.leaf.value == 1.0
    assert model.c_nodes[node.a].op == _lib.MC_EX_EXP
    assert model.c_nodes[root.b].leaf.value == F32(math.log(2.0) - math.log(math.pi))
    assert _trace.student_t_norm(1.0, False) == F32(-math.log(math.pi))
    model, _ = _nodes(lambda p: m.Cauchy(p["s"], 2.0).log_prob(0.3), {"s": F32(0.1)})
    assert model.c_nodes[model.c_nodes[model.n_nodes - 1].a].leaf.value == 1.0
    # a value, a loc or a scale alone is enough to trace
    P = _trace.Param("p", 0, ())
    for lp in (m.StudentT(3, 0.0, 1.0).log_prob(P), m.StudentT(3, P, 1.0).log_prob(0.5),
               m.StudentT(3, 0.0, P).log_prob(0.5), m.HalfStudentT(3, P).log_prob(0.5)):
        assert lp.terms[0].expr.op == _lib.MC_EX_ADD


def test_df_must_be_a_positive_constant():
    import mlx_mcmc_amd as m

    P = _trace.Param("p", 0, ())
    for make in (lambda: m.StudentT(P), lambda: m.HalfStudentT(P, 1.0)):
        with pytest.raises(_trace.TraceError, match="lgamma.*digamma"):
            make()
    for df in (0.0, -2.0, math.nan, math.inf, np.array([3.0, 4.0]), np.array([3.0])):
        with pytest.raises(ValueError):
            m.StudentT(df)
        with pytest.raises(ValueError):
            m.HalfStudentT(df, 2.0)
    assert m.StudentT(np.float32(2.5)).df == 2.5 and m.StudentT(np.array(3)).df == 3.0


def test_moments_and_host_samples():
    import mlx_mcmc_amd as m

    assert np.isnan(m.Cauchy(0.5, 2.0).mean()) and np.isnan(m.Cauchy(0.5, 2.0).variance())
    assert m.StudentT(1.5, 0.5, 2.0).mean() == F32(0.5)
    assert np.isinf(m.StudentT(1.5, 0.5, 2.0).variance())
    np.testing.assert_allclose(m.StudentT(4, 0.5, 2.0).variance(), 8.0)
    assert m.StudentT(4, 0.5, 2.0).mode() == F32(0.5) and m.HalfCauchy(2.0).mode() == 0
    assert np.isinf(m.HalfCauchy(2.0).mean())
    np.testing.assert_allclose(m.HalfStudentT(3, 2.0).mean(), 2.0 * 2 * math.sqrt(3) / math.pi,
                               rtol=1e-6)
    h = m.HalfStudentT(5, 1.5)
    x = np.abs(sps.t(5).rvs(400_000, random_state=1)) * 1.5
    np.testing.assert_allclose(h.mean(), x.mean(), rtol=1e-2)
    np.testing.assert_allclose(h.variance(), x.var(), rtol=3e-2)
    s = m.StudentT(4, 1.0, 0.5).sample(m.random.key(3), (4000,))
    assert s.dtype == F32 and s.shape == (4000,) and abs(np.median(s) - 1.0) < 0.05
    assert np.array_equal(s, m.StudentT(4, 1.0, 0.5).sample(m.random.key(3), (4000,)))
    s = m.HalfCauchy(2.0).sample(m.random.key(3), (4000,))
    assert np.all(s >= 0) and abs(np.median(s) - 2.0) < 0.2


# ---- the ABI ----------------------------------------------------------------------------------
P0 = {"kind": _lib.MC_OP_PSCALAR, "param_offset": 0}
P1 = {"kind": _lib.MC_OP_PSCALAR, "param_offset": 1}
DATA = {"kind": _lib.MC_OP_DATA, "pool_offset": 0}
NU4 = {"value": 4.0}
_LEAVES = [(L, -1, -1, -1, DATA), (L, -1, -1, -1, P0), (L, -1, -1, -1, P1)]


@pytest.mark.parametrize("nodes,msg", [
    (_LEAVES + [(32, 0, 1, -1, NU4)], b"bad arguments"),          # no scale
    (_LEAVES + [(32, 0, -1, 2, NU4)], b"bad arguments"),          # no loc
    (_LEAVES + [(33, 0, 1, 2, NU4)], b"bad arguments"),           # the half form reads no b
    (_LEAVES + [(33, 0, -1, -1, NU4)], b"bad arguments"),
    (_LEAVES + [(32, 0, 1, 3, NU4)], b"bad arguments"),           # forward reference
    (_LEAVES + [(31, 0, 1, 2, NU4)], b"unknown op"),              # 31 is not assigned
    (_LEAVES + [(34, 0, 1, 2, NU4)], b"unknown op"),
] + [(_LEAVES + [(op, 0, 1 if op == 32 else -1, 2, {"value": nu})], b"degrees of freedom")
     for op in (32, 33) for nu in (0.0, -1.0, math.nan, math.inf)]
  + [(_LEAVES + [(32, 0, 1, 2, None)], b"degrees of freedom")])   # leaf.value left at 0
def test_node_validation(nodes, msg):
    rc, err = _expr_program(nodes)
    assert rc == _lib.MC_ERR_INVALID and msg in err, (rc, err)
    if msg == b"degrees of freedom":
        assert b"term 0 node 3" in err, err


def _host_program(log_likelihood, shapes):
    lib = _lib.load()
    init = {k: np.ones(s, F32) for k, s in shapes.items()}
    lib.mc_debug_program_host_only(1)
    try:
        return _trace.Program(_trace.trace(log_likelihood, init, keep_order=True))
    finally:
        lib.mc_debug_program_host_only(0)


def test_student_t_terms_are_not_count_terms():
    """Host-only programs: the Student-t likelihoods build (the valid nodes pass
    validation) and mc_program_num_count_terms keeps counting count terms."""
    import _discrete as DS
    import mlx_mcmc_amd as m
    import mlx_mcmc_amd.core as mx

    lib = _lib.load()
    for name in ("regression", "cauchy", "half"):
        model = ST.likelihood(name)
        prog = _host_program(model.log_likelihood, model.shapes)
        assert prog.num_elements == ST.N_OBS, name
        assert lib.mc_program_num_count_terms(prog.handle) == 0, name
    d, dd = ST.data(), DS.data()
    mixed = _host_program(
        lambda p: (mx.sum(m.StudentT(4, p["a"] + p["b"] * d.x, p["s"]).log_prob(d.y))
                   + mx.sum(m.Poisson(log_rate=p["a"] + p["b"] * dd.x).log_prob(dd.yp))),
        {"a": (), "b": (), "s": ()})
    assert mixed.num_elements == 2 * ST.N_OBS
    assert lib.mc_program_num_count_terms(mixed.handle) == 1


# ---- the host sampler ---------------------------------------------------------------------------
def test_draw_is_a_pure_function_of_its_counter():
    base = ST.host_draw(4.0, 0.5, 2.0, 0, 11, 2, 7, 5)
    assert base == ST.host_draw(4.0, 0.5, 2.0, 0, 11, 2, 7, 5) and np.isfinite(base)
    others = [ST.host_draw(4.0, 0.5, 2.0, 0, *k) for k in
              ((12, 2, 7, 5), (11, 3, 7, 5), (11, 2, 8, 5), (11, 2, 7, 6))]
    assert len({float(base)} | {float(x) for x in others}) == 5


@pytest.mark.parametrize("nu", [0.7, 1.0, 3.0, 30.0])
def test_draw_is_location_scale_of_the_standard_draw(nu):
    obs = np.arange(300)
    t = ST.host_draws(nu, 0.0, 1.0, 0, 5, 1, 2, obs)
    m, s = F32(-1.7), F32(2.3)
    full = ST.host_draws(nu, m, s, 0, 5, 1, 2, obs)
    half = ST.host_draws(nu, 99.0, s, 1, 5, 1, 2, obs)            # (the half form reads no loc)
    assert full.tobytes() == (m + s * t).astype(F32).tobytes()
    assert half.tobytes() == np.abs(s * t).astype(F32).tobytes()
    assert np.all(np.isfinite(t)) and (t < 0).any() and (t > 0).any()


def test_draw_gives_nan_for_invalid_parameters():
    nan = math.nan
    for nu, m, s in ((4.0, 0.0, 0.0), (4.0, 0.0, -1.0), (4.0, 0.0, nan), (0.0, 0.0, 1.0),
                     (-2.0, 0.0, 1.0), (nan, 0.0, 1.0), (4.0, nan, 1.0)):
        assert np.isnan(ST.host_draw(nu, m, s, 0, 3, 0, 0, 0)), (nu, m, s)
    assert np.isnan(ST.host_draw(4.0, 0.0, -1.0, 1, 3, 0, 0, 0))


@pytest.mark.parametrize("nu", [0.7, 1.0, 3.0, 30.0])
def test_draws_follow_the_t_distribution(nu):
    """20 000 draws over obs = 0 .. 19 999 at one fixed seed: the
    Kolmogorov-Smirnov statistic against scipy.stats.t(nu) has D sqrt(n) < 2.2,
    the asymptotic 1.3e-4 point — an exact sampler fails a given seed with that
    probability, so a failure is a bug to find and not a seed to change."""
    n = 20_000
    t = ST.host_draws(nu, 0.0, 1.0, 0, 2024, 0, 0, np.arange(n)).astype(np.float64)
    assert np.all(np.isfinite(t))
    x = np.sort(t)
    cdf = sps.t(float(F32(nu))).cdf(x)
    k = np.arange(1, n + 1)
    D = max(np.max(k / n - cdf), np.max(cdf - (k - 1) / n))
    print(f"nu = {nu}: D sqrt(n) = {D * math.sqrt(n):.3f}")
    assert D * math.sqrt(n) < 2.2
