"""Categorical without a device: the reference's known answers restated as
numbers, the float64 node table against torch autograd and its own float32
restatement inside the derived gates, op codes, the tracer's lowering, its
errors, and the ABI's validation of the two nodes."""
import os
import re

import numpy as np
import pytest

import _categorical as CT
import _expr_ops as X
from mlx_mcmc_amd import _lib, _trace
from test_abi import _expr_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
L = _lib.MC_EX_LEAF


def _m():
    import mlx_mcmc_amd as m
    import mlx_mcmc_amd.core as mx
    return m, mx


# ---- the reference's known answers (its tests/test_new_distributions.py:187-261) ----------
def test_exported():
    m, _ = _m()
    from mlx_mcmc_amd import distributions
    assert "Categorical" in m.__all__ and "Categorical" in distributions.__all__
    assert issubclass(m.Categorical, m.Distribution)


def test_normalisation_and_num_categories():
    m, _ = _m()
    d = m.Categorical(probs=[0.2, 0.3, 0.5])
    assert d.num_categories == 3 and np.isclose(float(np.sum(d.probs)), 1.0)
    d = m.Categorical(probs=[2.0, 3.0, 5.0])              # normalised as p / sum p
    np.testing.assert_allclose(d.probs, [0.2, 0.3, 0.5], rtol=1e-6)
    d = m.Categorical(logits=[1.0, 2.0, 3.0])
    assert d.num_categories == 3 and np.isclose(float(np.sum(d.probs)), 1.0)
    assert d.probs.dtype == F32 and d.logits.dtype == F32


def test_log_prob_known_answers():
    m, _ = _m()
    d = m.Categorical(probs=[0.2, 0.5, 0.3])
    assert np.isclose(float(d.log_prob(0)), np.log(0.2), rtol=0.01)
    assert np.isclose(float(d.log_prob(1)), np.log(0.5), rtol=0.01)
    assert float(d.log_prob(-1)) == -np.inf and float(d.log_prob(3)) == -np.inf
    got = d.log_prob(np.array([0, 1, 2, 3, -1]))
    assert got.dtype == F32 and got.shape == (5,)
    np.testing.assert_allclose(got[:3], np.log([0.2, 0.5, 0.3]), rtol=1e-6)
    assert np.all(got[3:] == -np.inf)
    assert float(d.log_prob(0.5)) == -np.inf              # not an integer: invalid, as on the device


def test_logits_are_normalised_a_deliberate_departure():
    """The reference's logits= path returns the un-normalised logits; here the
    log-softmax, without overflow."""
    m, _ = _m()
    d = m.Categorical(logits=[2.0, 1.0, 0.5])
    z = np.array([2.0, 1.0, 0.5])
    np.testing.assert_allclose(d.log_prob([0, 1, 2]), z - np.log(np.exp(z).sum()), rtol=1e-6)
    np.testing.assert_array_equal(m.Categorical(logits=[1000.0, 0.0, -1000.0]).log_prob([0, 1, 2]),
                                  np.array([0.0, -1000.0, -2000.0], F32))


def test_constructor_errors():
    m, _ = _m()
    with pytest.raises(ValueError):
        m.Categorical()
    with pytest.raises(ValueError):
        m.Categorical(probs=[0.5, 0.5], logits=[1.0, 1.0])


def test_mode_entropy_repr():
    m, _ = _m()
    d = m.Categorical(probs=[0.1, 0.7, 0.2])
    assert int(d.mode()) == 1
    p = np.array([0.1, 0.7, 0.2])
    assert np.isclose(float(d.entropy()), -(p * np.log(p)).sum(), rtol=1e-6)
    assert np.isclose(float(m.Categorical(probs=[1.0, 0.0]).entropy()), 0.0)
    assert repr(d) == "Categorical(num_categories=3)"


# ---- the node table -------------------------------------------------------------------------
def test_op_codes_equal_the_header():
    text = open(os.path.join(ROOT, "include", "mcmc355.h")).read()
    for name, code in (("MC_EX_LOGADDEXP", 29), ("MC_EX_PICK", 30)):
        assert re.search(rf"\b{name}\s*=\s*{code}\b", text), name
        assert getattr(_lib, name) == code
    assert re.search(r"#define\s+MC_ABI_VERSION\s+2\b", text)
    assert _lib.MC_EX_POISSON_LOG_LP == 27 and _lib.MC_EXPR_MAX_NODES == 32


def test_gates_are_the_derived_ones():
    assert (CT.K_EXP, CT.K_L1P, CT.K_SIG) == (2.0, 2.828, 2.022)
    assert abs(CT.K_LAE - 7.828) < 1e-12 and CT.LAE_GATE == 8
    assert abs(CT.K_DA - 4.768) < 1e-12 and CT.DA_GATE == 5 and CT.DB_GATE == 6
    # the constant of the d-rounding term: max of x e^-x / (1 + e^-x)^2
    t = np.linspace(0, 40, 400001)
    assert (t * np.exp(-t) / (1 + np.exp(-t)) ** 2).max() <= 0.2240


def test_table_equals_torch_autograd():
    import torch

    A, B, nb = CT.lae_rows()
    a, b = A[:nb].ravel().astype(np.float64), B[:nb].ravel().astype(np.float64)
    ta, tb = torch.tensor(a, requires_grad=True), torch.tensor(b, requires_grad=True)
    v = torch.logaddexp(ta, tb)
    v.sum().backward()
    np.testing.assert_allclose(CT.lae64(A[:nb].ravel(), B[:nb].ravel()), v.detach().numpy(),
                               rtol=1e-14, atol=0)
    da, db = CT.lae_vjp64(A[:nb].ravel(), B[:nb].ravel())
    np.testing.assert_allclose(da, ta.grad.numpy(), rtol=1e-12, atol=1e-300)
    # (db = 1 - da rounds once in float64 too: half an ulp of the cotangent)
    np.testing.assert_allclose(db, tb.grad.numpy(), rtol=1e-12, atol=2.0 ** -52)
    np.testing.assert_array_equal(da + db, np.ones_like(da))     # the cotangents sum to c


def test_float32_restatement_sits_inside_the_gates():
    A, B, nb = CT.lae_rows()
    a, b = A[:nb].ravel(), B[:nb].ravel()
    assert np.abs(a - b).max() > 95 and np.abs(a - b).min() < 0.01
    ef = np.abs(CT.lae32(a, b).astype(np.float64) - CT.lae64(a, b)) / CT.lae_unit(a, b)
    da32, db32 = CT.lae_vjp32(a, b)
    da64, db64 = CT.lae_vjp64(a, b)
    u1 = float(np.spacing(F32(1.0)))
    ea = np.abs(da32.astype(np.float64) - da64) / u1
    eb = np.abs(db32.astype(np.float64) - db64) / u1
    print(f"float32 restatement: value {ef.max():.3f} (gate {CT.LAE_GATE}), da {ea.max():.3f} "
          f"(gate {CT.DA_GATE}), db {eb.max():.3f} (gate {CT.DB_GATE})")
    assert ef.max() <= CT.LAE_GATE and ea.max() <= CT.DA_GATE and eb.max() <= CT.DB_GATE


def test_edges_of_the_table():
    inf, nan, l2 = np.inf, np.nan, F32(np.log(2.0))
    assert CT.lae32(0.7, 0.7) == F32(0.7) + l2 and CT.lae32(1e30, 1e30) == F32(1e30)
    for a, b, v, da in ((-inf, 1.5, 1.5, 0.0), (1.5, -inf, 1.5, 1.0), (inf, 1.0, inf, 1.0),
                        (1.0, inf, inf, 0.0), (inf, -inf, inf, 1.0), (-inf, -inf, -inf, 0.5),
                        (inf, inf, inf, 0.5), (1000.0, 0.0, 1000.0, 1.0), (90.0, 0.0, 90.0, 1.0)):
        assert CT.lae32(a, b) == F32(v), (a, b)
        ga, gb = CT.lae_vjp32(a, b)
        assert ga == F32(da) and gb == F32(1.0 - da), (a, b, ga, gb)
    for a, b in ((nan, 1.0), (1.0, nan), (nan, nan), (nan, -inf)):
        assert np.isnan(CT.lae32(a, b)) and all(np.isnan(g) for g in CT.lae_vjp32(a, b)), (a, b)
    # 17 apart: the smaller argument's share, exp(-17) = 4.1e-8, is below half
    # an ulp of the value and of the cotangent: both saturate in float32
    assert CT.lae32(17.0, 0.0) == F32(17.0) and CT.lae_vjp32(17.0, 0.0) == (F32(1.0), F32(0.0))
    assert CT.lae32(0.0, 10.0) > F32(10.0) and CT.lae_vjp32(0.0, 10.0)[0] > 0
    v, hit, miss = CT.pick([0.0, 1.0, 2.5, nan, -0.0], 0.0, 7.0, -inf)
    np.testing.assert_array_equal(v, np.array([7.0, -inf, -inf, -inf, 7.0], F32))
    np.testing.assert_array_equal(hit + miss, np.ones(5, F32))


def test_core_logaddexp_on_concrete_values():
    _, mx = _m()
    got = mx.logaddexp(np.array([1.0, 1000.0, -np.inf], F32), np.array([2.0, 0.0, -np.inf], F32))
    assert got.dtype == F32
    np.testing.assert_array_equal(got, np.logaddexp(np.array([1.0, 1000.0, -np.inf], F32),
                                                    np.array([2.0, 0.0, -np.inf], F32)))
    e = mx.logaddexp(_trace.Param("a", 0, ()), 1.0)
    assert isinstance(e, _trace.Expr) and e.op == CT.LAE and len(e.args) == 2


# ---- the lowering ----------------------------------------------------------------------------
def _nodes(lp, init):
    model = _trace.trace(lp, init, keep_order=True)
    assert len(model.terms) == 1 and model.terms[0].dist == _lib.MC_DIST_EXPR
    return model, [model.c_nodes[i] for i in range(model.n_nodes)]


@pytest.mark.parametrize("K", [1, 2, 3, 10])
def test_lowering_of_scalar_classes(K):
    """K class leaves, K PICK, K - 1 LOGADDEXP, the label, the -inf constant
    and the difference: 3K + 2 nodes, of which 2K + 2 are not class leaves."""
    m, mx = _m()
    y = (np.arange(CT.N_OBS) % K).astype(F32)
    model, nodes = _nodes(lambda p: mx.sum(m.Categorical(logits=p["e"]).log_prob(y)),
                          {"e": np.zeros(K, F32)})
    assert model.n_nodes == 3 * K + 2
    ops = [n.op for n in nodes]
    assert ops.count(CT.PICK) == K and ops.count(CT.LAE) == K - 1 and ops[-1] == _lib.MC_EX_SUB
    data = [n for n in nodes if n.op == L and n.leaf.kind == _lib.MC_OP_DATA]
    assert len(data) == 1 and model.data.size == CT.N_OBS          # one label array
    np.testing.assert_array_equal(model.data, y)
    consts = [n.leaf.value for n in nodes if n.op == L and n.leaf.kind == _lib.MC_OP_CONST]
    assert consts == [-np.inf]
    picks = [n for n in nodes if n.op == CT.PICK]
    assert [n.leaf.value for n in picks] == [float(k) for k in range(K)]   # classes in order
    for k, n in enumerate(picks):
        assert nodes[n.a].leaf.kind == _lib.MC_OP_DATA
        eta = nodes[n.b]
        assert eta.op == L and eta.leaf.kind == _lib.MC_OP_PSCALAR and eta.leaf.param_offset == k
    root = nodes[-1]
    assert nodes[root.a].op == CT.PICK and nodes[root.a].leaf.value == K - 1
    assert nodes[root.b].op == (CT.LAE if K > 1 else L)


def test_node_array_forms():
    """K = 3 scalar classes fit the NMAX = 16 evaluator, the K = 3 regression
    with a reference class takes NMAX = 32; one leaf per predictor array."""
    m, mx = _m()
    d = CT.data()
    model, _ = _nodes(lambda p: mx.sum(m.Categorical(logits=p["e"]).log_prob(d.y)),
                      {"e": np.zeros(3, F32)})
    assert model.n_nodes == 11 <= 16
    lik = CT.likelihood(d)
    model, nodes = _nodes(lik.log_likelihood, {k: F32(0) for k in CT.REG_SHAPES})
    assert 16 < model.n_nodes == 18 <= 32
    assert model.data.size == 2 * d.N                              # the label and x, once each
    # what the class docstring says fits: 6K + 3 at K = 4, 9K + 4 at K = 3
    x2 = np.cos(d.x).astype(F32)
    model, _ = _nodes(lambda p: mx.sum(m.Categorical(
        logits=[p["a"][k] + p["b"][k] * d.x for k in range(4)]).log_prob(d.y)),
        {"a": np.zeros(4, F32), "b": np.zeros(4, F32)})
    assert model.n_nodes == 27
    model, _ = _nodes(lambda p: mx.sum(m.Categorical(
        logits=[p["a"][k] + p["b"][k] * d.x + p["c"][k] * x2 for k in range(3)]).log_prob(d.y)),
        {"a": np.zeros(3, F32), "b": np.zeros(3, F32), "c": np.zeros(3, F32)})
    assert model.n_nodes == 31


def _eval(root, values):
    """The traced expression on the host in float32 with the table's nodes."""
    def ev(e):
        if e.op == L:
            return values[e.leaf.name] if isinstance(e.leaf, _trace.Param) else np.asarray(e.leaf, F32)
        a = [None if x is None else ev(x) for x in e.args]
        with np.errstate(all="ignore"):
            return {_lib.MC_EX_ADD: lambda: a[0] + a[1], _lib.MC_EX_SUB: lambda: a[0] - a[1],
                    _lib.MC_EX_MUL: lambda: a[0] * a[1], _lib.MC_EX_LOG: lambda: np.log(a[0]),
                    _lib.MC_EX_GT: lambda: (a[0] > a[1]).astype(F32),
                    _lib.MC_EX_WHERE: lambda: np.where(a[0] != 0, a[1], a[2]).astype(F32),
                    CT.LAE: lambda: CT.lae32(a[0], a[1]),
                    CT.PICK: lambda: CT.pick(a[0], e.leaf, a[1], a[2])[0]}[e.op]()
    return ev(root)


def test_probs_lowering_is_guarded_and_normalised():
    m, _ = _m()
    P1, P2 = _trace.Param("p1", 0, ()), _trace.Param("p2", 1, ())
    y = np.array([0.0, 1.0, 2.0, 3.0], F32)
    root = m.Categorical(probs=[P1, P2, 1.0 - P1 - P2]).log_prob(y).terms[0].expr
    assert root.op == _lib.MC_EX_WHERE
    got = _eval(root, {"p1": F32(0.2), "p2": F32(0.5)})
    np.testing.assert_allclose(got[:3], np.log([0.2, 0.5, 0.3]), rtol=2e-6)
    assert got[3] == -np.inf
    for p1, p2 in ((0.7, 0.4), (-0.1, 0.5), (0.5, 0.0), (0.5, 0.5)):     # outside the simplex
        assert np.all(_eval(root, {"p1": F32(p1), "p2": F32(p2)}) == -np.inf), (p1, p2)
    # un-normalised probabilities: p / sum p, the reference's rule
    root = m.Categorical(probs=[P1, P2]).log_prob(np.array([0.0, 1.0], F32)).terms[0].expr
    np.testing.assert_allclose(_eval(root, {"p1": F32(2.0), "p2": F32(6.0)}),
                               np.log([0.25, 0.75]), rtol=2e-6)


def test_traced_log_prob_on_the_host_equals_the_table():
    m, _ = _m()
    d = CT.data()
    P = {k: _trace.Param(k, i, ()) for i, k in enumerate(CT.REG_SHAPES)}
    root = m.Categorical(logits=[0.0, P["a1"] + P["b1"] * d.x, P["a2"] + P["b2"] * d.x]
                         ).log_prob(d.y).terms[0].expr
    q = np.array([0.3, 0.8, -0.4, -0.6], F32)
    got = _eval(root, dict(zip(CT.REG_SHAPES, q)))
    np.testing.assert_allclose(got, CT.likelihood(d).ll(q), rtol=1e-5, atol=1e-6)


# ---- errors ------------------------------------------------------------------------------------
def test_tracer_errors():
    m, mx = _m()
    P = _trace.Param("p", 0, (3,))
    y = np.array([0.0, 1.0, 2.0], F32)
    with pytest.raises(_trace.TraceError, match="must be data or a constant"):
        m.Categorical(logits=P).log_prob(_trace.Param("y", 3, (3,)))          # a traced label
    with pytest.raises(_trace.TraceError, match="broadcast"):                # ragged shapes
        m.Categorical(logits=[P[0], P[1] * np.ones(4, F32), 0.0]).log_prob(y)
    with pytest.raises(_trace.TraceError, match="broadcast"):
        m.Categorical(logits=[P[0], P[1]]).log_prob(y) + m.Categorical(
            logits=[P[0], P[1] * np.ones(4, F32)]).log_prob(y)
    with pytest.raises(_trace.TraceError, match="1-D"):
        m.Categorical(logits=_trace.Param("s", 0, ()))
    # over the node limit: K = 11 scalar classes, a K = 5 regression
    big = _trace.Param("e", 0, (11,))
    with pytest.raises(_trace.TraceError, match="at most 32"):
        _trace.trace(lambda p: mx.sum(m.Categorical(logits=p["e"]).log_prob(y)),
                     {"e": np.zeros(11, F32)})
    assert m.Categorical(logits=big).num_categories == 11
    x = np.linspace(-1, 1, 3).astype(F32)
    with pytest.raises(_trace.TraceError, match="at most 32"):
        _trace.trace(lambda p: mx.sum(m.Categorical(
            logits=[p["a"][k] + p["b"][k] * x for k in range(5)]).log_prob(y)),
            {"a": np.zeros(5, F32), "b": np.zeros(5, F32)})
    # a log mass under mx.where: a log density is no expression operand
    with pytest.raises(_trace.TraceError):
        mx.where(np.array([1.0, 0.0, 1.0], F32), m.Categorical(logits=P).log_prob(y), 0.0)


P0 = {"kind": _lib.MC_OP_PSCALAR, "param_offset": 0}
P1 = {"kind": _lib.MC_OP_PSCALAR, "param_offset": 1}
P2 = {"kind": _lib.MC_OP_PSCALAR, "param_offset": 2}
DATA = {"kind": _lib.MC_OP_DATA, "pool_offset": 0}
K1 = {"value": 1.0}


@pytest.mark.parametrize("nodes,code,msg", [
    # a parameter leaf, and a non-leaf node, as the label
    ([(L, -1, -1, -1, P0), (L, -1, -1, -1, P1), (L, -1, -1, -1, P2), (30, 0, 1, 2, K1)],
     _lib.MC_ERR_UNSUPPORTED, b"pick node's label y"),
    ([(L, -1, -1, -1, DATA), (_lib.MC_EX_NEG, 0, -1, -1, None), (L, -1, -1, -1, P1),
      (L, -1, -1, -1, P2), (30, 1, 2, 3, K1)], _lib.MC_ERR_UNSUPPORTED, b"pick node's label y"),
    # arity
    ([(L, -1, -1, -1, DATA), (L, -1, -1, -1, P0), (30, 0, 1, -1, K1)], _lib.MC_ERR_INVALID,
     b"bad arguments"),
    ([(L, -1, -1, -1, P0), (29, 0, -1, -1, None)], _lib.MC_ERR_INVALID, b"bad arguments"),
    ([(L, -1, -1, -1, P0), (L, -1, -1, -1, P1), (29, 0, 1, 1, None)], _lib.MC_ERR_INVALID,
     b"bad arguments"),
    # 28 stays unassigned (tests/test_discrete_host.py holds it to be unknown)
    ([(L, -1, -1, -1, P0), (28, 0, -1, -1, None)], _lib.MC_ERR_INVALID, b"unknown op"),
    ([(L, -1, -1, -1, P0), (31, 0, -1, -1, None)], _lib.MC_ERR_INVALID, b"unknown op"),
])
def test_node_validation(nodes, code, msg):
    rc, err = _expr_program(nodes)
    assert rc == code and msg in err, (rc, err)


def test_valid_nodes_make_a_host_program():
    lib = _lib.load()
    m, mx = _m()
    lik = CT.likelihood()
    lib.mc_debug_program_host_only(1)
    try:
        prog = _trace.Program(_trace.trace(lik.log_likelihood, {k: F32(0) for k in CT.REG_SHAPES}))
        assert prog.num_elements == CT.N_OBS
        # no sampler is recorded for a Categorical term
        assert lib.mc_program_num_count_terms(prog.handle) == 0
    finally:
        lib.mc_debug_program_host_only(0)
