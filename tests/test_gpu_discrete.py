"""Bernoulli / Binomial / Poisson on the device: the count nodes on every
interpreter form against the float64 table of tests/_discrete.py (ulp bounds
derived there), the compiled evaluators against the interpreter, the three
N = 67 models against the oracle (tape, sampler decisions), two conjugate
posteriors, WAIC / PSIS-LOO on the count likelihoods and posterior predictive
replicates of count terms against the host definition."""
import functools

import numpy as np
import pytest

import _discrete as DS
import _expr_ops as X
import _pointwise as PW
import _psis as PS
from _near_tie import compare_trace, log_u, tie_bound
from oracle import samplers as S

pytestmark = pytest.mark.gpu
F32 = np.float32
NODES = list(DS.OP)


# ---- the nodes on the interpreter forms ------------------------------------------------
@functools.lru_cache(maxsize=None)
def _device(name):
    rows, nb = DS.eta_rows(name)
    out = {"rows": rows, "nb": nb, "V": DS.run_V(name, rows), "V32": DS.run_V(name, rows, "V32"),
           "VF": DS.run_V(name, rows, "VF")}
    etas = DS.const_etas(name)
    out["S"] = {c: DS.run_S(name, c[0], c[1], etas) for c in DS.S_COMBOS[name]}
    return out


def _table(name, rows):
    y, n = DS.yn_data(name)
    y, n = np.broadcast_to(y, rows.shape), np.broadcast_to(n, rows.shape)
    return y, n


@pytest.mark.parametrize("name", NODES)
def test_node_value_and_vjp_bulk(gpu, name):
    d = _device(name)
    rows = d["rows"][:d["nb"]]
    y, n = _table(name, rows)
    ok = DS._support(name, y.astype(np.float64), n.astype(np.float64))
    uf, ug = DS.units(name, y, n, rows)
    ef = np.abs(d["VF"][:d["nb"]].astype(np.float64) - DS.fwd64(name, y, n, rows))[ok] / uf[ok]
    eg = np.abs(d["V"][:d["nb"]].astype(np.float64) - DS.vjp64(name, y, n, rows))[ok] / ug[ok]
    print(f"{name}: max error value {ef.max():.3f} (gate {DS.FWD_GATE[name]}), "
          f"VJP {eg.max():.3f} (gate {DS.VJP_GATE[name]}) over {ok.sum()} points")
    assert ef.max() <= DS.FWD_GATE[name]
    assert eg.max() <= DS.VJP_GATE[name]
    # outside the support: -inf, no cotangent (whatever eta is)
    assert (~ok).any()
    assert np.all(d["VF"][:d["nb"]][~ok] == -np.inf) and np.all(d["V"][:d["nb"]][~ok] == 0.0)


@pytest.mark.parametrize("name", NODES)
def test_node_edges(gpu, name):
    d = _device(name)
    rows = d["rows"][d["nb"]:]
    assert rows.shape[0] == len(DS.ETA_EDGES)
    y, n = _table(name, rows)
    flat = lambda a: np.ascontiguousarray(a).reshape(-1)   # noqa: E731
    y, n, e = flat(y), flat(n), flat(rows)
    uf, ug = DS.units(name, y, n, e)
    skip = np.zeros(e.shape, bool)
    vf, vg = flat(d["VF"][d["nb"]:]), flat(d["V"][d["nb"]:])
    bad = X.edge_failures(vf, DS.fwd64(name, y, n, e), DS.fwd32(name, y, n, e), skip,
                          DS.FWD_GATE[name], unit=uf)
    assert bad.size == 0, [(float(y[i]), float(n[i]), float(e[i]), float(vf[i])) for i in bad[:8]]
    bad = X.edge_failures(vg, DS.vjp64(name, y, n, e), DS.vjp32(name, y, n, e), skip,
                          DS.VJP_GATE[name], unit=ug)
    assert bad.size == 0, [(float(y[i]), float(n[i]), float(e[i]), float(vg[i])) for i in bad[:8]]
    ok = DS._support(name, y.astype(np.float64), n.astype(np.float64))
    assert np.all(vf[~ok] == -np.inf) and np.all(vg[~ok] == 0.0)
    # the saturated logit keeps its value: no 0 * -inf
    if name == "bernoulli":
        sel = (y == 0) & (e == 90.0)
        assert sel.any() and np.all(vf[sel] == F32(-90.0))
    if name == "poisson":
        sel = (y == 0) & np.isneginf(e)
        assert sel.any() and np.all(vf[sel] == 0.0)
    if name == "binomial":
        sel = (y == 0) & (n == 0) & np.isfinite(e)
        assert sel.any() and np.all(vf[sel] == 0.0) and np.all(vg[sel] == 0.0)


@pytest.mark.parametrize("name", NODES)
def test_node_forms_agree(gpu, name):
    """V (NMAX = 16) and V32 (NMAX = 32) bit-identical per element; form S
    (one element, the wave-task path) bit-identical to forms VF / V at the
    elements that hold its (y, n), on the rows constant in eta."""
    d = _device(name)
    assert X.same_bits(d["V"], d["V32"]).all()
    y, n = DS.yn_data(name)
    const_v, const_g = d["VF"][DS.N_BULK_ROWS:], d["V"][DS.N_BULK_ROWS:]
    for (cy, cn), (lp, g) in d["S"].items():
        cols = np.nonzero((y == cy) & (n == cn))[0]
        assert cols.size
        for j in cols[:3]:
            assert X.same_bits(lp, const_v[:, j]).all(), (name, cy, cn, "value")
            assert X.same_bits(g, const_g[:, j]).all(), (name, cy, cn, "VJP")


@pytest.mark.parametrize("name,scale", [("bernoulli", 0.3), ("binomial", 0.1), ("poisson", 0.1)])
def test_node_value_only_pass(gpu, name, scale):
    """metropolis_hastings on a form-V program (every y inside the support)
    for 20 iterations on the interpreter's value-only pass: decisions equal
    the float64 restatement's up to a proven near-tie (tests/_near_tie.py)."""
    import torch

    import mlx_mcmc_amd as m
    from mlx_mcmc_amd import _lib, _trace

    rng = np.random.default_rng(9)
    n = rng.integers(0, 12, X.N_VEC).astype(F32) if name == "binomial" else None
    if name == "bernoulli":
        y = rng.integers(0, 2, X.N_VEC).astype(F32)
    elif name == "binomial":
        y = np.floor(rng.random(X.N_VEC) * (n + 1)).astype(F32)     # 0 <= y <= n, n = 0 among them
        assert np.all(y <= n) and (n == 0).any()
    else:
        y = rng.poisson(2.0, X.N_VEC).astype(F32)

    def log_prob(p):
        return _trace.expr_term(DS._node(name, y, n, _trace.Expr.of(p["a"]))).sum()

    f = DS.torch_node(name)
    ty = torch.tensor(y.astype(np.float64))
    tn = None if n is None else torch.tensor(n.astype(np.float64))

    def oracle(p):
        return f(ty, tn, p["a"].to(torch.float64)).sum()
    init = {"a": np.full(X.N_VEC, 0.4, F32)}
    nit, seed = 20, 5
    lib = _lib.load()
    lib.mc_debug_expr_jit(0)
    try:
        _, _, info = m.metropolis_hastings(log_prob, init, num_samples=nit, proposal_scale=scale,
                                           random_seed=seed, return_info=True, return_trace=True)
    finally:
        lib.mc_debug_expr_jit(-1)
    ref = S.metropolis_hastings(oracle, init, num_samples=nit, proposal_scale=scale,
                                random_seed=seed)
    acc, racc = info.trace["accepted"][0].astype(bool), np.array(ref.trace["accepted"])
    assert 0 < racc.sum() < nit, "mixed decisions"
    lu = log_u(m.random.key(seed).seed, 0, nit)
    same = nit
    for i in range(nit):
        tie = tie_bound(ref.trace["logp"][i])
        if acc[i] != racc[i]:
            assert abs(float(lu[i]) - ref.trace["ratio"][i]) <= tie, (name, i)
            same = i
            break
        assert abs(float(info.trace["energy"][0][i]) - ref.trace["logp"][i]) <= tie, (name, i)
    assert same >= 10, f"{name}: compared only {same} of {nit} iterations"


# ---- compiled evaluators -----------------------------------------------------------------
def _sample(algo, name, jit):
    import mlx_mcmc_amd as m
    from mlx_mcmc_amd import _lib, _trace

    lib = _lib.load()
    lib.mc_debug_expr_jit(1 if jit else 0)
    try:
        lp, init = DS.posterior_model(name, False)
        if algo == "hmc":
            s, _, info = m.hmc(lp, init, num_samples=12, num_warmup=12, step_size=0.02,
                               num_leapfrog_steps=5, key=m.random.key(4), num_chains=16,
                               progress=False, return_info=True, return_trace=True)
        elif algo == "nuts":
            s, _, info = m.nuts(lp, init, num_samples=8, num_warmup=8, step_size=0.02,
                                max_tree_depth=6, key=m.random.key(4), num_chains=16,
                                progress=False, return_info=True, return_trace=True)
        else:
            s, _, info = m.metropolis_hastings(lp, init, num_samples=40, proposal_scale=0.05,
                                               random_seed=4, num_chains=16, return_info=True,
                                               return_trace=True)
        state = lib.mc_program_expr_jit(_trace.compile_model(lp, init).handle)
    finally:
        lib.mc_debug_expr_jit(-1)
    return s, info, state


@pytest.mark.parametrize("algo,name", [("hmc", "bernoulli"), ("hmc", "binomial"), ("hmc", "poisson"),
                                       ("nuts", "poisson"), ("mh", "bernoulli")])
def test_tape_jit_bit_identical_to_interpreter(gpu, algo, name):
    s0, i0, st0 = _sample(algo, name, False)
    s1, i1, st1 = _sample(algo, name, True)
    assert st0 == 0 and st1 == 1, (st0, st1)
    for k in s0:
        np.testing.assert_array_equal(np.asarray(s0[k]), np.asarray(s1[k]), err_msg=k)
    for k, v in i0.trace.items():
        np.testing.assert_array_equal(v, i1.trace[k], err_msg=k)


N_LANE = 250


def _lane_model(oracle):
    """theta[250] under Normal(0, 1) and a broadcast intercept, nine terms of
    250 data elements each (the lane planner takes expression programs from
    2048 elements on): 0.1 sum_i node(y_ki; a + theta_i x_ki), Bernoulli and
    Poisson alternating — both packed cases of ex2_fwd / ex2_bwd."""
    rng = np.random.default_rng(61)
    xs = rng.uniform(0.5, 2.0, (9, N_LANE)).astype(F32) * rng.choice([-1.0, 1.0], (9, N_LANE)).astype(F32)
    ys = [(rng.integers(0, 2, N_LANE) if k % 2 == 0 else rng.poisson(1.5, N_LANE)).astype(F32)
          for k in range(9)]
    names = ["bernoulli" if k % 2 == 0 else "poisson" for k in range(9)]
    init = {"theta": np.zeros(N_LANE, F32), "a": F32(0.0)}
    if oracle:
        import torch
        t = lambda v: torch.tensor(np.asarray(v, np.float64))   # noqa: E731

        def log_prob(p):
            th, a = p["theta"].to(torch.float64), p["a"].to(torch.float64)
            lp = (float(X.C0_NORMAL) - 0.5 * th ** 2).sum() + (float(X.C0_NORMAL) - 0.5 * a ** 2)
            for k in range(9):
                lp = lp + float(F32(0.1)) * DS.torch_node(names[k])(t(ys[k]), None,
                                                                    a + th * t(xs[k])).sum()
            return lp
        return log_prob, init

    def log_prob(p):
        import mlx_mcmc_amd as m
        import mlx_mcmc_amd.core as mx
        from mlx_mcmc_amd import _trace
        lp = mx.sum(m.Normal(0, 1).log_prob(p["theta"])) + m.Normal(0, 1).log_prob(p["a"])
        for k in range(9):
            eta = _trace.Expr.of(p["a"] + p["theta"] * xs[k])
            lp = lp + 0.1 * _trace.expr_term(DS._node(names[k], ys[k], None, eta)).sum()
        return lp
    return log_prob, init


def _two_leapfrogs(lanes, q0, seed, eps):
    import torch

    from mlx_mcmc_amd import _engine, _lib, _trace

    lib = _lib.load()
    lp, init = _lane_model(False)
    C = q0.shape[0]
    lib.mc_debug_expr_jit(-1 if lanes else 0)
    try:
        prog = (_trace.compile_model(lp, init, slices=4, slice_kernel="lanes") if lanes
                else _trace.compile_model(lp, init, slices=1))
        if lanes:
            assert prog.slice_kernel == "lanes" and prog.num_slices == 4, prog.kernel_note
        cs = _engine.ChainSet(prog, C, q0, eps)
        smp = torch.empty((C, 1, prog.D), dtype=torch.float32, device=cs.device)
        tr = _engine.make_trace(C, 0, 1, cs.device)
        cs.run_hmc(samples=smp, trace=tr, iter_begin=0, iter_count=1, chain_offset=0, num_warmup=0,
                   num_samples=1, sample_begin=0, sample_capacity=1, seed=seed, step_size=eps,
                   target_accept=0.8, num_leapfrog_steps=2, adapt_step_size=False)
        torch.cuda.synchronize()
        cs.check_status()
        assert lib.mc_program_expr_jit(prog.handle) == (1 if lanes else 0)
        return smp[:, 0].cpu().numpy(), tr.numpy()
    finally:
        lib.mc_debug_expr_jit(-1)


def test_lane_jit_two_leapfrogs(gpu):
    """The lane kernel's pair code (ex2_fwd / ex2_bwd's packed Bernoulli and
    Poisson cases) against the interpreter tape over two leapfrog steps from
    16 starts (tests/test_gpu_expr_ops.py test_lane_jit_two_leapfrogs: the
    second step's gradient is the running kernel's own).  eval.h states the
    pair code bit-identical per component, and an element of theta sums its
    terms in term order on both kernels: the accepted draws are held to equal
    bits, and to the float64 restatement's position."""
    from oracle import philox as R

    eps, seed, C = 0.05, 20, 16     # (the float64 restatement accepts all 16)
    q0 = np.random.default_rng(7).normal(0.0, 0.3, (C, N_LANE + 1)).astype(F32)
    ql, tl = _two_leapfrogs(True, q0, seed, eps)
    qt, tt = _two_leapfrogs(False, q0, seed, eps)
    np.testing.assert_array_equal(tl["accepted"], tt["accepted"])
    assert tl["accepted"][:, 0].sum() >= 14
    olp, oinit = _lane_model(True)
    M = S.EagerModel(olp, oinit)
    for c in range(C):
        if not tl["accepted"][c, 0]:
            np.testing.assert_array_equal(ql[c], q0[c])
            continue
        q = q0[c].copy()
        p = np.asarray(R.momentum(seed, c, 0, M.D), F32)
        for _ in range(2):
            q, p = M.leapfrog(q, p, eps)
        np.testing.assert_allclose(ql[c], q, rtol=2e-5, atol=2e-6)
    ndiff = int((ql[:, :N_LANE] != qt[:, :N_LANE]).sum())
    assert ndiff == 0, f"{ndiff} elements of theta differ between lanes and tape"


def _capture(monkeypatch):
    from mlx_mcmc_amd import _trace
    made = []
    orig = _trace.compile_model

    def compile_model(*a, **k):
        made.append(orig(*a, **k))
        return made[-1]
    monkeypatch.setattr(_trace, "compile_model", compile_model)
    return made


def _poisson_lanes():
    """A Poisson regression per parameter: theta[250] under Normal(0, 1), nine
    Poisson(log_rate = theta x_k) terms (the sliced layout of _lane_model
    without its broadcast intercept)."""
    rng = np.random.default_rng(62)
    xs = rng.uniform(0.5, 1.5, (9, N_LANE)).astype(F32) * rng.choice([-1.0, 1.0], (9, N_LANE)).astype(F32)
    ys = rng.poisson(1.5, (9, N_LANE)).astype(F32)

    def log_prob(p):
        import mlx_mcmc_amd as m
        import mlx_mcmc_amd.core as mx
        lp = mx.sum(m.Normal(0, 1).log_prob(p["theta"]))
        for k in range(9):
            lp = lp + 0.1 * mx.sum(m.Poisson(log_rate=p["theta"] * xs[k]).log_prob(ys[k]))
        return lp
    return log_prob, {"theta": np.zeros(N_LANE, F32)}


def test_poisson_on_sliced_nuts_and_mh(gpu, monkeypatch):
    """One NUTS run on k_nuts_sl and one MH run on k_mh_sl of a Poisson
    regression, against the interpreter tape: trees identical for >= 6
    iterations per chain, MH decisions identical over 40 iterations."""
    import mlx_mcmc_amd as m
    from mlx_mcmc_amd import _lib

    lib = _lib.load()
    lp, init = _poisson_lanes()
    C = 8
    q0 = np.random.default_rng(3).normal(0.0, 0.3, (C, N_LANE)).astype(F32)
    kw = dict(num_samples=8, num_warmup=4, step_size=0.05, max_tree_depth=6,
              adapt_step_size=False, key=m.random.key(12), num_chains=C, progress=False,
              return_info=True, return_trace=True, initial_positions=q0)
    made = _capture(monkeypatch)
    _, _, a = m.nuts(lp, init, **kw)
    assert a.extra["kernel"] == "sliced", (a.extra, made[-1].kernel_note)
    lib.mc_debug_expr_jit(0)
    try:
        _, _, b = m.nuts(lp, init, nuts_kernel="tape", **kw)
    finally:
        lib.mc_debug_expr_jit(-1)
    assert b.extra["kernel"] == "tape", b.extra
    for c in range(C):
        same = 0
        for i in range(12):
            if (a.trace["tree_depth"][c][i] != b.trace["tree_depth"][c][i]
                    or a.trace["n_leapfrog"][c][i] != b.trace["n_leapfrog"][c][i]):
                break
            same += 1
        assert same >= 6, f"chain {c}: trees differ at iteration {same}"
    assert np.any(b.trace["tree_depth"] >= 2)
    kw = dict(num_samples=40, proposal_scale=0.02, random_seed=5, num_chains=C, return_info=True,
              return_trace=True, initial_positions=q0)
    _, _, a = m.metropolis_hastings(lp, init, **kw)
    assert lib.mc_program_mh_sliced(made[-1].handle) == 1, made[-1].kernel_note
    lib.mc_debug_expr_jit(0)
    lib.mc_debug_mh_sliced(0)
    try:
        _, _, b = m.metropolis_hastings(lp, init, **kw)
        assert lib.mc_program_mh_sliced(made[-1].handle) == 0
    finally:
        lib.mc_debug_mh_sliced(-1)
        lib.mc_debug_expr_jit(-1)
    np.testing.assert_array_equal(a.trace["accepted"], b.trace["accepted"])
    acc = a.trace["accepted"].astype(bool)
    assert 0 < acc.mean() < 1


# ---- the three models against the oracle -----------------------------------------------------
def _points(prog, init, k=6, spread=0.3, seed=7):
    rng = np.random.default_rng(seed)
    base = prog.layout.flatten(init)
    return np.stack([base + rng.normal(0, spread, base.size).astype(F32) for _ in range(k)])


@pytest.mark.parametrize("name", NODES)
def test_tape_matches_autograd(gpu, name):
    """tests/test_gpu_expr.py test_expr_tape_matches_autograd's bars."""
    from mlx_mcmc_amd import _engine, _lib, _trace

    lp_fn, init = DS.posterior_model(name, False)
    prog = _trace.compile_model(lp_fn, init)
    assert any(t.dist == _lib.MC_DIST_EXPR for t in prog.model.terms)
    assert prog.slice_kernel == "unsliced"
    olp, oinit = DS.posterior_model(name, True)
    M = S.EagerModel(olp, oinit)
    pts = _points(prog, init)
    lp, g = _engine.logp_grad(prog, pts)
    lp, g = lp.cpu().numpy(), g.cpu().numpy()
    for i, q in enumerate(pts):
        rl, rg = M.logp_grad(q)
        assert abs(lp[i] - rl) <= 2e-6 * max(1.0, abs(rl)) * 50, (i, lp[i], rl)
        np.testing.assert_allclose(g[i], rg, rtol=1e-4, atol=1e-3 * max(1.0, np.abs(rg).max()))
    lp2, g2 = _engine.logp_grad(prog, pts)
    assert np.array_equal(lp, lp2.cpu().numpy()) and np.array_equal(g, g2.cpu().numpy())


# (starts away from eta = 0; step sizes at which the float64 restatement's
# decisions are a mix, checked with oracle.samplers on the CPU)
START = {"bernoulli": ({"a": 0.8, "b": 1.2}, 0.1),
         "poisson": ({"a": 1.0, "b": 0.3}, 0.04)}


@pytest.mark.parametrize("name", ["bernoulli", "poisson"])
def test_hmc_trace_matches_oracle(gpu, name):
    import mlx_mcmc_amd as m

    lp, _ = DS.posterior_model(name, False)
    olp, _ = DS.posterior_model(name, True)
    start, eps = START[name]
    start = {k: F32(v) for k, v in start.items()}
    seed, n = 3, 40
    kw = dict(num_samples=40, num_warmup=40, step_size=eps, num_leapfrog_steps=10)
    _, _, info = m.hmc(lp, start, key=m.random.key(seed), progress=False, return_info=True,
                       return_trace=True, **kw)
    assert info.extra["kernel"] == "unsliced"
    ref = S.hmc(olp, start, seed=seed, **kw)
    tr = info.trace
    gpu_c = {"accepted": tr["accepted"][0][:n], "ratio": tr["accept_stat"][0][:n],
             "step_size": tr["step_size"][0][:n], "energy": tr["energy"][0][:n]}
    ref_c = {k: np.asarray(ref.trace[k])[:n] for k in ("accepted", "ratio", "step_size", "energy")}
    ref_c["log_u"] = log_u(seed, 0, n)
    same = compare_trace(gpu_c, ref_c, f"{name} seed {seed}", verbose=True)
    assert same >= 30 and np.asarray(ref.trace["accepted"][:same]).any()


@pytest.mark.parametrize("name", ["bernoulli", "poisson"])
def test_nuts_trees_match_oracle(gpu, name):
    import mlx_mcmc_amd as m

    lp, _ = DS.posterior_model(name, False)
    olp, _ = DS.posterior_model(name, True)
    start = {k: F32(v) for k, v in START[name][0].items()}
    n_w, n_s = 30, 10
    # (from step size 0.02: from the default 0.1 dual averaging drives the
    # Poisson chain into exp overflow after a dozen iterations)
    _, _, info = m.nuts(lp, start, num_samples=n_s, num_warmup=n_w, step_size=0.02,
                        key=m.random.key(2), progress=False, return_info=True, return_trace=True)
    assert info.extra["kernel"] == "tape"
    ref = S.nuts(olp, start, num_samples=n_s, num_warmup=n_w, step_size=0.02, seed=2)
    same = 0
    for i in range(n_w + n_s):
        if (info.trace["tree_depth"][0][i] != ref.trace["depth"][i]
                or info.trace["n_leapfrog"][0][i] != ref.trace["leaves"][i]):
            break
        same += 1
    assert same >= 10, f"trees diverged at iteration {same}"
    assert max(ref.trace["depth"][:same]) >= 2


@pytest.mark.parametrize("name", ["bernoulli", "poisson"])
def test_mh_decisions_match_oracle(gpu, name):
    import mlx_mcmc_amd as m

    lp, _ = DS.posterior_model(name, False)
    olp, _ = DS.posterior_model(name, True)
    start = {k: float(v) for k, v in START[name][0].items()}
    n = 150
    s, _, info = m.metropolis_hastings(lp, start, num_samples=n, proposal_scale=0.15,
                                       random_seed=5, return_info=True, return_trace=True)
    ref = S.metropolis_hastings(olp, start, num_samples=n, proposal_scale=0.15, random_seed=5)
    acc = info.trace["accepted"][0].astype(bool)
    assert list(acc) == ref.trace["accepted"] and 0 < acc.mean() < 1
    np.testing.assert_allclose(s["a"], ref.samples[:, 0], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("name,eps", [("binomial", 0.0045), ("poisson", 0.06)])
def test_conjugate_posterior_mean(gpu, name, eps):
    """Beta-Binomial (probs =) and Gamma-Poisson (rate =): the posterior mean
    within 4 MCSE of the exact value (the MCSE from the spread of the chain
    means, as the project's other posterior tests take it).  A fixed step
    size, ten steps of it about 1.5 posterior standard deviations (the
    reference's warmup rule leaves single chains stuck or resonant on these
    one-parameter posteriors); oracle.samplers.hmc at the same settings
    meets the bar on the CPU with 8 chains."""
    import mlx_mcmc_amd as m

    lp, init, mean, sd, pname = DS.conjugate(name)
    s, _, info = m.hmc(lp, init, num_samples=500, num_warmup=100, step_size=eps,
                       num_leapfrog_steps=10, adapt_step_size=False, key=m.random.key(1),
                       num_chains=32, progress=False, return_info=True)
    d = np.asarray(s[pname])
    assert d.shape == (32, 500) and np.all(info.accept_rate > 0.3)
    mcse = d.mean(1).std() / np.sqrt(d.shape[0])
    print(f"{name}: mean {d.mean():.5f} exact {mean:.5f} (MCSE {mcse:.5f}), sd {d.std():.4f} "
          f"exact {sd:.4f}")
    assert abs(d.mean() - mean) < 4 * mcse
    assert abs(d.std() - sd) < 0.1 * sd


def test_bernoulli_takes_the_hand_written_logistic_route(gpu):
    """N = 100 K, 64 chains, the default plan: Bernoulli(logits = a + b x)
    runs on the kernel route of workloads.logistic_regression."""
    import mlx_mcmc_amd as m
    import mlx_mcmc_amd.core as mx
    import workloads as W
    from mlx_mcmc_amd import _trace

    n = 100_000
    x, y = W.logistic_data(n)
    hand, _ = W.logistic_regression(W.ns_product(), n)

    def node(p):
        lp = m.Normal(0, 5).log_prob(p["a"]) + m.Normal(0, 5).log_prob(p["b"])
        return lp + mx.sum(m.Bernoulli(logits=p["a"] + p["b"] * x).log_prob(y))
    init = {"a": F32(-0.3), "b": F32(1.1)}
    routes = []
    for lp in (hand, node):
        prog = _trace.compile_model(lp, init)
        _, _, info = m.hmc(lp, init, num_samples=2, num_warmup=2, step_size=1e-3,
                           num_leapfrog_steps=3, key=m.random.key(1), num_chains=64,
                           progress=False, return_info=True)
        routes.append((info.extra["kernel"], prog.slice_kernel, prog.num_slices))
    print("routes (hand-written, Bernoulli):", routes)
    assert routes[0] == routes[1] and routes[0][0] != "unsliced", routes


# ---- WAIC and PSIS-LOO -------------------------------------------------------------------------
def _D():
    from mlx_mcmc_amd import diagnostics
    return diagnostics


@pytest.mark.parametrize("name", ["bernoulli", "poisson"])
def test_waic_and_loo(gpu, name):
    """C = 3, S = 37 as tests/_pointwise.py: the matrix and statistics at its
    bars, WAIC from them; PSIS-LOO at tests/test_gpu_psis.py's bars."""
    model = DS.likelihood(name)
    q = DS.draws(model)
    lay = DS.layout_of(model)
    got = _D().pointwise_log_likelihood(model.log_likelihood, q, lay, matrix=True, group=False)
    ref = model.ll(q, np.float64)
    mat = got["matrix"].cpu().numpy()
    assert mat.shape == (3, 37, DS.N_OBS)
    np.testing.assert_allclose(mat, ref, rtol=PW.RTOL, atol=PW.ATOL)
    own, model64 = PW.stats_of(mat), PW.stats_of(ref)
    for f in PW.FIELDS:
        np.testing.assert_allclose(got[f], own[f], rtol=1e-10, atol=0, err_msg=f)
        np.testing.assert_allclose(got[f], model64[f], rtol=PW.RTOL, atol=PW.ATOL, err_msg=f)
    w = _D().waic(model.log_likelihood, q, lay, group=False)
    wr = PW.waic_of(ref)
    np.testing.assert_allclose(w["pointwise"]["elpd_waic"], wr["elpd_i"], rtol=PW.RTOL, atol=PW.ATOL)
    np.testing.assert_allclose(w["elpd_waic"], wr["elpd_waic"], rtol=1e-5)
    loo = _D().loo(model.log_likelihood, q, lay, group=False, tail=True)
    own = PS.psis_matrix(mat.reshape(-1, DS.N_OBS))
    r64 = PS.psis_matrix(ref.reshape(-1, DS.N_OBS))
    assert loo["tail_len"] == own["tail_len"] == 23
    pw = loo["pointwise"]
    np.testing.assert_array_equal(loo["tail_n"], own["n"])
    for f, g in (("khat", pw["khat"]), ("elpd", pw["elpd_loo"])):
        np.testing.assert_allclose(g, own[f], rtol=1e-10, atol=0, err_msg=f)
    np.testing.assert_allclose(pw["elpd_loo"], r64["elpd"], rtol=PS.RTOL, atol=PS.ATOL)
    np.testing.assert_allclose(pw["khat"], r64["khat"], rtol=PS.RTOL, atol=PS.ATOL)
    assert loo["n_nonfinite"] == 0


# ---- posterior predictive replicates -------------------------------------------------------------
STAT = ("n", "mean", "m2", "below", "nonfinite", "equal")


def _pp(model, q, **kw):
    return _D().posterior_predictive(model.log_likelihood, q, DS.layout_of(model), group=False,
                                     **kw)


def _host_rep(model, q, seed, chain0=0, iter0=0):
    kind, tot, eta, y = model.operands(q)
    C, Sn, M = eta.shape
    rep = DS.host_draws(kind, tot, eta, seed, np.arange(C)[:, None, None] + chain0,
                        np.arange(Sn)[None, :, None] + iter0, np.arange(M)[None, None, :])
    return rep, y


@functools.lru_cache(maxsize=None)
def _replicated(name):
    d = DS.data()
    if name == "binomial":
        d.nt = d.nt.copy()
        d.nt[5] = F32(2.0 ** 23)           # a total beyond the exact range: NaN, counted
        d.ybin = d.ybin.copy()
        d.ybin[5] = 3.0
    model = DS.likelihood(name, d)
    q = DS.draws(model)
    if name == "poisson":
        q[1, 4, 0] = 20.0                   # exp(a + b x) >= 2^23 at that draw: NaN
    if name == "bernoulli":
        q[2, 7, 0] = np.nan
    got = _pp(model, q, seed=77, replicates=True)
    rep, y = _host_rep(model, q, 77)
    return model, q, got, rep, y


@pytest.mark.parametrize("name", NODES)
def test_replicates_equal_the_host_definition(gpu, name):
    model, q, got, rep, y = _replicated(name)
    dev = got["replicates"].cpu().numpy()
    assert dev.shape == rep.shape == (3, 37, DS.N_OBS) and dev.dtype == F32
    assert np.array_equal(np.isnan(dev), np.isnan(rep))
    assert np.nan_to_num(dev, nan=-1.0).tobytes() == np.nan_to_num(rep, nan=-1.0).tobytes()
    bad = np.isnan(rep)
    if name == "binomial":
        assert bad[:, :, 5].all() and not np.delete(bad, 5, axis=2).any()
    elif name == "poisson":
        assert bad[1, 4].all() and bad.sum() == DS.N_OBS
    else:
        assert bad[2, 7].all() and bad.sum() == DS.N_OBS
    fin = dev[~bad]
    assert np.all(fin == np.floor(fin)) and np.all(fin >= 0)
    ref = DS.stats_of(rep, y)
    assert got["nonfinite"].sum() == bad.sum() > 0
    for f in STAT:
        np.testing.assert_allclose(got[f], ref[f], rtol=1e-12, atol=0, err_msg=f)
    nfin = ref["n"] - ref["nonfinite"]
    with np.errstate(all="ignore"):
        np.testing.assert_allclose(got["pit"], ref["below"] / nfin, rtol=1e-12)
        np.testing.assert_allclose(got["pit_mid"], (ref["below"] + 0.5 * ref["equal"]) / nfin,
                                   rtol=1e-12)
    assert got["equal"].sum() > 0


def test_replicate_shards_and_thinning_reproduce_the_whole(gpu):
    model, q, got, rep, y = _replicated("poisson")
    whole = got["replicates"].cpu().numpy()
    nz = lambda a: np.nan_to_num(a, nan=-1.0).tobytes()   # noqa: E731
    # shards of chains
    a = _pp(model, q[:1], seed=77, replicates=True)
    b = _pp(model, q[1:], seed=77, replicates=True, chain_offset=1)
    assert nz(np.concatenate([a["replicates"].cpu().numpy(), b["replicates"].cpu().numpy()])) \
        == nz(whole)
    m = _D().merge_predictive([a, b])
    for f in STAT:
        np.testing.assert_allclose(m[f], got[f], rtol=1e-12, atol=0, err_msg=f)
    # shards of iterations
    a = _pp(model, q[:, :20], seed=77, replicates=True)
    b = _pp(model, q[:, 20:], seed=77, replicates=True, iter_offset=20)
    both = np.concatenate([a["replicates"].cpu().numpy(), b["replicates"].cpu().numpy()], axis=1)
    assert nz(both) == nz(whole)
    m = _D().merge_predictive([a, b])
    for f in STAT:
        np.testing.assert_allclose(m[f], got[f], rtol=1e-12, atol=0, err_msg=f)
    # thin = 3: iterations 0, 3, 6, ...
    t = _pp(model, q, seed=77, replicates=True, thin=3)
    assert nz(t["replicates"].cpu().numpy()) == nz(whole[:, ::3])
    ref = DS.stats_of(rep[:, ::3], y[:, ::3])
    for f in STAT:
        np.testing.assert_allclose(t[f], ref[f], rtol=1e-12, atol=0, err_msg=f)
    # without the replicates: the same statistics
    s = _pp(model, q, seed=77)
    for f in STAT:
        np.testing.assert_array_equal(s[f], got[f], err_msg=f)


def test_mixed_normal_and_poisson_terms(gpu):
    import _predictive as PP
    import mlx_mcmc_amd as m
    import mlx_mcmc_amd.core as mx

    d = DS.data()
    z = np.random.default_rng(5).standard_normal(13).astype(F32)

    def lik(p):
        return (mx.sum(m.Normal(p["a"], 1.5).log_prob(z))
                + mx.sum(m.Poisson(log_rate=p["a"] + p["b"] * d.x).log_prob(d.yp)))
    model = DS.likelihood("poisson", d)
    q = DS.draws(model)
    got = _D().posterior_predictive(lik, q, DS.layout_of(model), seed=9, replicates=True,
                                    group=False)
    dev = got["replicates"].cpu().numpy()
    assert dev.shape == (3, 37, 13 + DS.N_OBS)
    C, Sn = 3, 37
    ch, it = np.arange(C)[:, None, None], np.arange(Sn)[None, :, None]
    want_n = PP.host_draws(PP.NORMAL, np.broadcast_to(q[..., 0:1], (C, Sn, 13)), 1.5, 9, ch, it,
                           np.arange(13)[None, None, :])
    kind, tot, eta, y = model.operands(q)
    want_p = DS.host_draws(kind, tot, eta, 9, ch, it, 13 + np.arange(DS.N_OBS)[None, None, :])
    assert dev[..., :13].tobytes() == np.ascontiguousarray(want_n).tobytes()
    assert np.ascontiguousarray(dev[..., 13:]).tobytes() == want_p.tobytes()
    ref = DS.stats_of(np.concatenate([want_n, want_p], 2),
                      np.concatenate([np.broadcast_to(z, (C, Sn, 13)), y], 2))
    for f in STAT:
        np.testing.assert_allclose(got[f], ref[f], rtol=1e-12, atol=0, err_msg=f)


def test_ties_are_for_programs_with_a_count_term(gpu):
    """A fused-only likelihood: no ``equal`` from the facade, its former
    workspace size (five fields per block), and MC_ERR_UNSUPPORTED from
    mc_predictive_eq when the caller asks for the ties."""
    import torch

    import _predictive as PP
    from mlx_mcmc_amd import _lib, _trace

    model = PP.normal_gather(C=8, S=400)
    lay = PP.layout_of(model)
    got = _D().posterior_predictive(model.log_likelihood, model.draws, lay, seed=3, group=False)
    assert "equal" not in got and "pit_mid" not in got
    prog = _trace.pointwise_program(model.log_likelihood, lay)
    lib = _lib.load()
    assert lib.mc_program_num_count_terms(prog.handle) == 0
    C, Sn, _ = model.draws.shape
    nb = lib.mc_predictive_workspace_bytes(prog.handle, C, Sn, 1)
    assert nb > 0 and nb % (_lib.MC_PP_COUNT * model.M * 8) == 0      # B blocks of five fields
    x = torch.tensor(model.draws, device=gpu)
    st = torch.empty((_lib.MC_PP_COUNT, model.M), dtype=torch.float64, device=gpu)
    eq = torch.empty(model.M, dtype=torch.float64, device=gpu)
    ws = torch.empty(int(nb), dtype=torch.uint8, device=gpu)
    rc = lib.mc_predictive_eq(prog.handle, C, Sn, 1, 3, 0, 0, _lib.ptr(x), _lib.ptr(st),
                              _lib.ptr(eq), None, _lib.ptr(ws), nb, _lib.stream_handle())
    assert rc == _lib.MC_ERR_UNSUPPORTED and b"count term" in lib.mc_last_error()
    # a count likelihood: one more f64 per block and observation
    cm = DS.likelihood("poisson")
    cp = _trace.pointwise_program(cm.log_likelihood, DS.layout_of(cm))
    assert lib.mc_program_num_count_terms(cp.handle) == 1
    nb = lib.mc_predictive_workspace_bytes(cp.handle, 8, 400, 1)
    assert nb > 0 and nb % ((_lib.MC_PP_COUNT + 1) * cm.M * 8) == 0


def test_concrete_log_prob_on_the_device(gpu):
    """log_prob on concrete values (mc_discrete_log_prob): the node's bits as
    the tape forms them, plus the normaliser; probs = / rate = outside their
    domain give -inf."""
    import mlx_mcmc_amd as m
    from scipy import stats as sps

    y = np.array([0, 1, 4, 7, 9, -1, 2.5], F32)
    got = m.Poisson(log_rate=F32(0.7)).log_prob(y)
    assert got.dtype == F32 and np.all(got[5:] == -np.inf)
    np.testing.assert_allclose(got[:5], sps.poisson(np.exp(np.float64(F32(0.7)))).logpmf(y[:5]),
                               rtol=2e-6, atol=2e-5)
    n = np.full(7, 9.0, F32)
    got = m.Binomial(n, probs=F32(0.3)).log_prob(y)
    np.testing.assert_allclose(got[:5], sps.binom(9, np.float64(F32(0.3))).logpmf(y[:5]),
                               rtol=2e-6, atol=2e-5)
    assert np.all(got[5:] == -np.inf)
    assert np.all(m.Binomial(n, probs=F32(1.0)).log_prob(y) == -np.inf)
    got = m.Bernoulli(logits=np.array([-90.0, 0.0, 90.0], F32)).log_prob(F32(1.0))
    np.testing.assert_array_equal(got, DS.fwd32("bernoulli", 1.0, None, [-90.0, 0.0, 90.0]))
    assert np.all(m.Poisson(rate=F32(-1.0)).log_prob(y) == -np.inf)
