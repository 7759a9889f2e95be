"""The Student-t family on the device: MC_EX_STUDENT_T_LP and
MC_EX_HALF_STUDENT_T_LP on every interpreter form against the float64 table of
tests/_student_t.py (ulp gates derived there), the compiled evaluators against
the interpreter, the two N = 67 models against the oracle (tape, sampler
decisions), an exact one-parameter posterior, the kernel route at N = 100 K,
WAIC / PSIS-LOO on the regression likelihood, posterior predictive replicates
against the host definition, and concrete log_prob against scipy.stats."""
import functools
import math

import numpy as np
import pytest

import _expr_ops as X
import _pointwise as PW
import _psis as PS
import _student_t as ST
from _near_tie import compare_trace, log_u
from oracle import samplers as S

pytestmark = pytest.mark.gpu
F32 = np.float32
CASES = [(name, nu) for name in ST.NODES for nu in ST.NUS]


# ---- the nodes on the interpreter forms ------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bulk(name, nu):
    v, m, s = ST.bulk(name, nu)
    return {"args": (v, m, s), "VF": ST.run_V(name, nu, v, m, s, "VF"),
            "V": ST.run_V(name, nu, v, m, s), "V32": ST.run_V(name, nu, v, m, s, "V32")}


@functools.lru_cache(maxsize=None)
def _edge(name, nu):
    v, m, s = ST.edges(name)
    out = {"args": (v, m, s), "VF": ST.run_V(name, nu, v, m, s, "VF"),
           "V": ST.run_V(name, nu, v, m, s), "V32": ST.run_V(name, nu, v, m, s, "V32")}
    out["S"] = ST.run_S(name, nu, v, m, s)
    return out


@pytest.mark.parametrize("name,nu", CASES)
def test_node_value_and_vjp_bulk(gpu, name, nu):
    d = _bulk(name, nu)
    args = d["args"]
    uf, ug = ST.units(name, nu, *args)
    ef = np.abs(d["VF"].astype(np.float64) - ST.fwd64(name, nu, *args)) / uf
    print(f"{name} nu = {nu}: max error value {ef.max():.3f} (gate {ST.FWD_GATE}) over "
          f"{ef.size} points")
    ref = ST.vjp64(name, nu, *args)
    worst = {}
    for k in ST.diff_names(name):
        eg = np.abs(d["V"][k].astype(np.float64) - ref[k]) / ug[k]
        worst[k] = eg.max()
        print(f"    VJP {k}: {eg.max():.3f} (gate {ST.VJP_GATE[k]})")
    assert ef.max() <= ST.FWD_GATE
    for k, e in worst.items():
        assert e <= ST.VJP_GATE[k], k
    # NMAX = 16 and NMAX = 32 agree bit for bit
    for k in ST.diff_names(name):
        assert X.same_bits(d["V"][k], d["V32"][k]).all(), k


@pytest.mark.parametrize("name,nu", CASES)
def test_node_edges(gpu, name, nu):
    d = _edge(name, nu)
    args = d["args"]
    uf, ug = ST.units(name, nu, *args)
    skip = np.zeros(args[0].shape, bool)
    bad = X.edge_failures(d["VF"], ST.fwd64(name, nu, *args), ST.fwd32(name, nu, *args), skip,
                          ST.FWD_GATE, unit=uf)
    assert bad.size == 0, [(tuple(float(a[i]) for a in args), float(d["VF"][i])) for i in bad[:8]]
    r64, r32 = ST.vjp64(name, nu, *args), ST.vjp32(name, nu, *args)
    for k in ST.diff_names(name):
        bad = X.edge_failures(d["V"][k], r64[k], r32[k], skip, ST.VJP_GATE[k], unit=ug[k])
        assert bad.size == 0, (k, [(tuple(float(a[i]) for a in args), float(d["V"][k][i]))
                                   for i in bad[:8]])
    # the classes the header names: q = inf gives -inf and zero cotangents; the
    # half form below its support (and at a NaN v) -inf and zero cotangents
    v, m, s = args
    with np.errstate(all="ignore"):
        z = (v - (0 if ST.is_half(name) else m)) / s
        far = np.isinf(z * z) & (s > 0) & np.isfinite(s)
    if ST.is_half(name):
        far &= v >= 0
        out = ~(v >= 0)
        assert out.any() and np.all(d["VF"][out] == -np.inf)
        assert all(np.all(d["V"][k][out] == 0) for k in ST.diff_names(name))
    assert far.sum() >= 2 and np.all(d["VF"][far] == -np.inf)
    assert all(np.all(d["V"][k][far] == 0) for k in ST.diff_names(name))
    # every form gives the same bits
    lp, g = d["S"]
    assert X.same_bits(lp, d["VF"]).all()
    for k in ST.diff_names(name):
        assert X.same_bits(d["V"][k], d["V32"][k]).all(), k
        assert X.same_bits(g[k], d["V"][k]).all(), k


# ---- compiled evaluators -----------------------------------------------------------------
def _sample(algo, model, jit):
    import mlx_mcmc_amd as m
    from mlx_mcmc_amd import _lib, _trace

    lib = _lib.load()
    lib.mc_debug_expr_jit(1 if jit else 0)
    try:
        lp, init = ST.MODELS[model](False)
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


@pytest.mark.parametrize("model", list(ST.MODELS))
@pytest.mark.parametrize("algo", ["hmc", "nuts", "mh"])
def test_tape_jit_bit_identical_to_interpreter(gpu, algo, model):
    s0, i0, st0 = _sample(algo, model, False)
    s1, i1, st1 = _sample(algo, model, True)
    assert st0 == 0 and st1 == 1, (st0, st1)
    for k in s0:
        np.testing.assert_array_equal(np.asarray(s0[k]), np.asarray(s1[k]), err_msg=k)
    for k, v in i0.trace.items():
        np.testing.assert_array_equal(v, i1.trace[k], err_msg=k)


N_LANE = 250


def _lane_model(oracle, broadcast=True):
    """theta[250] under Normal(0, 1) (and a broadcast intercept), nine terms of
    250 data elements each (the lane planner takes expression programs from
    2048 elements on): 0.1 sum_i lp(y_ki; a + theta_i x_ki, s_k), StudentT(4)
    and HalfStudentT(3) of |y| alternating — both pair cases of ex2_fwd /
    ex2_bwd, the half form with theta in its scale exp(0.1 theta_i x_ki)."""
    rng = np.random.default_rng(63)
    xs = rng.uniform(0.5, 2.0, (9, N_LANE)).astype(F32) * rng.choice([-1.0, 1.0], (9, N_LANE)).astype(F32)
    ys = rng.standard_t(4, (9, N_LANE)).astype(F32)
    init = {"theta": np.zeros(N_LANE, F32)}
    if broadcast:
        init["a"] = F32(0.0)
    c4, c3 = ST.norm64(4.0, False), ST.norm64(3.0, True)
    if oracle:
        import torch
        from torch import distributions as TD
        t = lambda v: torch.tensor(np.asarray(v, np.float64))   # noqa: E731

        def log_prob(p):
            th = p["theta"].to(torch.float64)
            a = p["a"].to(torch.float64) if broadcast else 0.0
            lp = TD.Normal(0.0, 1.0).log_prob(th).sum()
            if broadcast:
                lp = lp + TD.Normal(0.0, 1.0).log_prob(a)
            for k in range(9):
                if k % 2 == 0:
                    term = TD.StudentT(4.0, a + th * t(xs[k]), 1.5).log_prob(t(ys[k]))
                else:
                    sc = torch.exp(0.1 * (th * t(xs[k])))
                    term = math.log(2.0) + TD.StudentT(3.0, 0.0, sc).log_prob(t(np.abs(ys[k])))
                lp = lp + float(F32(0.1)) * term.sum()
            return lp
        return log_prob, init

    def log_prob(p):
        import mlx_mcmc_amd as m
        import mlx_mcmc_amd.core as mx
        lp = mx.sum(m.Normal(0, 1).log_prob(p["theta"]))
        if broadcast:
            lp = lp + m.Normal(0, 1).log_prob(p["a"])
        for k in range(9):
            if k % 2 == 0:
                loc = p["a"] + p["theta"] * xs[k] if broadcast else p["theta"] * xs[k]
                term = m.StudentT(4.0, loc, 1.5).log_prob(ys[k])
            else:
                term = m.HalfStudentT(3.0, mx.exp(0.1 * (p["theta"] * xs[k]))).log_prob(np.abs(ys[k]))
            lp = lp + 0.1 * mx.sum(term)
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
    """The lane kernel's pair code (ex2_fwd / ex2_bwd's Student-t cases) against
    the interpreter tape over two leapfrog steps from 16 starts, at the bar of
    tests/test_gpu_discrete.py test_lane_jit_two_leapfrogs: the same decisions,
    theta bit for bit, and the float64 restatement's position."""
    from oracle import philox as R

    eps, seed, C = 0.05, 20, 16
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


def test_student_t_on_sliced_nuts_and_mh(gpu, monkeypatch):
    """One NUTS run on k_nuts_sl and one MH run on k_mh_sl of a Student-t
    regression per parameter, against the interpreter tape
    (test_poisson_on_sliced_nuts_and_mh's bars): trees identical for >= 6
    iterations per chain, MH decisions identical over 40 iterations."""
    import mlx_mcmc_amd as m
    from mlx_mcmc_amd import _lib

    lib = _lib.load()
    lp, init = _lane_model(False, broadcast=False)
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


# ---- the two models against the oracle -----------------------------------------------------
def _points(prog, init, k=6, spread=0.3, seed=7):
    rng = np.random.default_rng(seed)
    base = prog.layout.flatten(init)
    return np.stack([base + rng.normal(0, spread, base.size).astype(F32) for _ in range(k)])


@pytest.mark.parametrize("model", list(ST.MODELS))
def test_tape_matches_autograd(gpu, model):
    """tests/test_gpu_discrete.py test_tape_matches_autograd's bars."""
    from mlx_mcmc_amd import _engine, _lib, _trace

    lp_fn, init = ST.MODELS[model](False)
    prog = _trace.compile_model(lp_fn, init)
    ops = [prog.model.c_nodes[i].op for i in range(prog.model.n_nodes)]
    assert ST.OP["student_t"] in ops
    assert (ST.OP["half_student_t"] in ops) == (model == "hierarchy")
    olp, oinit = ST.MODELS[model](True)
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


# (starts near the posterior; step sizes at which the float64 restatement's
# log ratios stay above -0.5 over the compared iterations, checked with
# oracle.samplers on the CPU: at 0.12 / 0.25 its warmup meets trajectories with
# energy errors of 4 and 23, which amplify the f32 rounding of any evaluator to
# 1.1 of the near-tie bound — iteration 20 and iteration 1 on an MI355X)
START = {"regression": ({"a": 0.4, "b": 0.9, "log_s": -0.2}, 0.03),
         "hierarchy": ({"mu": 0.3, "log_tau": -0.3, "theta": np.full(8, 0.3, F32)}, 0.05)}


def _start(model):
    return {k: (np.asarray(v, F32) if np.ndim(v) else F32(v)) for k, v in START[model][0].items()}


@pytest.mark.parametrize("model", list(ST.MODELS))
def test_hmc_trace_matches_oracle(gpu, model):
    import mlx_mcmc_amd as m

    lp, _ = ST.MODELS[model](False)
    olp, _ = ST.MODELS[model](True)
    start, eps = _start(model), START[model][1]
    seed, n = 3, 40
    kw = dict(num_samples=40, num_warmup=40, step_size=eps, num_leapfrog_steps=10)
    _, _, info = m.hmc(lp, start, key=m.random.key(seed), progress=False, return_info=True,
                       return_trace=True, **kw)
    ref = S.hmc(olp, start, seed=seed, **kw)
    tr = info.trace
    gpu_c = {"accepted": tr["accepted"][0][:n], "ratio": tr["accept_stat"][0][:n],
             "step_size": tr["step_size"][0][:n], "energy": tr["energy"][0][:n]}
    ref_c = {k: np.asarray(ref.trace[k])[:n] for k in ("accepted", "ratio", "step_size", "energy")}
    ref_c["log_u"] = log_u(seed, 0, n)
    same = compare_trace(gpu_c, ref_c, f"{model} seed {seed}", verbose=True)
    assert same >= 30 and np.asarray(ref.trace["accepted"][:same]).any()


@pytest.mark.parametrize("model", list(ST.MODELS))
def test_nuts_trees_match_oracle(gpu, model):
    import mlx_mcmc_amd as m

    lp, _ = ST.MODELS[model](False)
    olp, _ = ST.MODELS[model](True)
    start = _start(model)
    n_w, n_s = 30, 10
    _, _, info = m.nuts(lp, start, num_samples=n_s, num_warmup=n_w, step_size=0.02,
                        key=m.random.key(2), progress=False, return_info=True, return_trace=True)
    ref = S.nuts(olp, start, num_samples=n_s, num_warmup=n_w, step_size=0.02, seed=2)
    same = 0
    for i in range(n_w + n_s):
        if (info.trace["tree_depth"][0][i] != ref.trace["depth"][i]
                or info.trace["n_leapfrog"][0][i] != ref.trace["leaves"][i]):
            break
        same += 1
    assert same >= 10, f"trees diverged at iteration {same}"
    assert max(ref.trace["depth"][:same]) >= 2


@pytest.mark.parametrize("model", list(ST.MODELS))
def test_mh_decisions_match_oracle(gpu, model):
    import mlx_mcmc_amd as m
    from _near_tie import tie_bound

    lp, _ = ST.MODELS[model](False)
    olp, _ = ST.MODELS[model](True)
    start = _start(model)
    n, seed = 150, 5
    s, _, info = m.metropolis_hastings(lp, start, num_samples=n, proposal_scale=0.15,
                                       random_seed=seed, return_info=True, return_trace=True)
    ref = S.metropolis_hastings(olp, start, num_samples=n, proposal_scale=0.15, random_seed=seed)
    acc, racc = info.trace["accepted"][0].astype(bool), np.array(ref.trace["accepted"])
    assert 0 < racc.mean() < 1
    lu = log_u(m.random.key(seed).seed, 0, n)
    same = n
    for i in range(n):
        if acc[i] != racc[i]:
            # a flip only at a proven near-tie
            assert abs(float(lu[i]) - ref.trace["ratio"][i]) <= tie_bound(ref.trace["logp"][i]), i
            same = i
            break
    assert same >= 100, f"compared only {same} of {n} decisions"


def test_exact_posterior_of_the_location_model(gpu):
    """y_i ~ StudentT(4, mu, 1), mu ~ Normal(0, 10), N = 67: the posterior mean
    within 4 MCSE of the float64 quadrature value and the sd within 10 %
    (test_conjugate_posterior_mean's gates), 32 chains x 500 draws at a fixed
    step size, ten steps of it about 1.5 posterior sd.  oracle.samplers.hmc at
    the same settings meets the bar on the CPU with 8 chains."""
    import mlx_mcmc_amd as m

    lp, init, mean, sd = ST.location(False)
    eps = ST.location_step(sd)
    s, _, info = m.hmc(lp, init, num_samples=500, num_warmup=100, step_size=eps,
                       num_leapfrog_steps=10, adapt_step_size=False, key=m.random.key(1),
                       num_chains=32, progress=False, return_info=True)
    d = np.asarray(s["mu"])
    assert d.shape == (32, 500) and np.all(info.accept_rate > 0.3)
    mcse = d.mean(1).std() / np.sqrt(d.shape[0])
    print(f"mean {d.mean():.5f} exact {mean:.5f} (MCSE {mcse:.5f}), sd {d.std():.4f} exact "
          f"{sd:.4f}, step {eps}")
    assert abs(d.mean() - mean) < 4 * mcse
    assert abs(d.std() - sd) < 0.1 * sd


def test_class_form_takes_the_hand_written_route(gpu):
    """N = 100 K, 64 chains, the default plan: StudentT(4, a + b x, s) runs on
    the kernel route of the hand-written elementary-node form, and that route
    is not the chain-per-workgroup one."""
    import mlx_mcmc_amd as m
    import mlx_mcmc_amd.core as mx
    from mlx_mcmc_amd import _trace

    n = 100_000
    rng = np.random.default_rng(0)
    x = rng.normal(0, 1, n).astype(F32)
    y = (0.5 + 0.8 * x + 0.7 * rng.standard_t(4, n)).astype(F32)
    c = float(F32(ST.norm64(4.0, False)))

    def prior(p):
        return (m.Normal(0, 5).log_prob(p["a"]) + m.Normal(0, 5).log_prob(p["b"])
                + m.Normal(0, 1).log_prob(p["log_s"]))

    def hand(p):
        s = mx.exp(p["log_s"])
        z = (y - (p["a"] + p["b"] * x)) / s
        return prior(p) + mx.sum(-2.5 * mx.log1p(z * z / 4.0) - mx.log(s) + c)

    def node(p):
        return prior(p) + mx.sum(m.StudentT(4, p["a"] + p["b"] * x,
                                            mx.exp(p["log_s"])).log_prob(y))
    init = {"a": F32(0.4), "b": F32(0.7), "log_s": F32(-0.3)}
    routes = []
    for lp in (hand, node):
        prog = _trace.compile_model(lp, init)
        _, _, info = m.hmc(lp, init, num_samples=2, num_warmup=2, step_size=1e-3,
                           num_leapfrog_steps=3, key=m.random.key(1), num_chains=64,
                           progress=False, return_info=True)
        routes.append((info.extra["kernel"], prog.slice_kernel, prog.num_slices))
    print("routes (hand-written, StudentT):", routes)
    assert routes[0] == routes[1] and routes[0][0] != "unsliced", routes


# ---- WAIC and PSIS-LOO -------------------------------------------------------------------------
def _D():
    from mlx_mcmc_amd import diagnostics
    return diagnostics


def test_waic_and_loo(gpu):
    """C = 3, S = 37 as tests/_pointwise.py: the matrix and statistics at its
    bars, WAIC from them; PSIS-LOO at tests/test_gpu_psis.py's bars."""
    model = ST.likelihood("regression")
    q = ST.draws(model)
    lay = ST.layout_of(model)
    got = _D().pointwise_log_likelihood(model.log_likelihood, q, lay, matrix=True, group=False)
    ref = model.ll(q, np.float64)
    mat = got["matrix"].cpu().numpy()
    assert mat.shape == (3, 37, ST.N_OBS)
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
    own = PS.psis_matrix(mat.reshape(-1, ST.N_OBS))
    r64 = PS.psis_matrix(ref.reshape(-1, ST.N_OBS))
    assert loo["tail_len"] == own["tail_len"] == 23
    pw = loo["pointwise"]
    np.testing.assert_array_equal(loo["tail_n"], own["n"])
    for f, g in (("khat", pw["khat"]), ("elpd", pw["elpd_loo"])):
        np.testing.assert_allclose(g, own[f], rtol=1e-10, atol=0, err_msg=f)
    np.testing.assert_allclose(pw["elpd_loo"], r64["elpd"], rtol=PS.RTOL, atol=PS.ATOL)
    np.testing.assert_allclose(pw["khat"], r64["khat"], rtol=PS.RTOL, atol=PS.ATOL)
    assert loo["n_nonfinite"] == 0


# ---- posterior predictive replicates -------------------------------------------------------------
STAT = ("n", "mean", "m2", "below", "nonfinite")


def _pp(model, q, **kw):
    return _D().posterior_predictive(model.log_likelihood, q, ST.layout_of(model), group=False,
                                     **kw)


def _host_rep(model, q, seed, chain0=0, iter0=0, obs0=0):
    loc, s, y = model.operands(q)
    C, Sn, M = loc.shape
    rep = ST.host_draws(model.nu, loc, s, model.half, seed, np.arange(C)[:, None, None] + chain0,
                        np.arange(Sn)[None, :, None] + iter0, obs0 + np.arange(M)[None, None, :])
    return rep, y


@functools.lru_cache(maxsize=None)
def _replicated(name):
    model = ST.likelihood(name)
    q = ST.draws(model)
    q[1, 4, -1] = np.nan                    # a NaN scale at that draw: NaN, counted
    got = _pp(model, q, seed=77, replicates=True)
    rep, y = _host_rep(model, q, 77)
    return model, q, got, rep, y


@pytest.mark.parametrize("name", ["regression", "half", "cauchy"])
def test_replicates_equal_the_host_definition(gpu, name):
    import _predictive as PP

    model, q, got, rep, y = _replicated(name)
    dev = got["replicates"].cpu().numpy()
    assert dev.shape == rep.shape == (3, 37, ST.N_OBS) and dev.dtype == F32
    assert np.array_equal(np.isnan(dev), np.isnan(rep))
    assert np.nan_to_num(dev, nan=-1.0).tobytes() == np.nan_to_num(rep, nan=-1.0).tobytes()
    bad = np.isnan(rep)
    assert bad[1, 4].all() and bad.sum() == ST.N_OBS
    if model.half:
        assert np.all(dev[~bad] >= 0)
    else:
        assert (dev[~bad] < 0).any()
    ref = PP.stats_of(rep, y)
    assert got["nonfinite"].sum() == bad.sum() > 0
    for f in STAT:
        np.testing.assert_allclose(got[f], ref[f], rtol=1e-12, atol=0, err_msg=f)
    nfin = ref["n"] - ref["nonfinite"]
    np.testing.assert_allclose(got["pit"], ref["below"] / nfin, rtol=1e-12)
    assert "equal" not in got and "pit_mid" not in got


def test_replicate_shards_and_thinning_reproduce_the_whole(gpu):
    import _predictive as PP

    model, q, got, rep, y = _replicated("regression")
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
    ref = PP.stats_of(rep[:, ::3], y[:, ::3])
    for f in STAT:
        np.testing.assert_allclose(t[f], ref[f], rtol=1e-12, atol=0, err_msg=f)
    # without the replicates: the same statistics
    s = _pp(model, q, seed=77)
    for f in STAT:
        np.testing.assert_array_equal(s[f], got[f], err_msg=f)


def test_mixed_normal_and_student_t_terms(gpu):
    import _predictive as PP
    import mlx_mcmc_amd as m
    import mlx_mcmc_amd.core as mx

    d = ST.data()
    z = np.random.default_rng(5).standard_normal(13).astype(F32)

    def lik(p):
        return (mx.sum(m.Normal(p["a"], 1.5).log_prob(z))
                + mx.sum(m.StudentT(4, p["a"] + p["b"] * d.x, p["s"]).log_prob(d.y)))
    model = ST.likelihood("regression", d)
    q = ST.draws(model)
    got = _D().posterior_predictive(lik, q, ST.layout_of(model), seed=9, replicates=True,
                                    group=False)
    dev = got["replicates"].cpu().numpy()
    C, Sn = 3, 37
    assert dev.shape == (C, Sn, 13 + ST.N_OBS)
    ch, it = np.arange(C)[:, None, None], np.arange(Sn)[None, :, None]
    want_n = PP.host_draws(PP.NORMAL, np.broadcast_to(q[..., 0:1], (C, Sn, 13)), 1.5, 9, ch, it,
                           np.arange(13)[None, None, :])
    want_t, y = _host_rep(model, q, 9, obs0=13)
    assert dev[..., :13].tobytes() == np.ascontiguousarray(want_n).tobytes()
    assert np.ascontiguousarray(dev[..., 13:]).tobytes() == want_t.tobytes()
    ref = PP.stats_of(np.concatenate([want_n, want_t], 2),
                      np.concatenate([np.broadcast_to(z, (C, Sn, 13)), y], 2))
    for f in STAT:
        np.testing.assert_allclose(got[f], ref[f], rtol=1e-12, atol=0, err_msg=f)
    assert "equal" not in got


def test_ties_stay_with_the_count_terms(gpu):
    """A Student-t-only program: no ``equal`` / ``pit_mid``, no count term, a
    workspace of five fields per block, and MC_ERR_UNSUPPORTED from
    mc_predictive_eq.  Beside a Poisson term the ties are back."""
    import torch

    import _discrete as DS
    import mlx_mcmc_amd as m
    import mlx_mcmc_amd.core as mx
    from mlx_mcmc_amd import _lib, _trace

    model = ST.likelihood("regression")
    lay = ST.layout_of(model)
    lib = _lib.load()
    prog = _trace.pointwise_program(model.log_likelihood, lay)
    assert lib.mc_program_num_count_terms(prog.handle) == 0
    C, Sn = 8, 400
    nb = lib.mc_predictive_workspace_bytes(prog.handle, C, Sn, 1)
    assert nb > 0 and nb % (_lib.MC_PP_COUNT * model.M * 8) == 0
    q = ST.draws(model, C=C, S=Sn)
    got = _pp(model, q, seed=3)
    assert "equal" not in got and "pit_mid" not in got and got["n"][0] == C * Sn
    x = torch.tensor(q, device=gpu)
    st = torch.empty((_lib.MC_PP_COUNT, model.M), dtype=torch.float64, device=gpu)
    eq = torch.empty(model.M, dtype=torch.float64, device=gpu)
    ws = torch.empty(int(nb), dtype=torch.uint8, device=gpu)
    rc = lib.mc_predictive_eq(prog.handle, C, Sn, 1, 3, 0, 0, _lib.ptr(x), _lib.ptr(st),
                              _lib.ptr(eq), None, _lib.ptr(ws), nb, _lib.stream_handle())
    assert rc == _lib.MC_ERR_UNSUPPORTED and b"count term" in lib.mc_last_error()
    # Student-t + Poisson: the ties of every term are counted
    d, dd = ST.data(), DS.data()

    def lik(p):
        return (mx.sum(m.StudentT(4, p["a"] + p["b"] * d.x, p["s"]).log_prob(d.y))
                + mx.sum(m.Poisson(log_rate=p["a"] + p["b"] * dd.x).log_prob(dd.yp)))
    q = ST.draws(model)
    got = _D().posterior_predictive(lik, q, lay, seed=3, group=False)
    assert got["equal"].shape == (2 * ST.N_OBS,) and "pit_mid" in got
    assert got["equal"][:ST.N_OBS].sum() == 0 and got["equal"][ST.N_OBS:].sum() > 0
    mixed = _trace.pointwise_program(lik, lay)
    assert lib.mc_program_num_count_terms(mixed.handle) == 1


# ---- concrete log_prob ---------------------------------------------------------------------------
def test_concrete_log_prob_on_the_device(gpu):
    """log_prob on concrete values (mc_student_t_log_prob) against scipy.stats
    at the count classes' tolerances; -inf below the half forms' support; the
    node's own bits for one case."""
    import mlx_mcmc_amd as m
    from scipy import stats as sps

    x = np.array([-30.0, -2.5, -0.1, 0.0, 0.7, 3.0, 250.0], F32)
    x64 = x.astype(np.float64)
    got = m.StudentT(4, F32(0.3), F32(1.7)).log_prob(x)
    assert got.dtype == F32 and got.shape == x.shape
    np.testing.assert_allclose(got, sps.t(4, loc=np.float64(F32(0.3)),
                                          scale=np.float64(F32(1.7))).logpdf(x64),
                               rtol=2e-6, atol=2e-5)
    got = m.Cauchy(F32(0.3), F32(1.7)).log_prob(x)
    np.testing.assert_allclose(got, sps.cauchy(np.float64(F32(0.3)),
                                               np.float64(F32(1.7))).logpdf(x64),
                               rtol=2e-6, atol=2e-5)
    loc = np.linspace(-1, 1, 7).astype(F32)
    got = m.StudentT(2.5, loc, F32(0.8)).log_prob(F32(0.4))
    np.testing.assert_allclose(got, sps.t(2.5, loc=loc.astype(np.float64),
                                          scale=np.float64(F32(0.8))).logpdf(0.4),
                               rtol=2e-6, atol=2e-5)
    got = m.HalfCauchy(F32(5.0)).log_prob(x)
    assert np.all(got[:3] == -np.inf)
    np.testing.assert_allclose(got[3:], sps.halfcauchy(scale=5.0).logpdf(x64[3:]),
                               rtol=2e-6, atol=2e-5)
    got = m.HalfStudentT(3, F32(2.0)).log_prob(x)
    assert np.all(got[:3] == -np.inf)
    np.testing.assert_allclose(got[3:], math.log(2.0) + sps.t(3, scale=2.0).logpdf(x64[3:]),
                               rtol=2e-6, atol=2e-5)
    assert m.HalfCauchy(1.0).log_prob(F32(np.nan)) == -np.inf
    # the node's own bits (normaliser taken off again in f32: exact for these)
    core = m.StudentT(4, F32(0.3), F32(1.7)).log_prob(x)
    want = (ST.fwd32("student_t", 4.0, x, 0.3, 1.7)
            + F32(ST.norm64(4.0, False))).astype(F32)
    assert np.all(np.abs(core.astype(np.float64) - want) <= ST.FWD_GATE * X.ulp(want))
    lib_bits = m.HalfStudentT(1, F32(1.0)).log_prob(F32(0.0))
    assert lib_bits == F32(ST.norm64(1.0, True))          # -log 1 - 1 * log1p(0) = 0 exactly
