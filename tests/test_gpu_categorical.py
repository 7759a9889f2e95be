"""Categorical on the device: MC_EX_LOGADDEXP and MC_EX_PICK on every
interpreter form against the float64 table of tests/_categorical.py (ulp gates
derived there), the compiled evaluators against the interpreter, the N = 67
models against the oracle (tape, sampler decisions), K = 2 against Bernoulli,
the example-05 probs= model, an exact posterior by quadrature, the kernel
route at N = 100 K, WAIC / PSIS-LOO on the Categorical likelihood, and the
sampling rule of ``Categorical.sample``.

Posterior predictive replicates of a Categorical term are not built: the term
keeps the "has no sampling distribution" error (pinned below)."""
import functools

import numpy as np
import pytest

import _categorical as CT
import _discrete as DS
import _expr_ops as X
import _pointwise as PW
import _psis as PS
from _near_tie import compare_trace, log_u, tie_bound
from oracle import samplers as S

pytestmark = pytest.mark.gpu
F32 = np.float32
U1 = float(np.spacing(F32(1.0)))       # the forms' cotangent is 1


# ---- the nodes on the interpreter forms ------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lae():
    A, B, nb = CT.lae_rows()
    out = {"A": A, "B": B, "nb": nb, "V": CT.run("lae", "V", A, B),
           "V32": CT.run("lae", "V32", A, B), "VF": CT.run("lae", "VF", A, B)}
    out["S"] = CT.run("lae", "S", A[CT.N_BULK_ROWS:, 0], B[CT.N_BULK_ROWS:, 0])
    return out


def test_logaddexp_bulk(gpu):
    d = _lae()
    nb = d["nb"]
    A, B = d["A"][:nb], d["B"][:nb]
    assert np.abs(A - B).max() > 95 and np.abs(A - B).min() < 0.01
    ef = np.abs(d["VF"][:nb].astype(np.float64) - CT.lae64(A, B)) / CT.lae_unit(A, B)
    da, db = CT.lae_vjp64(A, B)
    ea = np.abs(d["V"][0][:nb].astype(np.float64) - da) / U1
    eb = np.abs(d["V"][1][:nb].astype(np.float64) - db) / U1
    print(f"logaddexp over {A.size} points: value {ef.max():.3f} (gate {CT.LAE_GATE}), "
          f"da {ea.max():.3f} (gate {CT.DA_GATE}), db {eb.max():.3f} (gate {CT.DB_GATE})")
    assert ef.max() <= CT.LAE_GATE
    assert ea.max() <= CT.DA_GATE and eb.max() <= CT.DB_GATE
    # the class cotangents sum to the incoming one, exactly
    np.testing.assert_array_equal(d["V"][0][:nb] + d["V"][1][:nb], np.ones_like(A))


def test_logaddexp_edges(gpu):
    d = _lae()
    nb = d["nb"]
    assert d["A"].shape[0] - nb == len(CT.LAE_EDGES)
    flat = lambda a: np.ascontiguousarray(a).reshape(-1)   # noqa: E731
    a, b = flat(d["A"][nb:]), flat(d["B"][nb:])
    skip = np.zeros(a.shape, bool)
    one = np.full(a.shape, U1)
    vf = flat(d["VF"][nb:])
    bad = X.edge_failures(vf, CT.lae64(a, b), CT.lae32(a, b), skip, CT.LAE_GATE,
                          unit=CT.lae_unit(a, b))
    assert bad.size == 0, [(float(a[i]), float(b[i]), float(vf[i])) for i in bad[:8]]
    for j, gate in ((0, CT.DA_GATE), (1, CT.DB_GATE)):
        vg = flat(d["V"][j][nb:])
        bad = X.edge_failures(vg, CT.lae_vjp64(a, b)[j], CT.lae_vjp32(a, b)[j], skip, gate, unit=one)
        assert bad.size == 0, [(j, float(a[i]), float(b[i]), float(vg[i])) for i in bad[:8]]
    # the classes the header states, on the first element of each edge row
    row = {tuple(str(float(t)) for t in e): k for k, e in enumerate(CT.LAE_EDGES)}
    val, ga, gb = d["VF"][nb:, 0], d["V"][0][nb:, 0], d["V"][1][nb:, 0]
    inf = np.inf

    def at(x, y):
        return row[tuple(str(float(F32(t))) for t in (x, y))]
    k = at(0.7, 0.7)
    assert val[k] == F32(0.7) + F32(np.log(2.0)) and ga[k] == 0.5 and gb[k] == 0.5
    for x, y, v, g in ((-inf, 1.5, 1.5, 0.0), (1.5, -inf, 1.5, 1.0), (-inf, -inf, -inf, 0.5),
                       (inf, inf, inf, 0.5), (inf, 1.0, inf, 1.0), (1.0, inf, inf, 0.0),
                       (inf, -inf, inf, 1.0), (1000.0, 0.0, 1000.0, 1.0), (0.0, 90.0, 90.0, 0.0)):
        k = at(x, y)
        assert val[k] == F32(v) and ga[k] == F32(g) and gb[k] == F32(1.0 - g), (x, y, val[k], ga[k])
    for x, y in ((np.nan, 1.0), (1.0, np.nan), (np.nan, np.nan), (np.nan, -inf)):
        k = at(x, y)
        assert np.isnan(val[k]) and np.isnan(ga[k]) and np.isnan(gb[k]), (x, y)


def test_logaddexp_forms_agree(gpu):
    """V (NMAX = 16) and V32 (NMAX = 32) bit-identical per element; form S
    (one element, scalar leaves) bit-identical to VF / V on the rows constant
    along the elements."""
    d = _lae()
    assert X.same_bits(d["V"][0], d["V32"][0]).all() and X.same_bits(d["V"][1], d["V32"][1]).all()
    lp, (ga, gb) = d["S"]
    c = CT.N_BULK_ROWS
    for j in (0, 1, CT.N_VEC - 1):
        assert X.same_bits(lp, d["VF"][c:, j]).all()
        assert X.same_bits(ga, d["V"][0][c:, j]).all() and X.same_bits(gb, d["V"][1][c:, j]).all()


@pytest.mark.parametrize("k", [0.0, 1.0])
def test_pick_is_exact_on_every_form(gpu, k):
    y = CT.pick_labels()
    b, c = CT.pick_rows()
    want, hit, miss = CT.pick(y, k, b, c)
    vf = CT.run("pick", "VF", b, c, k, y)
    assert X.same_bits(vf, want).all()
    ga, gb = CT.run("pick", "V", b, c, k, y)
    np.testing.assert_array_equal(ga, np.broadcast_to(hit, b.shape))
    np.testing.assert_array_equal(gb, np.broadcast_to(miss, b.shape))
    g32 = CT.run("pick", "V32", b, c, k, y)
    assert X.same_bits(ga, g32[0]).all() and X.same_bits(gb, g32[1]).all()
    assert hit.sum() > 0 and miss.sum() > 0 and np.isnan(y).any()
    if k == 0.0:                       # -0 is label 0; NaN is no label
        assert hit[0][np.signbit(y) & (y == 0)].all() and not hit[0][np.isnan(y)].any()
    for label in (k, k + 1.0, k + 0.5, np.nan):       # form S: in, out, between, NaN
        lp, (sa, sb) = CT.run("pick", "S", b[:3, 0], c[:3, 0], k, np.array([label], F32))
        w, h, ms = CT.pick(label, k, b[:3, 0], c[:3, 0])
        assert X.same_bits(lp, w).all() and np.all(sa == h) and np.all(sb == ms), label


def test_log_prob_does_not_overflow(gpu):
    """Logits (1000, 0, -1000): the naive log(sum(exp(.))) is inf from 88."""
    import mlx_mcmc_amd as m
    import mlx_mcmc_amd.core as mx
    from mlx_mcmc_amd import _engine, _trace

    for label, want in ((0.0, 0.0), (1.0, -1000.0), (2.0, -2000.0), (3.0, -np.inf), (0.5, -np.inf)):
        prog = _trace.compile_model(
            lambda p: mx.sum(m.Categorical(logits=p["e"]).log_prob(np.array([label], F32))),
            {"e": np.zeros(3, F32)})
        lp, g = _engine.logp_grad(prog, np.array([[1000.0, 0.0, -1000.0]], F32))
        assert float(lp.cpu().numpy()[0]) == want, (label, lp)
        g = g.cpu().numpy()[0]
        # y - softmax: the log-sum side keeps its finite cotangent at an invalid label
        hot = np.array([label == 0.0, label == 1.0, label == 2.0], F32)
        np.testing.assert_array_equal(g, hot - np.array([1.0, 0.0, 0.0], F32))


# ---- compiled evaluators -----------------------------------------------------------------
def _sample(algo, name, jit):
    import mlx_mcmc_amd as m
    from mlx_mcmc_amd import _lib, _trace

    lib = _lib.load()
    lib.mc_debug_expr_jit(1 if jit else 0)
    try:
        lp, init = CT.posterior_model(name, False)
        if algo == "hmc":
            s, _, info = m.hmc(lp, init, num_samples=12, num_warmup=12, step_size=0.05,
                               num_leapfrog_steps=5, key=m.random.key(4), num_chains=16,
                               progress=False, return_info=True, return_trace=True)
        elif algo == "nuts":
            s, _, info = m.nuts(lp, init, num_samples=8, num_warmup=8, step_size=0.05,
                                max_tree_depth=6, key=m.random.key(4), num_chains=16,
                                progress=False, return_info=True, return_trace=True)
        else:
            s, _, info = m.metropolis_hastings(lp, init, num_samples=40, proposal_scale=0.1,
                                               random_seed=4, num_chains=16, return_info=True,
                                               return_trace=True)
        state = lib.mc_program_expr_jit(_trace.compile_model(lp, init).handle)
    finally:
        lib.mc_debug_expr_jit(-1)
    return s, info, state


@pytest.mark.parametrize("algo,name", [("hmc", "intercept"), ("hmc", "regression"),
                                       ("nuts", "regression"), ("mh", "regression")])
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
    250 data elements each (tests/test_gpu_discrete.py _lane_model): 0.1 sum_i
    log p(y_ki | logits [0, a + theta_i x_ki, -theta_i x_ki]) — the packed
    LOGADDEXP and PICK cases of ex2_fwd / ex2_bwd."""
    rng = np.random.default_rng(63)
    xs = rng.uniform(0.5, 2.0, (9, N_LANE)).astype(F32) * rng.choice([-1.0, 1.0], (9, N_LANE)).astype(F32)
    ys = rng.integers(0, 3, (9, N_LANE)).astype(F32)
    init = {"theta": np.zeros(N_LANE, F32), "a": F32(0.0)}
    if oracle:
        import torch

        def log_prob(p):
            th, a = p["theta"].to(torch.float64), p["a"].to(torch.float64)
            lp = (float(X.C0_NORMAL) - 0.5 * th ** 2).sum() + (float(X.C0_NORMAL) - 0.5 * a ** 2)
            for k in range(9):
                x = CT._t(xs[k])
                E = torch.stack([torch.zeros_like(th), a + th * x, -(th * x)], 0)
                idx = torch.tensor(ys[k].astype(np.int64))[None, :]
                ll = torch.gather(E, 0, idx)[0] - torch.logsumexp(E, 0)
                lp = lp + float(F32(0.1)) * ll.sum()
            return lp
        return log_prob, init

    def log_prob(p):
        import mlx_mcmc_amd as m
        import mlx_mcmc_amd.core as mx
        lp = mx.sum(m.Normal(0, 1).log_prob(p["theta"])) + m.Normal(0, 1).log_prob(p["a"])
        for k in range(9):
            tx = p["theta"] * xs[k]
            lp = lp + 0.1 * mx.sum(m.Categorical(logits=[0.0, p["a"] + tx, -tx]).log_prob(ys[k]))
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
    """The lane kernel's pair code (ex2_fwd / ex2_bwd's packed LOGADDEXP and
    PICK cases) against the interpreter tape over two leapfrog steps from 16
    starts, as tests/test_gpu_discrete.py does: accepted draws held to equal
    bits, and to the float64 restatement's position."""
    from oracle import philox as R

    eps, seed, C = 0.05, 20, 16
    q0 = np.random.default_rng(7).normal(0.0, 0.3, (C, N_LANE + 1)).astype(F32)
    ql, tl = _two_leapfrogs(True, q0, seed, eps)
    qt, tt = _two_leapfrogs(False, q0, seed, eps)
    np.testing.assert_array_equal(tl["accepted"], tt["accepted"])
    assert tl["accepted"][:, 0].sum() >= 12
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


# ---- the models against the oracle -----------------------------------------------------------
def _points(prog, init, k=6, spread=0.3, seed=7):
    rng = np.random.default_rng(seed)
    base = prog.layout.flatten(init)
    return np.stack([base + rng.normal(0, spread, base.size).astype(F32) for _ in range(k)])


@pytest.mark.parametrize("name", ["intercept", "regression"])
def test_tape_matches_autograd(gpu, name):
    """tests/test_gpu_discrete.py test_tape_matches_autograd's bars."""
    from mlx_mcmc_amd import _engine, _lib, _trace

    lp_fn, init = CT.posterior_model(name, False)
    prog = _trace.compile_model(lp_fn, init)
    assert any(t.dist == _lib.MC_DIST_EXPR for t in prog.model.terms)
    assert prog.slice_kernel == "unsliced"
    olp, oinit = CT.posterior_model(name, True)
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


def test_two_classes_equal_bernoulli(gpu):
    """Categorical(logits=[0, eta]) against Bernoulli(logits=eta) on the same
    data: an independent check of the whole lowering.  Per observation the two
    log masses differ by at most the two nodes' gates — Bernoulli's 8 ulp of
    its value (tests/_discrete.py) and LOGADDEXP's 8 ulp of max(0, |eta|) +
    log1p(e), plus the final difference's half ulp; the gradient factors by
    Bernoulli's 3 and LOGADDEXP's 6 ulp of |y| + sigma <= 2 — summed over the
    N = 67 observations with their |x_i| (and the two sums' own roundings, N / 2
    ulp of the largest partial sum each)."""
    import mlx_mcmc_amd as m
    import mlx_mcmc_amd.core as mx
    from mlx_mcmc_amd import _engine, _trace

    d = DS.data()
    init = {"a": F32(0.0), "b": F32(0.0)}
    cat = _trace.compile_model(lambda p: mx.sum(m.Categorical(
        logits=[0.0, p["a"] + p["b"] * d.x]).log_prob(d.yb)), init)
    ber = _trace.compile_model(lambda p: mx.sum(m.Bernoulli(
        logits=p["a"] + p["b"] * d.x).log_prob(d.yb)), init)
    pts = _points(cat, init, k=8, spread=1.0)
    lc, gc = (t.cpu().numpy().astype(np.float64) for t in _engine.logp_grad(cat, pts))
    lb, gb = (t.cpu().numpy().astype(np.float64) for t in _engine.logp_grad(ber, pts))
    x = d.x.astype(np.float64)
    for i, q in enumerate(pts):
        eta = np.abs(q[0] + q[1] * x)
        lse = eta + np.log1p(np.exp(-eta))                  # max(0, |eta|) + log1p(e), >= |value|
        tol_v = ((DS.FWD_GATE["bernoulli"] + CT.LAE_GATE + 0.5) * X.ulp(lse)).sum()
        tol_v += d.N * float(X.ulp(lse.sum()))
        u2 = float(X.ulp(2.0))
        per = (DS.VJP_GATE["bernoulli"] + CT.DB_GATE) * u2
        tol_g = np.array([per * d.N, per * np.abs(x).sum()])
        tol_g += d.N * X.ulp(np.array([d.N, np.abs(x).sum()]))
        assert abs(lc[i] - lb[i]) <= tol_v, (i, lc[i], lb[i], tol_v)
        assert np.all(np.abs(gc[i] - gb[i]) <= tol_g), (i, gc[i], gb[i], tol_g)


# (starts away from the mode; fixed HMC step sizes at which the float64
# restatement's decisions are a mix — 26 and 22 of the first 30 accepted, the
# rejected log ratios between -0.4 and -3.7 — and its trees reach depth 3,
# checked with oracle.samplers on the CPU.  The step sizes stay clear of the
# stability edge, 0.42 for the intercept model, beyond which the trajectories
# blow up: next to it two float32 evaluations of one trajectory separate
# faster than the near-tie bound allows — at 0.345 the intercept run's H_init
# was 11 ulp from the restatement's at iteration 22, bound 8)
START = {"intercept": {"e1": 0.5, "e2": -0.8},
         "regression": {"a1": 0.6, "b1": 1.0, "a2": -0.5, "b2": -0.9}}
HMC_EPS = {"intercept": 0.33, "regression": 0.36}


@pytest.mark.parametrize("name", ["intercept", "regression"])
def test_hmc_trace_matches_oracle(gpu, name):
    import mlx_mcmc_amd as m

    lp, _ = CT.posterior_model(name, False)
    olp, _ = CT.posterior_model(name, True)
    start = {k: F32(v) for k, v in START[name].items()}
    seed, n = 3, 40
    kw = dict(num_samples=40, num_warmup=40, step_size=HMC_EPS[name], num_leapfrog_steps=10,
              adapt_step_size=False)
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
    acc = np.asarray(ref.trace["accepted"][:same])
    assert same >= 30 and acc.any() and not acc.all()


@pytest.mark.parametrize("name", ["intercept", "regression"])
def test_nuts_trees_match_oracle(gpu, name):
    import mlx_mcmc_amd as m

    lp, _ = CT.posterior_model(name, False)
    olp, _ = CT.posterior_model(name, True)
    start = {k: F32(v) for k, v in START[name].items()}
    n_w, n_s = 30, 10
    _, _, info = m.nuts(lp, start, num_samples=n_s, num_warmup=n_w, step_size=0.1,
                        key=m.random.key(2), progress=False, return_info=True, return_trace=True)
    assert info.extra["kernel"] == "tape"
    ref = S.nuts(olp, start, num_samples=n_s, num_warmup=n_w, step_size=0.1, seed=2)
    same = 0
    for i in range(n_w + n_s):
        if (info.trace["tree_depth"][0][i] != ref.trace["depth"][i]
                or info.trace["n_leapfrog"][0][i] != ref.trace["leaves"][i]):
            break
        same += 1
    assert same >= 10, f"trees diverged at iteration {same}"
    assert max(ref.trace["depth"][:same]) >= 2


@pytest.mark.parametrize("name", ["intercept", "regression"])
def test_mh_decisions_match_oracle(gpu, name):
    import mlx_mcmc_amd as m

    lp, _ = CT.posterior_model(name, False)
    olp, _ = CT.posterior_model(name, True)
    start = {k: float(v) for k, v in START[name].items()}
    n = 150
    s, _, info = m.metropolis_hastings(lp, start, num_samples=n, proposal_scale=0.15,
                                       random_seed=5, return_info=True, return_trace=True)
    ref = S.metropolis_hastings(olp, start, num_samples=n, proposal_scale=0.15, random_seed=5)
    acc, racc = info.trace["accepted"][0].astype(bool), np.array(ref.trace["accepted"])
    assert 0 < racc.mean() < 1
    lu = log_u(m.random.key(5).seed, 0, n)
    for i in range(n):          # a flip only at a proven near-tie
        if acc[i] != racc[i]:
            assert abs(float(lu[i]) - ref.trace["ratio"][i]) <= tie_bound(ref.trace["logp"][i]), i
            assert i >= 100, f"decisions agree for {i} of {n} steps only"
            break
    else:
        k0 = list(START[name])[0]
        np.testing.assert_allclose(s[k0], ref.samples[:, 0], rtol=1e-5, atol=1e-6)


def test_example_05_probs_model_under_mh(gpu):
    """p3 = 1 - p1 - p2 under Categorical(probs=): from (0.33, 0.33) with
    proposal_scale 0.02 the decisions equal the float64 restatement's, the
    proposals outside the simplex (log density -inf, 25 of the 150 in the
    restatement) included; the tape gives -inf there and nothing else."""
    import mlx_mcmc_amd as m
    from mlx_mcmc_amd import _engine, _trace

    lp, init = CT.simplex_model(False)
    olp, _ = CT.simplex_model(True)
    n = 150
    s, _, info = m.metropolis_hastings(lp, dict(init), num_samples=n, proposal_scale=0.02,
                                       random_seed=5, return_info=True, return_trace=True)
    ref = S.metropolis_hastings(olp, {k: float(v) for k, v in init.items()}, num_samples=n,
                                proposal_scale=0.02, random_seed=5)
    outside = [i for i, r in enumerate(ref.trace["ratio"]) if r == -np.inf]
    assert len(outside) >= 10 and 0 < np.mean(ref.trace["accepted"]) < 1
    acc = info.trace["accepted"][0].astype(bool)
    assert list(acc) == ref.trace["accepted"]
    np.testing.assert_allclose(s["p1"], ref.samples[:, 0], rtol=1e-5, atol=1e-6)
    prog = _trace.compile_model(lp, init)
    pts = np.array([[0.5, 0.3], [0.7, 0.4], [-0.1, 0.5], [0.5, 0.5], [0.2, 1.1]], F32)
    got = _engine.logp_grad(prog, pts)[0].cpu().numpy()
    M = S.EagerModel(olp, init)
    assert np.isfinite(got[0]) and abs(got[0] - M.logp(pts[0])) <= 1e-4 * abs(got[0])
    assert np.all(got[1:] == -np.inf)


def test_exact_posterior(gpu):
    """Logits [0, e1, e2], Normal(0, 2) priors, counts 14 / 9 / 7, against the
    2-D quadrature of tests/_categorical.py: means within 4 MCSE (the MCSE from
    the spread of the 32 chain means), standard deviations within 10 %
    (test_conjugate_posterior_mean's bars).  A fixed step size of 0.07, ten
    steps: oracle.samplers.hmc at these settings meets the bars on the CPU
    with 8 chains."""
    import mlx_mcmc_amd as m

    mean, sd = CT.exact_posterior()
    lp, init = CT.posterior_model("intercept", False, y=CT.exact_labels())
    s, _, info = m.hmc(lp, init, num_samples=500, num_warmup=100, step_size=0.07,
                       num_leapfrog_steps=10, adapt_step_size=False, key=m.random.key(1),
                       num_chains=32, progress=False, return_info=True)
    assert np.all(info.accept_rate > 0.3)
    for j, k in enumerate(("e1", "e2")):
        d = np.asarray(s[k])
        assert d.shape == (32, 500)
        mcse = d.mean(1).std() / np.sqrt(d.shape[0])
        print(f"{k}: mean {d.mean():.5f} exact {mean[j]:.5f} (MCSE {mcse:.5f}), sd {d.std():.4f} "
              f"exact {sd[j]:.4f}")
        assert abs(d.mean() - mean[j]) < 4 * mcse
        assert abs(d.std() - sd[j]) < 0.1 * sd[j]


def test_categorical_takes_the_hand_written_route(gpu):
    """N = 100 K, 64 chains, the default plan: the node model runs on the
    kernel route of the hand-written model (scripts/bench_categorical.py's two
    models: one-hot mx.where masks and the naive log(1 + exp e1 + exp e2), each
    logit built once so that the hand-written model holds 4 N data floats.
    Written with + / * it expands the affine logits at both uses, holds 6 N
    floats and runs on the unsliced tape — "slice data exceed the LDS budget" —
    where the node model, 2 N floats, stays on the lanes)."""
    import mlx_mcmc_amd as m
    from mlx_mcmc_amd import _trace
    from scripts.bench_categorical import models

    node, hand, init = models(100_000)
    routes = []
    for lp in (hand, node):
        prog = _trace.compile_model(lp, init)
        _, _, info = m.hmc(lp, init, num_samples=2, num_warmup=2, step_size=1e-3,
                           num_leapfrog_steps=3, key=m.random.key(1), num_chains=64,
                           progress=False, return_info=True)
        routes.append((info.extra["kernel"], prog.slice_kernel, prog.num_slices))
        print("route:", routes[-1], prog.kernel_note)
    print("routes (hand-written, Categorical):", routes)
    assert routes[0] == routes[1] and routes[0][0] != "unsliced", routes


# ---- WAIC and PSIS-LOO -------------------------------------------------------------------------
def _D():
    from mlx_mcmc_amd import diagnostics
    return diagnostics


def test_waic_and_loo(gpu):
    """C = 3, S = 37 as tests/test_gpu_discrete.py: the matrix and statistics
    at tests/_pointwise.py's bars, PSIS-LOO at tests/_psis.py's."""
    model = CT.likelihood()
    q = CT.draws(model)
    lay = CT.layout_of(model)
    got = _D().pointwise_log_likelihood(model.log_likelihood, q, lay, matrix=True, group=False)
    ref = model.ll(q, np.float64)
    mat = got["matrix"].cpu().numpy()
    assert mat.shape == (3, 37, CT.N_OBS)
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
    own = PS.psis_matrix(mat.reshape(-1, CT.N_OBS))
    r64 = PS.psis_matrix(ref.reshape(-1, CT.N_OBS))
    assert loo["tail_len"] == own["tail_len"] == 23
    pw = loo["pointwise"]
    np.testing.assert_array_equal(loo["tail_n"], own["n"])
    for f, g in (("khat", pw["khat"]), ("elpd", pw["elpd_loo"])):
        np.testing.assert_allclose(g, own[f], rtol=1e-10, atol=0, err_msg=f)
    np.testing.assert_allclose(pw["elpd_loo"], r64["elpd"], rtol=PS.RTOL, atol=PS.ATOL)
    np.testing.assert_allclose(pw["khat"], r64["khat"], rtol=PS.RTOL, atol=PS.ATOL)
    assert loo["n_nonfinite"] == 0


def test_no_sampling_distribution_yet(gpu):
    """Posterior predictive replicates of a Categorical term are not part of
    this change: the term keeps the expression terms' error."""
    model = CT.likelihood()
    with pytest.raises(Exception, match="has no sampling distribution"):
        _D().posterior_predictive(model.log_likelihood, CT.draws(model), CT.layout_of(model),
                                  seed=3, group=False)


# ---- Categorical.sample ---------------------------------------------------------------------------
def test_sample_known_answers(gpu):
    """The reference's sampling KATs with its bounds
    (tests/test_new_distributions.py:228-256)."""
    import mlx_mcmc_amd as m

    s = m.Categorical(probs=[0.2, 0.5, 0.3]).sample(m.random.key(0), shape=(1000,))
    assert s.shape == (1000,) and np.all(s >= 0) and np.all(s < 3)
    s = m.Categorical(probs=[0.1, 0.6, 0.3]).sample(m.random.key(42), shape=(10000,))
    for k, p in enumerate((0.1, 0.6, 0.3)):
        assert np.isclose(np.mean(s == k), p, atol=0.02)
    s = m.Categorical(probs=[1 / 3, 1 / 3, 1 / 3]).sample(m.random.key(123), shape=(9000,))
    for k in range(3):
        assert 2700 < np.sum(s == k) < 3300
    assert np.ndim(m.Categorical(logits=[0.0, 1.0]).sample(m.random.key(1))) == 0
