"""Every expression node (include/mcmc355.h mc_expr_op) on every evaluator,
one op at a time, against the float64 table of tests/_expr_ops.py (which
tests/test_expr_ops_reference.py holds to torch float64 autograd).

The interpreter (csrc/eval.h eval_expr_n; mc_logp_grad never runs compiled
code): per op one program per form (S: the wave-task path, V / VF: the strided
path's NMAX = 16 instantiation, V32: NMAX = 32), 4096 bulk points plus the
edge inputs in one launch each.
  * value and VJP in ulp of the float32 spacing of the reference (a log
    density: of its terms' summed magnitudes, _expr_ops.units): 0 for the
    single-operation ops, eval.h's documented figures for div / exp / log,
    twice the measured figure (MEASURED_ULP) for the rest, a VJP stated
    through the node's value v with K_fwd ulp(v) |d formula / d v| on top;
  * edges by class (NaN, the sign of an infinity, zero or not; -inf with zero
    cotangents outside a support) and finite ones by the same ulp bound
    against the float64 reference; the one-rounding-per-operation float32
    evaluation is an alternative only at the points where it departs from
    that reference (an intermediate left the float32 range); outside ex_div's
    divisor range what its comment states is pinned
    (test_div_outside_its_range), and nothing more is asserted of a formula
    that divides there;
  * forms S, V, VF and V32 bit-identical per element: measured so, every form
    runs ex_fwd / ex_bwd on the same float32 inputs;
  * the value-only pass (Metropolis-Hastings) against a float64 restatement.

What the measurement found (MI355X): ex_log1p returned 0 for arguments beyond
2^126 (its quotient x / (u - 1) left ex_div's range) — fixed, the quotient is
left out where it is 1; ex_div returns +-inf for a subnormal divisor whatever
the dividend, which its comment did not say — the comment now does; ex_exp's
subnormal results are zero (the unit flushes them) — the comment now says so.
Pinned, not derived: exp(x) = 0 for x < log(FLT_MIN); a quotient of 0 for a
divisor beyond 2^126 and of +-inf for a subnormal one.

The compiled evaluators run three models that together hold every op as a
node (_expr_ops.GROUPS): the tape JIT through tests/test_gpu_expr_jit.py's
bit-identity bar (tests/_jit_models.py MODELS), the lane JIT (k_hmc_lr,
ex2_fwd / ex2_bwd pair code) here against the interpreter tape of the same
program — two leapfrog steps, since a launch's first gradient is the
initialisation kernel's (the interpreter's) on every kernel — and ops_transc
on the sliced NUTS and MH kernels.  The planner puts
no expression program on the lanes in one slice (slice_kernel="lanes" with
num_slices=1 is an EngineError, asserted below: a real limit, csrc/program.hip
plan_lanes1), so the lane runs take the automatic plan's 4 slices; an element
of theta still belongs to one slice, its gradient unsummed.
"""
import functools
import math

import numpy as np
import pytest

import _expr_ops as X
import workloads as W
from _near_tie import compare_trace, log_u, tie_bound

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _device(name):
    """Every form of the op over inputs(name), one launch each."""
    args, nb = X.inputs(name)
    out = {"args": args, "nb": nb}
    if name != "where":
        out["S"] = X.run_S(name, args)
    out["V"] = X.run_V(name, args)
    out["V32"] = X.run_V(name, args, "V32")
    out["VF"] = X.run_V(name, args, "VF")
    return out


def _show(name, args, i):
    return f"{name}({', '.join(repr(float(a[i])) for a in args)})"


@pytest.mark.parametrize("name", X.OPS)
def test_value_and_vjp_bulk(gpu, name):
    d = _device(name)
    nb = d["nb"]
    args = [a[:nb] for a in d["args"]]
    forms = [("V", d["VF"][:nb], [g[:nb] for g in d["V"]])]
    if name != "where":
        forms.append(("S", d["S"][0][:nb], [g[:nb] for g in d["S"][1]]))
    for form, fwd, vjps in forms:
        err = X.bulk_errors(name, args, fwd, vjps)
        print(f"{name} form {form}: max ulp error " +
              ", ".join(f"{k}: {v:.3f}" for k, v in err.items()))
        if name in X.EXACT:
            assert X.same_bits(fwd, X.fwd64(name, *args).astype(np.float32)).all()
            for g, r in zip(vjps, X.vjp64(name, *args)):
                assert X.same_bits(g, r.astype(np.float32)).all()
            continue
        assert err["fwd"] <= X.fwd_gate(name), (name, form, err)
        for j in range(len(vjps)):
            assert err[j] <= X.vjp_gate(name, j), (name, form, j, err)


@pytest.mark.parametrize("name", X.OPS)
def test_edges(gpu, name):
    d = _device(name)
    nb = d["nb"]
    args = [a[nb:] for a in d["args"]]
    skip_f, skip_v = X.unspecified(name, *args)
    uf, ug = X.units(name, *args)
    bad = X.edge_failures(d["VF"][nb:], X.fwd64(name, *args), X.fwd32(name, *args), skip_f,
                          X.fwd_gate(name), unit=uf)
    assert bad.size == 0, [(_show(name, args, i), float(d["VF"][nb + i])) for i in bad[:8]]
    slack = X.vjp_slack(name, args, X.fwd_gate(name))
    for j, (r64, r32) in enumerate(zip(X.vjp64(name, *args), X.vjp32(name, *args))):
        g = d["V"][j][nb:]
        bad = X.edge_failures(g, r64, r32, skip_v, X.vjp_gate(name, j), slack[j], unit=ug[j])
        assert bad.size == 0, [(_show(name, args, i), j, float(g[i])) for i in bad[:8]]
    # outside a support: -inf with zero cotangents
    if name in ("halfnormal_lp", "exponential_lp", "gamma_lp", "beta_lp"):
        v = args[0]
        out = (v < 0) if name in ("halfnormal_lp", "exponential_lp") else ~(v > 0)
        if name == "beta_lp":
            out |= ~(v < 1)
        out &= ~np.isnan(v)
        assert out.any()
        assert np.all(d["VF"][nb:][out] == -np.inf)
        for g in d["V"]:
            assert np.all(g[nb:][out] == 0.0)


@pytest.mark.parametrize("name", X.OPS)
def test_forms_agree(gpu, name):
    """S (wave-task), V (strided, NMAX = 16) and V32 (NMAX = 32) bit-identical
    per element, bulk and edges; so is form VF's value to form S's.  That
    each form takes the path named is known from the host tables only
    (tests/test_expr_ops_reference.py test_builders_trace_to_the_intended_root
    and the dispatch rules it cites): the library has no query for the path a
    launch took, so a change of those rules could leave this test comparing
    one path with itself."""
    d = _device(name)
    for j, (a, b) in enumerate(zip(d["V"], d["V32"])):
        ne = np.nonzero(~X.same_bits(a, b))[0]
        assert ne.size == 0, ("V32", j, [_show(name, d["args"], i) for i in ne[:8]])
    if name == "where":
        return
    ne = np.nonzero(~X.same_bits(d["S"][0], d["VF"]))[0]
    assert ne.size == 0, ("value", [_show(name, d["args"], i) for i in ne[:8]])
    for j, (a, b) in enumerate(zip(d["S"][1], d["V"])):
        ne = np.nonzero(~X.same_bits(a, b))[0]
        assert ne.size == 0, ("S", j, [_show(name, d["args"], i) for i in ne[:8]])


def test_log1p_beyond_the_division_range(gpu):
    """The finding: log1p of arguments beyond 2^126 (0 before the fix)."""
    x = np.array([1e38, 2.0 ** 126 * 1.5, X.FLT_MAX, 2.0 ** 126], np.float32)
    fwd, _ = X.run_S("log1p", (x,))
    assert np.all(X.ulp_err(fwd, X.fwd64("log1p", x)) <= X.fwd_gate("log1p")), fwd


def test_div_outside_its_range(gpu):
    """What ex_div's comment says of the divisors outside its range, pinned:
    beyond 2^126 in magnitude the quotient is 0, a subnormal divisor gives
    +-inf (the sign the quotient's) even where the quotient is finite."""
    big = [(3.0, 2.0 ** 126 * (1 + 2.0 ** -22)), (3.0, 2.0 ** 127), (-5.0, -1.5 * 2.0 ** 127),
           (X.FLT_MAX, X.FLT_MAX), (-X.FLT_MAX, X.FLT_MAX)]
    sub = [(1.0, X.SUBN), (3.0, -X.SUBN), (8 * X.SUBN, X.SUBN), (1e-30, 2e-39),
           (X.FLT_MIN, X.SUBN), (-X.FLT_MIN, X.SUBN)]
    x, y = (np.array(c, np.float32) for c in zip(*(big + sub)))
    fwd, _ = X.run_S("div", (x, y))
    assert np.all(fwd[:len(big)] == 0.0), fwd
    want = np.where((x < 0) != (y < 0), -np.inf, np.inf)[len(big):]
    np.testing.assert_array_equal(fwd[len(big):], want)
    # the last divisor inside the range: within the documented ulp
    x, y = np.array([3.0, -5.0], np.float32), np.array([2.0 ** 126, -2.0 ** 126], np.float32)
    fwd, _ = X.run_S("div", (x, y))
    assert np.all(X.ulp_err(fwd, X.fwd64("div", x, y)) <= X.fwd_gate("div")), fwd


# ---- the value-only pass (Metropolis-Hastings, eval_lp_grad<WPC, true>) ----------
_MH_START = {"log1p": (0.5,), "pow": (1.5, 0.7), "gamma_lp": (0.8, 2.5, 1.3)}


@pytest.mark.parametrize("name,scale", [("log1p", 0.2), ("pow", 0.2), ("gamma_lp", 0.05)])
def test_value_only_pass_matches_float64(gpu, name, scale):
    """metropolis_hastings on the form-V program for 20 iterations, the
    interpreter's value-only pass: decisions equal a float64 restatement's
    (oracle/samplers.py over the torch float64 op) unless |log U - ratio| is
    within tests/_near_tie.py's bound, log p before a flip within it."""
    import mlx_mcmc_amd as m
    from mlx_mcmc_amd import _lib
    from oracle import samplers as S

    built = X.build_V(name, [np.zeros(X.N_VEC, np.float32)] * X.arity(name))
    init = {k: np.full(X.N_VEC, v, np.float32) for k, v in zip(built.init, _MH_START[name])}
    n, seed = 20, 5
    lib = _lib.load()
    lib.mc_debug_expr_jit(0)
    try:
        s, rate, info = m.metropolis_hastings(built.log_prob, init, num_samples=n,
                                              proposal_scale=scale, random_seed=seed,
                                              return_info=True, return_trace=True)
    finally:
        lib.mc_debug_expr_jit(-1)
    ref = S.metropolis_hastings(X.oracle_V(name), init, num_samples=n, proposal_scale=scale,
                                random_seed=seed)
    acc = info.trace["accepted"][0].astype(bool)
    racc = np.array(ref.trace["accepted"])
    assert 0 < racc.sum() < n, "mixed decisions"
    lu = log_u(m.random.key(seed).seed, 0, n)
    same = n
    for i in range(n):
        tie = tie_bound(ref.trace["logp"][i])
        if acc[i] != racc[i]:
            gap = abs(float(lu[i]) - ref.trace["ratio"][i])
            assert gap <= tie, f"{name}: flip at {i} is no near-tie: gap {gap} > {tie}"
            print(f"{name}: decisions identical for {i} of {n}, near-tie at {i}")
            same = i
            break
        assert abs(float(info.trace["energy"][0][i]) - ref.trace["logp"][i]) <= tie, (name, i)
    assert same >= 10, f"{name}: compared only {same} of {n} iterations"


def _capture_programs(monkeypatch):
    """The programs the samplers compile, so that a test can ask the one that
    ran for its kernel and JIT state."""
    from mlx_mcmc_amd import _trace

    made = []
    orig = _trace.compile_model

    def compile_model(*a, **k):
        made.append(orig(*a, **k))
        return made[-1]
    monkeypatch.setattr(_trace, "compile_model", compile_model)
    return made


# ---- the lane JIT (k_hmc_lr: ex2_fwd / ex2_bwd) against the interpreter tape -------
def _k_op(group):
    return max(max([X.fwd_gate(n)] + [X.vjp_gate(n, j) for j in range(len(X.diff_args(n)))])
               for n in X.GROUP_OPS[group])


def _two_leapfrogs(group, lanes, q0, seed, eps):
    """num_leapfrog_steps=2, no adaptation, num_warmup=0, num_samples=1."""
    import torch

    from mlx_mcmc_amd import _engine, _lib, _trace

    lib = _lib.load()
    lp, init = X.group_model(group)(W.ns_product())
    C = q0.shape[0]
    lib.mc_debug_expr_jit(-1 if lanes else 0)
    try:
        prog = (_trace.compile_model(lp, init, slices=4, slice_kernel="lanes") if lanes
                else _trace.compile_model(lp, init, slices=1))
        if lanes:
            assert prog.slice_kernel == "lanes" and prog.num_slices == 4, prog.kernel_note
            assert not prog.kernel_note, prog.kernel_note
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


# seed and spread of the starts (chosen on the CPU: the float64 restatement
# accepts 15, 16 and 16 of the 16)
_PROBE = {"ops_arith": (4, 0.6), "ops_transc": (20, 0.3), "ops_density": (20, 0.3)}


def _probe_reference(group, q0, seed, eps):
    """The two leapfrog steps of every chain in float64 (the shared Philox
    normals and accept draw): g1 = g(q1), the momentum p32 that moves q1 to
    q2, q2, H_init and the decision."""
    from oracle import philox as R
    from oracle import samplers as S

    olp, oinit = X.group_model(group)(W.ns_oracle())
    M = S.EagerModel(olp, oinit)
    ref = []
    for c in range(q0.shape[0]):
        q = q0[c].astype(np.float64)
        p0 = np.asarray(R.momentum(seed, c, 0, M.D), np.float64)
        lp0, g0 = _lp_grad64(M, q)
        ph = p0 + 0.5 * eps * g0
        q1 = q + eps * ph
        _, g1 = _lp_grad64(M, q1)
        p32 = ph + eps * g1
        q2 = q1 + eps * p32
        lp2, g2 = _lp_grad64(M, q2)
        p2 = p32 + 0.5 * eps * g2
        h0, h2 = -lp0 + 0.5 * p0 @ p0, -lp2 + 0.5 * p2 @ p2
        lu = float(R.logf_u01(R.uniform(seed, c, 0, R.TAG_ACCEPT)))
        ref.append(dict(g1=g1, p32=p32, q2=q2, h0=h0, acc=lu < -(h2 - h0)))
    return ref


@pytest.mark.parametrize("group", list(X.GROUPS))
def test_lane_jit_two_leapfrogs(gpu, group):
    """Two leapfrog steps from 16 starts.  The launch's first gradient g(q0)
    and H_init come from the initialisation kernel, which runs the statically
    compiled interpreter for the lane program and the tape program alike
    (csrc/api.hip k_init), so one leapfrog step would compare the interpreter
    with itself.  The second step moves q1 = q0 + eps (p0 + (eps / 2) g(q0))
    — the same bits in both runs — to q2 = q1 + eps (p_half + eps g(q1)), and
    g(q1) is the running kernel's own: the lane kernel's pair code (ex2_fwd /
    ex2_bwd) against the interpreter tape.  The gradient element of a
    parameter-vector leaf is unsummed, so per element of theta the accepted
    draws agree within eps^2 K_op ulp(|g(q1)|) + 2 ulp(eps |p_3/2|) +
    2 ulp(|q2|): K_op, the largest gate of the group's ops, for the two
    evaluations of the gradient, one ulp of the momentum for each of its two
    updates, and the rounding of the position (g(q1), p_3/2 = p_half + eps g(q1)
    and q2 from the float64 restatement and the shared Philox normals).  The
    starts and the seed are such that the restatement alone accepts at least
    14 of the 16.  H_init is not compared between the runs (the same number
    from k_init on both sides); it is held to the restatement, and the short
    run compares the later iterations' energies."""
    eps, (seed, spread), C = 0.25, _PROBE[group], 16
    _, init = X.group_model(group)(W.ns_product())
    D = sum(int(np.size(v)) for v in init.values())
    q0 = np.random.default_rng(7).normal(0.0, spread, (C, D)).astype(np.float32)
    nth = X.N_GROUP
    ref = _probe_reference(group, q0, seed, eps)
    assert sum(r["acc"] for r in ref) >= 14, [r["acc"] for r in ref]
    ql, tl = _two_leapfrogs(group, True, q0, seed, eps)
    qt, tt = _two_leapfrogs(group, False, q0, seed, eps)
    assert tl["accepted"][:, 0].sum() >= 14
    np.testing.assert_array_equal(tl["accepted"], tt["accepted"])
    K = _k_op(group)
    worst = 0.0
    for c in range(C):
        r = ref[c]
        assert abs(float(tt["energy"][c, 0]) - r["h0"]) <= tie_bound(r["h0"]), c
        if not tl["accepted"][c, 0]:
            np.testing.assert_array_equal(ql[c], q0[c])
            continue
        bound = (eps * eps * K * X.ulp(r["g1"]) + 2 * X.ulp(eps * r["p32"])
                 + 2 * X.ulp(r["q2"]))[:nth]
        diff = np.abs(ql[c, :nth].astype(np.float64) - qt[c, :nth])
        worst = max(worst, float(np.max(diff / bound)))
        assert np.all(diff <= bound), (group, c, int(np.argmax(diff / bound)))
        # (both against the restatement: the moved position itself)
        np.testing.assert_allclose(ql[c], r["q2"], rtol=2e-5, atol=2e-6)
    ndiff = int((ql[:, :nth] != qt[:, :nth]).sum())
    print(f"{group}: lane vs tape draws differ by at most {worst:.3f} of the bound, "
          f"{ndiff} of {ql[:, :nth].size} elements of theta differ in bits")
    # Measured: not one element of theta differs.  eval.h states that each
    # component of the pair code is bit-identical to the scalar path's result,
    # and an element of theta sums its terms in term order on both kernels:
    # held to that.  (A hand mutation of ex2_exp, its low part of x log2(e)
    # dropped, fails the bound above on ops_transc.)
    assert ndiff == 0, f"{group}: {ndiff} elements of theta differ between lanes and tape"


@pytest.mark.parametrize("group", list(X.GROUPS))
def test_lanes_decline_one_slice(gpu, group):
    """The limit that keeps the lane runs at 4 slices: stated, not skipped."""
    from mlx_mcmc_amd import _lib, _trace

    lp, init = X.group_model(group)(W.ns_product())
    with pytest.raises(_lib.EngineError, match="an unsliced expression program runs on the tape"):
        _trace.compile_model(lp, init, slices=1, slice_kernel="lanes")
    # the automatic plan: 4 slices on the lanes
    prog = _trace.compile_model(lp, init)
    assert prog.slice_kernel == "lanes" and prog.num_slices == 4, prog.kernel_note


def _lp_grad64(M, q):
    import torch

    x = torch.tensor(np.asarray(q, np.float64), requires_grad=True)
    lp = M.fn(M._params(x))
    (g,) = torch.autograd.grad(lp, x)
    return float(lp.detach()), g.numpy()


@pytest.mark.parametrize("group", list(X.GROUPS))
def test_lane_jit_short_run(gpu, group, monkeypatch):
    """12 warmup + 12 draws, 8 chains: decisions, log ratios, H_init and step
    sizes equal the interpreter tape's until a proven near-tie, at least 80 %
    of the chain-iterations compared."""
    import mlx_mcmc_amd as m
    from mlx_mcmc_amd import _lib

    lib = _lib.load()
    lp, init = X.group_model(group)(W.ns_product())
    C, n, seed = 8, 24, 9
    D = sum(int(np.size(v)) for v in init.values())
    q0 = np.random.default_rng(8).normal(0.0, 0.3, (C, D)).astype(np.float32)
    # (step sizes at which the decisions are a mix)
    eps = {"ops_arith": 0.05, "ops_transc": 0.25, "ops_density": 0.05}[group]
    kw = dict(num_samples=12, num_warmup=12, step_size=eps, num_leapfrog_steps=5,
              key=m.random.key(seed), num_chains=C, progress=False, return_info=True,
              return_trace=True, initial_positions=q0)
    made = _capture_programs(monkeypatch)
    _, _, il = m.hmc(lp, init, slice_kernel="lanes", num_slices=4, **kw)
    assert il.extra["kernel"] == "lanes" and "kernel_note" not in il.extra
    assert len(made) == 1 and made[0].slice_kernel == "lanes" and made[0].num_slices == 4
    assert lib.mc_program_expr_jit(made[0].handle) == 1, made[0].kernel_note
    lib.mc_debug_expr_jit(0)
    try:
        _, _, it = m.hmc(lp, init, num_slices=1, **kw)
        assert lib.mc_program_expr_jit(made[1].handle) == 0
    finally:
        lib.mc_debug_expr_jit(-1)
    assert it.extra["kernel"] == "unsliced"
    total = 0
    for c in range(C):
        a = {"accepted": il.trace["accepted"][c], "ratio": il.trace["accept_stat"][c],
             "step_size": il.trace["step_size"][c], "energy": il.trace["energy"][c]}
        b = {"accepted": it.trace["accepted"][c], "ratio": it.trace["accept_stat"][c],
             "step_size": it.trace["step_size"][c], "energy": it.trace["energy"][c],
             "log_u": log_u(seed, c, n)}
        total += compare_trace(a, b, f"{group} chain {c}", verbose=True)
    acc = it.trace["accepted"].astype(bool)
    assert 0 < acc.sum() < acc.size, "mixed decisions"
    assert total >= math.ceil(0.8 * C * n), f"{group}: compared {total} of {C * n}"


# ---- the sliced NUTS and MH kernels: the same generated term code ------------------
def _start(group, C, seed):
    _, init = X.group_model(group)(W.ns_product())
    D = sum(int(np.size(v)) for v in init.values())
    return np.random.default_rng(seed).normal(0.0, 0.3, (C, D)).astype(np.float32)


def test_sliced_nuts_trees_equal_the_tape(gpu, monkeypatch):
    """ops_transc on k_nuts_sl at a fixed step size: tree depths and leaf
    counts identical to the interpreter tape's (k_nuts, JIT off) for at least
    6 iterations on every chain."""
    import mlx_mcmc_amd as m
    from mlx_mcmc_amd import _lib

    lib = _lib.load()
    lp, init = X.group_model("ops_transc")(W.ns_product())
    C = 8
    kw = dict(num_samples=8, num_warmup=4, step_size=0.05, max_tree_depth=6,
              adapt_step_size=False, key=m.random.key(12), num_chains=C, progress=False,
              return_info=True, return_trace=True, initial_positions=_start("ops_transc", C, 3))
    made = _capture_programs(monkeypatch)
    _, _, a = m.nuts(lp, init, **kw)
    assert a.extra["kernel"] == "sliced", a.extra
    assert made[-1].nuts_kernel(6) == "sliced"
    assert lib.mc_program_expr_jit(made[-1].handle) == 1, made[-1].kernel_note
    lib.mc_debug_expr_jit(0)
    try:
        _, _, b = m.nuts(lp, init, nuts_kernel="tape", **kw)
        assert lib.mc_program_expr_jit(made[-1].handle) == 0
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
        print(f"ops_transc NUTS chain {c}: trees identical for {same} of 12, depths "
              f"{list(b.trace['tree_depth'][c][:same])}")
        assert same >= 6, f"chain {c}: trees differ at iteration {same}"
    assert np.any(b.trace["tree_depth"] >= 2)


def test_sliced_mh_decisions_equal_the_tape(gpu, monkeypatch):
    """ops_transc on k_mh_sl (value only): the decisions of 40 iterations
    identical to the tape's (k_mh, interpreter)."""
    import mlx_mcmc_amd as m
    from mlx_mcmc_amd import _lib, _trace

    lib = _lib.load()
    lp, init = X.group_model("ops_transc")(W.ns_product())
    made = _capture_programs(monkeypatch)
    C = 8
    kw = dict(num_samples=40, proposal_scale=0.05, random_seed=6, num_chains=C,
              return_info=True, return_trace=True, initial_positions=_start("ops_transc", C, 4))
    _, _, a = m.metropolis_hastings(lp, init, **kw)
    # (the program that ran: on k_mh_sl, its expression terms compiled)
    assert len(made) == 1 and lib.mc_program_mh_sliced(made[0].handle) == 1, made[0].kernel_note
    assert lib.mc_program_expr_jit(made[0].handle) == 1, made[0].kernel_note
    lib.mc_debug_expr_jit(0)
    lib.mc_debug_mh_sliced(0)
    try:
        _, _, b = m.metropolis_hastings(lp, init, **kw)
        assert lib.mc_program_mh_sliced(made[1].handle) == 0
        assert lib.mc_program_expr_jit(made[1].handle) == 0
    finally:
        lib.mc_debug_mh_sliced(-1)
        lib.mc_debug_expr_jit(-1)
    acc = b.trace["accepted"].astype(bool)
    assert 0 < acc.sum() < acc.size, "mixed decisions"
    np.testing.assert_array_equal(a.trace["accepted"], b.trace["accepted"])
