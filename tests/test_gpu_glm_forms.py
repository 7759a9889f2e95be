"""The design-matrix gradient path (csrc/glm.h, glm_wide.h, glm_softmax.h,
run_glm.hip) beyond the one form of tests/_glm.py: every operand branch and
prior of tests/_glm_forms.py, the chunk loop of mc_logp_grad / mc_state_init,
saturated inputs, a poisoned chain beside clean ones, observations outside the
support, and hmc() against the oracle on two non-default forms.

The gate everywhere is that of tests/test_gpu_glm.py: |lp - ref| <= 1e-5 max(1,
|ref|), gradients rtol 2e-4, atol 2e-5 max(1, max |g|), against the float64
closed form; tests/test_glm_forms_reference.py holds the float32 closed form to
it at every input used here."""
import numpy as np
import pytest

import _glm
import _glm_forms as F
import _glm_softmax as G
from _near_tie import compare_trace, log_u
from oracle import samplers as S

pytestmark = pytest.mark.gpu

KERNEL = {False: "k_glm_grad /", True: "k_glm_grad_wide /"}


def compiled(f, d, S_, wide=False):
    from mlx_mcmc_amd import _trace

    lp_fn, init = F.model(F.ns_product(), f, d)
    prog = _trace.compile_model(lp_fn, init, slices=S_, glm_kernel="wide" if wide else "auto")
    assert prog.slice_kernel == "glm" and KERNEL[wide] in prog.kernel_note
    assert prog.D == F.layout(f)[1]
    return prog


def evaluate(prog, q):
    """logp_grad twice: the same bytes; as NumPy."""
    from mlx_mcmc_amd import _engine

    lp, g = (t.cpu().numpy() for t in _engine.logp_grad(prog, q))
    lp2, g2 = (t.cpu().numpy() for t in _engine.logp_grad(prog, q))
    assert lp.tobytes() == lp2.tobytes() and g.tobytes() == g2.tobytes()
    return lp, g


# ---- a. the form matrix ------------------------------------------------------------
@pytest.mark.parametrize("N,P,C,S_", F.SHAPES + [F.WIDE])
@pytest.mark.parametrize("family,name", F.CASES)
def test_every_form_matches_f64(gpu, family, name, N, P, C, S_):
    """No intercept, a constant one, one declared after a sliced beta; a constant,
    raw and exp scale; the offset on and off on every family; every prior dist,
    transform, weight and range of plan_glm.hip's table (the forms of
    tests/_glm_forms.py), on k_glm_grad and at P = 129 on k_glm_grad_wide.  The
    float32 closed form: worst lp 0.025 of the bound, worst gradient 0.008."""
    wide = (N, P, C, S_) == F.WIDE
    f, d = F.form(name, family, P), F.data(family, N, P)
    prog = compiled(f, d, S_, wide)
    assert prog.glm_slices(C) == S_
    q = F.points(f, C)
    lp, g = evaluate(prog, q)
    F.assert_gate(lp, g, *F.closed_form(f, d, q), what=f"{family} {name} {N}x{P} C={C} S={S_}")
    if name == "sliced":  # the parameter in no term
        assert np.all(g[:, F.layout(f)[0]["u"][0]] == 0.0)


# ---- b. the chunk loop of run_glm.hip glm_eval ------------------------------------------
# plan: (kind, N, P, K or family, slices, C, the first chunk's chains, a row inside it)
CHUNK_PLANS = {
    "scalar-33x3": ("glm", 33, 3, "normal", 1, 290, 256, 100),
    "scalar-97x33-S3": ("glm", 97, 33, "poisson", 3, 290, 256, 100),
    "wide-33x129": ("wide", 33, 129, "bernoulli", 1, 290, 256, 100),
    "softmax-K32": ("softmax", 33, 3, 32, 1, 19, 8, 3),
    "softmax-K17-no-intercept": ("softmax", 33, 3, 17, 1, 19, 8, 3),
    "softmax-K3": ("softmax", 33, 5, 3, 1, 70, 64, 5),
}


@pytest.mark.parametrize("plan", list(CHUNK_PLANS))
def test_chunked_evaluation(gpu, plan):
    """mc_logp_grad runs kGlmScratchBlocks = 8 gradient blocks at a time: 256
    chains, 8 CPB on a softmax plan.  290 chains are two chunks, the second one
    full and one ragged block; softmax at Kp = 32 runs 19 chains as 8 + 8 + 3 and
    at Kp = 4 (CPB = 8) 70 chains as 64 + 6.  Every row is inside the gate (the
    float32 closed form: worst lp 0.041 of the bound, worst gradient 0.002), and a
    row's bytes do not depend on the rows before it: the call on q[a:] equals the
    tail of the call on q, for a at the chunk boundary and inside the chunk."""
    from mlx_mcmc_amd import _engine, _trace

    kind, N, P, fam, S_, C, chunk, inside = CHUNK_PLANS[plan]
    if kind == "softmax":
        icpt = "no-intercept" not in plan
        d = G.data(N, P, fam)
        prog = _trace.compile_model(*G.model(G.ns_product(), d, icpt), slices=S_)
        assert prog.slice_kernel == "glm" and "k_glm_softmax_grad" in prog.kernel_note
        q = np.random.default_rng(5).normal(size=(C, prog.D)).astype(np.float32)
        ref = G.closed_form(d, q, icpt)
    else:
        f, d = F.form("sliced", fam, P), F.data(fam, N, P)
        prog = compiled(f, d, S_, kind == "wide")
        q = F.points(f, C)
        ref = F.closed_form(f, d, q)
    assert {prog.glm_slices(c) for c in (1, C - chunk, chunk, C)} == {S_}
    lp, g = evaluate(prog, q)
    F.assert_gate(lp, g, *ref, what=plan)
    for a in (chunk, inside):
        tl, tg = (t.cpu().numpy() for t in _engine.logp_grad(prog, q[a:]))
        assert lp[a:].tobytes() == tl.tobytes(), f"lp of rows {a}: differs from the call on q[{a}:]"
        assert g[a:].tobytes() == tg.tobytes(), f"gradient of rows {a}: differs"


@pytest.mark.parametrize("sampler", ["hmc", "hmc-softmax", "nuts"])
def test_state_init_in_chunks_through_the_samplers(gpu, sampler):
    """mc_state_init takes the same chunk loop: 290 chains in one call and as 256
    + 34 through chain_offset (softmax K = 32: 19 as 8 + 11) give the same bytes
    per global chain, as tests/test_gpu_glm.py
    test_chains_do_not_depend_on_the_split has it for one chunk."""
    import mlx_mcmc_amd as m

    if sampler == "hmc-softmax":
        d = G.data(33, 3, 32)
        lp_fn, init = G.model(G.ns_product(), d)
        C, first = 19, 8
    else:
        f, d = F.form("sliced", "poisson", 3), F.data("poisson", 33, 3)
        lp_fn, init = F.model(F.ns_product(), f, d)
        C, first = 290, 256
    kw = dict(num_samples=3, num_warmup=3, step_size=0.05, key=m.random.key(9), progress=False,
              num_slices=1)
    if sampler == "nuts":
        kw.update(nuts_kernel="glm", max_tree_depth=3)
    else:
        kw.update(num_leapfrog_steps=2)

    def run(n, off=0):
        s, _ = (m.nuts if sampler == "nuts" else m.hmc)(lp_fn, init, num_chains=n, chain_offset=off,
                                                          **kw)
        return np.concatenate([np.asarray(s[k]).reshape(n, 3, -1) for k in init], axis=2)

    whole = run(C)
    assert np.isfinite(whole).all() and np.ptp(whole[:, :, 0]) > 0
    split = np.concatenate([run(first), run(C - first, off=first)])
    assert whole.tobytes() == split.tobytes()


# ---- c. saturation -------------------------------------------------------------------
@pytest.mark.parametrize("N,P,C,S_", F.SHAPES)
@pytest.mark.parametrize("kind,level", [("bernoulli", 100.0), ("poisson", 20.0), ("exp", -4.0),
                                        ("exp", 4.0), ("raw", 0.05), ("raw", 20.0)])
def test_saturated_inputs_match_f64(gpu, kind, level, N, P, C, S_):
    """ex_softplus / ex_sigmoid at |eta| up to 100 in both signs, ex_exp at eta up
    to 20, and a Normal scale of e^-4, e^4, 0.05 and 20.  The float32 closed form:
    worst lp 0.009 of the bound at |eta| = 100, 0.165 at Poisson eta = 20 (the
    largest of 20, 10, 5: 0.035 at 10, 0.017 at 5), at most 0.022 on the four
    Normal scales; worst gradient 0.010."""
    f, d, q = F.saturated(kind, level, N, P, C)
    if kind in ("bernoulli", "poisson"):
        eta = q[:, :1].astype(np.float64) + q[:, 1:1 + P].astype(np.float64) @ d.X.T
        assert abs((np.abs(eta) if kind == "bernoulli" else eta).max() - level) < 1e-3 * level
        if kind == "bernoulli":
            for y in (0, 1):
                assert eta[:, d.y == y].max() > 50 and eta[:, d.y == y].min() < -50
    prog = compiled(f, d, S_)
    lp, g = evaluate(prog, q)
    F.assert_gate(lp, g, *F.closed_form(f, d, q), what=f"{kind} {level:g} {N}x{P} C={C} S={S_}")


# ---- d. a poisoned chain ---------------------------------------------------------------
POISON_PLANS = {
    "scalar-33x3": ("glm", 33, 3, "poisson", 1),
    "scalar-97x33-S3": ("glm", 97, 33, "normal", 3),
    "wide-33x129": ("wide", 33, 129, "bernoulli", 1),
    "softmax-K3": ("softmax", 33, 5, 3, 1),
    "softmax-K32": ("softmax", 33, 3, 32, 1),
}


@pytest.mark.parametrize("poison", [np.inf, np.nan, 1e30])
@pytest.mark.parametrize("plan", list(POISON_PLANS))
def test_a_poisoned_chain_does_not_leak(gpu, plan, poison):
    """"A chain is one MFMA column and columns never mix" (csrc/glm.h) with a
    column that is not finite: chain 5 of 33 (on softmax K = 3 one of the 8
    chains of gradient block 0, its classes among the ds_swizzle exchanges of the
    others') holds inf, NaN or 1e30 in every coefficient, so 0 * inf = NaN lands
    in its zero-padded operand rows.  Every other chain's log density and
    gradient keep the bytes of the clean call."""
    from mlx_mcmc_amd import _trace

    kind, N, P, fam, S_ = POISON_PLANS[plan]
    C, bad = 33, 5
    if kind == "softmax":
        d = G.data(N, P, fam)
        prog = _trace.compile_model(*G.model(G.ns_product(), d), slices=S_)
        assert "k_glm_softmax_grad" in prog.kernel_note
        q = np.random.default_rng(5).normal(size=(C, prog.D)).astype(np.float32)
    else:
        f, d = F.form("sliced", fam, P), F.data(fam, N, P)
        prog = compiled(f, d, S_, kind == "wide")
        q = F.points(f, C)
    lp, g = evaluate(prog, q)
    assert np.isfinite(lp).all() and np.isfinite(g).all()
    qp = q.copy()
    qp[bad] = poison
    plp, pg = evaluate(prog, qp)
    keep = np.arange(C) != bad
    assert plp[keep].tobytes() == lp[keep].tobytes()
    assert pg[keep].tobytes() == g[keep].tobytes()
    if not np.isfinite(poison):
        assert not np.isfinite(plp[bad])


# ---- e. observations outside the support -------------------------------------------------
@pytest.mark.parametrize("family,bad", [("bernoulli", 0.5), ("poisson", 2.5), ("poisson", -1.0)])
def test_an_observation_outside_the_support(gpu, family, bad):
    """k_glm_grad gives such a row log p = -inf and no residual (rr = 0): every
    chain's log density is -inf, and the gradient is the closed form's without
    that row's residual, inside the gate."""
    N, P, C, S_ = F.SHAPES[1]
    f, d = F.form("plain", family, P), _glm.data(family, N, P)
    d.y[40] = bad
    prog = compiled(f, d, S_)
    q = F.points(f, C)
    lp, g = evaluate(prog, q)
    rlp, rg = F.closed_form(f, d, q)
    assert np.all(rlp == -np.inf) and np.all(lp == -np.inf)
    print(f"{family} y = {bad}: gradient error {np.abs(g - rg).max():.2e} "
          f"(max |g| {np.abs(rg).max():.2e})")
    np.testing.assert_allclose(g, rg, rtol=2e-4, atol=2e-5 * max(1.0, np.abs(rg).max()))


# ---- f. hmc() against the oracle on non-default forms --------------------------------------
@pytest.mark.parametrize("S_", [1, 3])
@pytest.mark.parametrize("family,name,eps,seed", [("bernoulli", "sliced", 0.3, 3),
                                                  ("normal", "rawscale", 0.04, 11)])
def test_hmc_matches_oracle(gpu, family, name, eps, seed, S_):
    """As tests/test_gpu_glm.py test_hmc_matches_oracle, on a sliced beta with
    the intercept declared after it and a parameter in no term (Bernoulli), and
    on a raw scale under a HalfNormal prior (Normal).  The step sizes come from
    the oracle's chains alone, on the CPU.  Bernoulli at 0.3: its four chains
    accept 26, 20, 25 and 24 of their 30 iterations, no log ratio below -2.3 (0.2
    accepts 110 of 120; at 0.5 the log ratios reach -233: past leapfrog's
    stability limit).  Normal at 0.04: 28, 30, 30 and 28 of 30, no log ratio
    below -1.1 (at 0.06 they reach -203)."""
    import mlx_mcmc_amd as m

    n = 30
    f, d = F.form(name, family, 5), F.data(family, 97, 5)
    lp_fn, init = F.model(F.ns_product(), f, d)
    olp, _ = F.model(F.ns_torch(), f, d)
    kw = dict(num_samples=15, num_warmup=15, step_size=eps, num_leapfrog_steps=10)
    _, _, info = m.hmc(lp_fn, init, key=m.random.key(seed), num_chains=4, progress=False,
                       return_info=True, return_trace=True, num_slices=S_, **kw)
    assert info.extra["kernel"] == "glm" and info.extra["glm_slices"] == S_
    tr, total, acc = info.trace, 0, []
    for c in range(4):
        ref = S.hmc(olp, init, seed=seed, chain=c, **kw)
        gpu_c = {"accepted": tr["accepted"][c][:n], "ratio": tr["accept_stat"][c][:n],
                 "step_size": tr["step_size"][c][:n], "energy": tr["energy"][c][:n]}
        ref_c = {k: np.asarray(ref.trace[k])[:n] for k in ("accepted", "ratio", "step_size",
                                                            "energy")}
        ref_c["log_u"] = log_u(seed, c, n)
        same = compare_trace(gpu_c, ref_c, f"{family} {name} chain {c}", verbose=True)
        assert same >= 5, f"{family} {name} chain {c}: compared only {same}"
        total += same
        acc += list(ref_c["accepted"])
    assert total >= 0.7 * 4 * n, f"{family} {name}: only {total} of {4 * n} iterations compared"
    assert any(acc) and not all(acc)
