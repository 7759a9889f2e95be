"""The per-chain diagonal mass matrix on the GPU (csrc/metric.h; k_hmc / k_nuts
with MET, mc_hmc_run_metric / mc_nuts_run_metric):

  1. a metric of ones reproduces the run without a metric bit for bit, on every
     instantiation family (waves per chain 1 / 4 / 8, LDS and global arena,
     expression terms compiled and interpreted);
  2. a fixed metric against the unchanged oracle run in the whitened
     coordinates q~ = q / sqrt(minv);
  3. the first window's update against the formula applied in f64 to the
     positions a second chain set stored;
  4. an adapted NUTS run is the same bits in one launch, in chunks that cut
     through a window, and with its chains split over two chain sets;
  5. adaptation finds the scales of a badly scaled Gaussian and shortens the
     trees.
"""
import ctypes

import numpy as np
import pytest

import workloads as W
from oracle import samplers as S

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------
def _diag_normal(ns, scales):
    scales = np.asarray(scales, np.float32)

    def log_prob(params):
        return ns.sum(ns.Normal(0, scales).log_prob(params["x"]))

    return log_prob


def _engine_run(prog, algo, C, q0, eps, *, metric, adapt=False, chunks=None, num_warmup,
                num_samples, chain_offset=0, seed=5, L=5, depth=5, adapt_step_size=True,
                trace=True):
    """One run at engine level: (samples [C, S, D], scalars, trace dict, chain set).
    metric: None (mc_*_run), or an inverse mass / "ones" (mc_*_run_metric)."""
    import torch
    from mlx_mcmc_amd import _engine

    cs = _engine.ChainSet(prog, C, q0, eps)
    if metric is not None:
        cs.set_metric(None if isinstance(metric, str) else metric)
    total = num_warmup + num_samples
    samples = torch.zeros((C, max(num_samples, 1), prog.D), dtype=torch.float32, device=cs.device)
    tr = _engine.make_trace(C, 0, total, cs.device) if trace else None
    cfg = dict(chain_offset=chain_offset, num_warmup=num_warmup, num_samples=num_samples,
               sample_begin=0, sample_capacity=num_samples, seed=seed, step_size=eps,
               target_accept=0.8 if algo == "hmc" else 0.65, adapt_step_size=adapt_step_size)
    if algo == "hmc":
        cfg["num_leapfrog_steps"] = L
    else:
        cfg["max_tree_depth"] = depth
    if metric is None:
        launch = cs.run_hmc if algo == "hmc" else cs.run_nuts
    else:
        f = cs.run_hmc_metric if algo == "hmc" else cs.run_nuts_metric
        launch = lambda **kw: f(adapt=adapt, **kw)  # noqa: E731
    for a, b in (chunks or [(0, total)]):
        launch(samples=samples, trace=tr, iter_begin=a, iter_count=b - a, **cfg)
    torch.cuda.synchronize()
    return samples.cpu().numpy(), cs.scalars(), (tr.numpy() if tr else None), cs


# ---------------------------------------------------------------------------
# 1. ones are the identity
# ---------------------------------------------------------------------------
def _identity_model(name):
    ns = W.ns_product()
    if name == "wpc1":        # D = 70: not a multiple of 4, above one wave's stride of 64
        return W.iso_normal(ns, 70), 1, 0.1
    if name == "wpc4":
        return W.hierarchical(ns, *W.SHAPES["small"]), 4, 0.01
    if name == "wpc8":
        return W.hierarchical(ns, 7, 20_000), 8, 0.002
    if name == "global":      # 5 * 3300 f32 > 64 KB: the HMC arena leaves LDS (NUTS's too)
        return W.iso_normal(ns, 3300), 4, 0.05
    return W.logistic_regression(ns), 1, 0.01   # "expr", "expr_interp": expression terms


@pytest.mark.parametrize("algo", ["hmc", "nuts"])
@pytest.mark.parametrize("name", ["wpc1", "wpc4", "wpc8", "global", "expr", "expr_interp"])
def test_ones_reproduce_the_run_without_a_metric(gpu, name, algo):
    from mlx_mcmc_amd import _lib, _trace

    (lp, init), wpc, eps = _identity_model(name)
    lib = _lib.load()
    if name == "expr_interp":
        lib.mc_debug_expr_jit(0)
    try:
        prog = _trace.compile_model(lp, init, slices=1)
        assert prog.waves_per_chain == wpc
        if name.startswith("expr"):
            assert prog.model.n_exprs > 0
            assert lib.mc_program_expr_jit(prog.handle) == (1 if name == "expr" else 0)
        ws = (lib.mc_hmc_workspace_bytes(prog.handle, 4) if algo == "hmc"
              else lib.mc_nuts_workspace_bytes(prog.handle, 4, 5))
        assert (ws > 0) == (name == "global")          # the arena in LDS, or not
        q0 = prog.layout.flatten(init)
        kw = dict(num_warmup=10, num_samples=10)
        base = _engine_run(prog, algo, 4, q0, eps, metric=None, **kw)
        ones = _engine_run(prog, algo, 4, q0, eps, metric="ones", **kw)
        adapt = _engine_run(prog, algo, 4, q0, eps, metric="ones", adapt=True, **kw)
    finally:
        lib.mc_debug_expr_jit(-1)
    assert np.all(np.isfinite(base[0])) and np.ptp(base[0]) > 0
    # the adapting run too: 10 warmup iterations are below the schedule's 20
    for run in (ones, adapt):
        assert run[0].tobytes() == base[0].tobytes()
        assert run[1].tobytes() == base[1].tobytes()
        for k, v in base[2].items():
            assert run[2][k].tobytes() == v.tobytes(), k
        assert np.all(run[3].inverse_mass().cpu().numpy() == 1)
        assert not run[3].metric_scalars()["n_updates"].any()


def test_metric_run_refuses_a_lane_resident_plan(gpu):
    """mc_*_run_metric on a program whose launches go to the lane-resident
    kernels: MC_ERR_UNSUPPORTED with a message, nothing launched."""
    from mlx_mcmc_amd import _engine, _lib, _trace

    lp, init = W.iso_normal(W.ns_product(), 70)
    prog = _trace.compile_model(lp, init)          # the automatic plan: one lane-resident slice
    assert prog.slice_kernel == "lanes" and prog.nuts_kernel(5) == "lanes"
    for algo in ("hmc", "nuts"):
        with pytest.raises(_lib.EngineError, match="chain-per-workgroup") as e:
            _engine_run(prog, algo, 2, prog.layout.flatten(init), 0.1, metric="ones",
                        num_warmup=2, num_samples=2)
        assert e.value.code == _lib.MC_ERR_UNSUPPORTED


# ---------------------------------------------------------------------------
# 2. a fixed metric against the oracle in whitened coordinates
# ---------------------------------------------------------------------------
def _whitened_case(name):
    """(product log_prob, oracle log_prob, start, minv dict, h_scale).  h_scale
    (tests/_near_tie.py): the magnitude of H's summands where H itself is a
    near-zero sum of them — the Gaussian's sum_j |log s_j| + D * 0.5 log(2 pi)
    of normalisers plus D for the quadratic and kinetic parts (about D / 2
    each); 0 for the hierarchical model, whose |H| ~ 1400 is the larger."""
    if name == "diag":
        scales = (10.0 ** (-2.0 * np.arange(10) / 9)).astype(np.float32)   # two decades
        start = {"x": (0.5 * scales * np.cos(np.arange(10))).astype(np.float32)}
        # a metric near the scales, not on them (the identity in disguise otherwise)
        minv = {"x": (scales * (1.0 + 0.3 * np.sin(np.arange(10)))).astype(np.float32) ** 2}
        h_scale = float(np.abs(np.log(scales)).sum() + 10 * 0.5 * np.log(2 * np.pi) + 10)
        return (_diag_normal(W.ns_product(), scales), _diag_normal(W.ns_oracle(), scales), start,
                minv, h_scale)
    plp, init = W.hierarchical(W.ns_product(), *W.SHAPES["small"])
    olp, _ = W.hierarchical(W.ns_oracle(), *W.SHAPES["small"])
    G = W.SHAPES["small"][0]
    minv = {"mu": np.float32(0.5), "tau": np.float32(0.4), "sigma": np.float32(5e-4),
            "theta": np.full(G, 7e-3, np.float32)}
    return plp, olp, init, minv, 0.0


def _whiten(olp, start, minv):
    """The oracle's problem in q~ = q / s, s = sqrt(minv): log_prob(s * q~) from q0 / s."""
    import torch

    s = {k: np.sqrt(np.asarray(v, np.float32)) for k, v in minv.items()}
    st = {k: torch.as_tensor(v) for k, v in s.items()}
    wlp = lambda p: olp({k: st[k] * p[k] for k in p})  # noqa: E731
    wstart = {k: (np.asarray(v, np.float32) / s[k]).astype(np.float32) for k, v in start.items()}
    flat_s = np.concatenate([np.broadcast_to(s[k], np.shape(start[k])).ravel() for k in start])
    return wlp, wstart, flat_s.astype(np.float32)


@pytest.mark.parametrize("name", ["diag", "small"])
def test_fixed_metric_hmc_matches_whitened_oracle(gpu, name):
    """Same seed and chain: accept decisions equal up to the first proven
    near-tie (tests/_near_tie.py), ratios within rtol 1e-3 / atol 2e-3, step
    sizes identical, positions s * q~ within rtol 1e-3 before the tie."""
    import mlx_mcmc_amd as m
    from _near_tie import compare_trace, log_u

    plp, olp, start, minv, h_scale = _whitened_case(name)
    wlp, wstart, s = _whiten(olp, start, minv)
    # step sizes (and, for the hierarchical model, a seed) at which the whitened
    # oracle's decisions are a mix, about three in four accepted, and the
    # rejected trajectories are ordinary ones (log ratios down to -10): one
    # that runs into tau or sigma near 0 ends at a log ratio of -1e2 .. -1e15,
    # chaotic in its last digits
    n_w, n_s = 20, 20
    eps, seed = (1.2, 3) if name == "diag" else (0.35, 4)
    samples, _, info = m.hmc(plp, start, num_samples=n_s, num_warmup=n_w, step_size=eps,
                             num_leapfrog_steps=5, key=m.random.key(seed), progress=False,
                             return_info=True, return_trace=True, inverse_mass_matrix=minv)
    assert info.extra["kernel"] == "unsliced" and "tape" in info.extra["kernel_note"]
    ref = S.hmc(wlp, wstart, num_samples=n_s, num_warmup=n_w, step_size=eps,
                num_leapfrog_steps=5, seed=seed)
    tr = info.trace
    gpu_c = {"accepted": tr["accepted"][0].astype(bool), "ratio": tr["accept_stat"][0],
             "step_size": tr["step_size"][0], "energy": tr["energy"][0]}
    ref_c = {k: np.asarray(ref.trace[k]) for k in ("accepted", "ratio", "step_size", "energy")}
    ref_c["log_u"] = log_u(seed, 0, n_w + n_s)
    upto = compare_trace(gpu_c, ref_c, f"metric hmc {name}", verbose=True,
                         h_scale=h_scale)
    assert upto >= 30, f"decisions diverged at iteration {upto}"
    assert 0 < ref_c["accepted"][:upto].mean() < 1          # a mix of decisions
    dev = np.abs(gpu_c["ratio"][:upto] - ref_c["ratio"][:upto])
    print(f"metric hmc {name}: max |ratio diff| {dev.max():.3g} over {upto} iterations")
    np.testing.assert_allclose(gpu_c["ratio"][:upto], ref_c["ratio"][:upto], rtol=1e-3, atol=2e-3)
    k = max(0, upto - n_w)
    flat = np.concatenate([np.reshape(samples[n], (n_s, -1)) for n in start], axis=1)
    np.testing.assert_allclose(flat[:k], s * ref.samples[:k], rtol=1e-3, atol=1e-5)
    assert k >= 10


@pytest.mark.parametrize("name", ["diag", "small"])
def test_fixed_metric_nuts_matches_whitened_oracle(gpu, name):
    """Same seed and chain, fixed step size: tree depths and leaf counts equal
    up to the first flip, which must be a near-tie the oracle proves (a slice /
    divergence gap or a relative U-turn dot within the bounds of
    tests/test_gpu_nuts_trace.py); positions within rtol 1e-3 before it, and
    alpha within rtol 1e-4 on the Gaussian.  The hierarchical model's H ~ 1400
    has an f32 ulp of 1.2e-4, and a leaf's alpha = exp(H0 - H') moves by that
    much, relatively, per ulp of H: rtol 1e-4 is below the format's resolution
    there.  The whitened oracle rounds s * q~ once more and sums the kinetic
    energy in another order; the measured maximum deviation is 3.1e-4 (2.5 ulp
    of H), gated at four times that, 1.24e-3 — about 10 ulp of H, the order of
    the 8 ulp tests/_near_tie.py allows two correct f32 sums of H."""
    import mlx_mcmc_amd as m

    plp, olp, start, minv, h_scale = _whitened_case(name)
    wlp, wstart, s = _whiten(olp, start, minv)
    n_w, n_s, seed = 10, 20, 11
    eps = 0.3 if name == "diag" else 0.15
    kw = dict(num_samples=n_s, num_warmup=n_w, step_size=eps, max_tree_depth=5,
              adapt_step_size=False)
    samples, _, info = m.nuts(plp, start, key=m.random.key(seed), progress=False,
                              return_info=True, return_trace=True, inverse_mass_matrix=minv, **kw)
    assert info.extra["kernel"] == "tape"
    ref = S.nuts(wlp, wstart, seed=seed, **kw)
    rt = {k: np.asarray(v) for k, v in ref.trace.items()}
    tr = info.trace
    n, D = n_w + n_s, s.size
    gd, gl = tr["tree_depth"][0], tr["n_leapfrog"][0]
    same = next((i for i in range(n) if gd[i] != rt["depth"][i] or gl[i] != rt["leaves"][i]), n)
    print(f"metric nuts {name}: trees identical for {same} of {n} iterations, depths "
          f"{sorted(set(rt['depth'][:same].tolist()))}")
    if same < n:
        i = same
        ulp = float(np.spacing(np.float32(max(abs(rt["energy"][i]) + D, h_scale))))
        drift = abs(float(tr["energy"][0][i]) - rt["energy"][i])
        tie, tie_dot = 8 * ulp + 4 * drift, 1e-5 + 4 * drift / max(abs(rt["energy"][i]), 1.0)
        assert (rt["slice_gap"][i] <= tie or rt["div_gap"][i] <= tie
                or rt["uturn_margin"][i] <= tie_dot), \
            (f"trees differ at iteration {i} with no near-tie: slice {rt['slice_gap'][i]:.3g}, "
             f"divergence {rt['div_gap'][i]:.3g}, U-turn {rt['uturn_margin'][i]:.3g}; "
             f"bounds {tie:.3g} / {tie_dot:.3g}")
    assert same >= 15, f"trees diverged at iteration {same}"
    assert rt["depth"][:same].max() >= 2                    # real trees
    dev = np.abs(tr["accept_stat"][0][:same] / rt["alpha"][:same] - 1)
    print(f"metric nuts {name}: max relative alpha deviation {dev.max():.3g}")
    np.testing.assert_allclose(tr["accept_stat"][0][:same], rt["alpha"][:same],
                               rtol=1e-4 if name == "diag" else 1.24e-3, atol=1e-6)
    k = max(0, same - n_w)
    flat = np.concatenate([np.reshape(samples[nm], (n_s, -1)) for nm in start], axis=1)
    np.testing.assert_allclose(flat[:k], s * ref.samples[:k], rtol=1e-3, atol=1e-5)


# ---------------------------------------------------------------------------
# 3. adaptation arithmetic
# ---------------------------------------------------------------------------
def test_first_window_update_matches_the_formula(gpu):
    """HMC, fixed step size, W = 100: the only window is [15, 90).  Run A adapts
    and is launched exactly through iteration 89; run B (num_warmup = 0, a
    metric of ones) stores the same iterations as samples — draws are a pure
    function of the iteration and A's metric is ones until the update."""
    from mlx_mcmc_amd import _lib, _trace

    D, C, Wm = 7, 3, 100
    ends = (ctypes.c_int64 * 8)()
    assert _lib.load().mc_metric_schedule(Wm, ends, 8) == 1 and ends[0] == 90
    lp, init = W.illcond_normal(W.ns_product(), D)
    prog = _trace.compile_model(lp, init, slices=1)
    rng = np.random.default_rng(1)
    q0 = (W.illcond_scales(D) * rng.normal(size=(C, D))).astype(np.float32)
    common = dict(seed=9, L=5, adapt_step_size=False, trace=False)
    _, _, _, A = _engine_run(prog, "hmc", C, q0, 0.02, metric="ones", adapt=True,
                             chunks=[(0, 40), (40, 90)], num_warmup=Wm, num_samples=0, **common)
    sB, _, _, B = _engine_run(prog, "hmc", C, q0, 0.02, metric="ones", chunks=[(0, 90)],
                              num_warmup=0, num_samples=90, **common)
    assert A.positions().cpu().numpy().tobytes() == B.positions().cpu().numpy().tobytes()
    x = sB[:, 15:90, :].astype(np.float64)                      # the window's 75 positions
    n = x.shape[1]
    var = x.var(axis=1, ddof=1)
    assert np.all(var > 0)
    want = (n / (n + 5.0)) * var + 1e-3 * (5.0 / (n + 5.0))
    got = A.inverse_mass().cpu().numpy()
    np.testing.assert_allclose(got, want, rtol=1e-4)
    np.testing.assert_allclose(A._metric_section("msqrt").cpu().numpy(), 1 / np.sqrt(want),
                               rtol=1e-4)
    ms = A.metric_scalars()
    assert ms["n_updates"].tolist() == [1] * C and ms["n_window"].tolist() == [0] * C
    assert not A._metric_section("mean").cpu().numpy().any()    # the accumulator reset
    assert not A._metric_section("m2").cpu().numpy().any()
    # B never adapted
    assert np.all(B.inverse_mass().cpu().numpy() == 1)


# ---------------------------------------------------------------------------
# 4. launch and chain splitting
# ---------------------------------------------------------------------------
def test_adapted_nuts_is_invariant_to_launch_and_chain_splits(gpu):
    """W = 150 (one window, [75, 100)), 20 samples, D = 10, 4 chains, step size
    and metric both adapting: one launch, chunks that cut through the window,
    and chains 2 + 2 with chain_offset give the same bits."""
    from mlx_mcmc_amd import _trace

    D, C = 10, 4
    lp, init = W.illcond_normal(W.ns_product(), D)
    prog = _trace.compile_model(lp, init, slices=1)
    rng = np.random.default_rng(2)
    q0 = (W.illcond_scales(D) * rng.normal(size=(C, D))).astype(np.float32)
    kw = dict(metric="ones", adapt=True, num_warmup=150, num_samples=20, depth=6, seed=21)
    one = _engine_run(prog, "nuts", C, q0, 0.05, **kw)
    cut = _engine_run(prog, "nuts", C, q0, 0.05,
                      chunks=[(0, 80), (80, 97), (97, 100), (100, 155), (155, 170)], **kw)
    halves = [_engine_run(prog, "nuts", 2, q0[o:o + 2], 0.05, chain_offset=o, **kw)
              for o in (0, 2)]

    def parts(run):
        return [run[0], run[1], run[3].inverse_mass().cpu().numpy(),
                run[3]._metric_section("msqrt").cpu().numpy(), run[3].metric_scalars(),
                run[2]["tree_depth"], run[2]["accept_stat"], run[2]["step_size"]]

    ref = parts(one)
    assert ref[4]["n_updates"].tolist() == [1] * C and ref[4]["da_origin"].tolist() == [100] * C
    assert np.all(ref[2] != 1) and np.all(np.isfinite(ref[0]))
    # the metric did its work: the adapted scales order as the model's do
    assert np.all(ref[2][:, 0] > ref[2][:, -1])
    for a, b in zip(ref, parts(cut)):
        assert a.tobytes() == b.tobytes()
    split = [np.concatenate([x, y]) for x, y in zip(parts(halves[0]), parts(halves[1]))]
    for a, b in zip(ref, split):
        assert a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------
# 5. it works
# ---------------------------------------------------------------------------
def test_adaptation_finds_the_scales_and_shortens_the_trees(gpu):
    """Diagonal Gaussian, D = 16, scales over 1.5 decades, NUTS, W = 1000, 8
    chains, 500 samples.  The last window holds 500 draws: the relative sd of
    its variance estimate is sqrt(2 / ESS), 0.14 even at ESS = 100, so a factor
    of 2 is five sigma.  The pooled posterior sd of 4000 draws is within 10 %
    of the scale (1 / sqrt(2 ESS) ~ 2 % at ESS = 1500)."""
    import mlx_mcmc_amd as m

    D, C = 16, 8
    scales = (10.0 ** (-1.5 * np.arange(D) / (D - 1))).astype(np.float32)
    lp = _diag_normal(W.ns_product(), scales)
    init = {"x": np.zeros(D, np.float32)}
    kw = dict(num_samples=500, num_warmup=1000, num_chains=C, key=m.random.key(17),
              progress=False, return_info=True)
    s_ad, _, ad = m.nuts(lp, init, adapt_mass_matrix=True, **kw)
    s_id, _, ident = m.nuts(lp, init, nuts_kernel="tape", **kw)
    assert ad.extra["kernel"] == "tape" and "tape" in ad.extra["kernel_note"]
    assert "inverse_mass_matrix" not in ident.extra
    minv = ad.extra["inverse_mass_matrix"]
    assert minv.shape == (C, D) and ad.extra["metric_updates"].tolist() == [5] * C
    ratio = minv / scales.astype(np.float64) ** 2
    print(f"minv / s^2 in [{ratio.min():.3f}, {ratio.max():.3f}]; mean depth adapted "
          f"{ad.mean_tree_depth.mean():.2f}, identity {ident.mean_tree_depth.mean():.2f}; "
          f"step size adapted {ad.step_size.mean():.3f}, identity {ident.step_size.mean():.4f}")
    assert np.all(ratio >= 0.5) and np.all(ratio <= 2.0)
    sd = s_ad["x"].reshape(-1, D).std(axis=0)
    np.testing.assert_allclose(sd, scales, rtol=0.10)
    assert ad.mean_tree_depth.mean() < ident.mean_tree_depth.mean()
    # a second run starts from the final metric
    _, _, again = m.nuts(lp, init, num_samples=20, num_warmup=20, num_chains=C,
                         key=m.random.key(18), progress=False, return_info=True,
                         inverse_mass_matrix=minv)
    np.testing.assert_array_equal(again.extra["inverse_mass_matrix"], minv)
    assert again.extra["metric_updates"].tolist() == [0] * C
