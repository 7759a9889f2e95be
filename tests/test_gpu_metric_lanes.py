"""The diagonal mass matrix on the lane-resident NUTS kernel (k_nuts_lr with MET,
csrc/nuts_lanes.h; mc_nuts_run_metric_lanes, ``nuts(nuts_kernel="lanes")``) —
the twins of tests/test_gpu_metric.py on the opt-in path:

  1. a metric of ones reproduces mc_nuts_run bit for bit on every instantiation
     (one, two and four register slots, the replicated-lane plan, with and
     without the draw wave);
  2. a fixed metric against the unchanged oracle in whitened coordinates;
  3. the first window's update against the formula in f64;
  4. an adapted run is the same bits in one launch, in chunks that cut through
     a window, and with its chains split over two chain sets;
  5. adaptation finds the scales and shortens the trees;
  6. routing: what "lanes" accepts, refuses, and leaves alone.

``nuts_kernel="lanes"`` is accepted with a mass matrix only: without one it stays
the ValueError that tests/test_tracer.py::test_nuts_kernel_choice_is_checked pins
(test 6 checks that, and the identity run of test 5 takes the default "auto",
which runs the same kernel).
"""
import ctypes

import numpy as np
import pytest

import workloads as W
from oracle import samplers as S

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------
# helpers (tests/test_gpu_metric.py's, on the lanes entry point)
# ---------------------------------------------------------------------------
def _diag_normal(ns, scales):
    scales = np.asarray(scales, np.float32)

    def log_prob(params):
        return ns.sum(ns.Normal(0, scales).log_prob(params["x"]))

    return log_prob


def _decades(D, decades):
    return (10.0 ** (-decades * np.arange(D) / (D - 1))).astype(np.float32)


def _engine_run(prog, C, q0, eps, *, metric, adapt=False, chunks=None, num_warmup, num_samples,
                chain_offset=0, seed=5, depth=5, adapt_step_size=True, trace=True):
    """One NUTS run at engine level: (samples [C, S, D], scalars, trace dict,
    chain set).  metric: None (mc_nuts_run) or "ones" (mc_nuts_run_metric_lanes)."""
    import torch
    from mlx_mcmc_amd import _engine

    cs = _engine.ChainSet(prog, C, q0, eps)
    if metric is not None:
        cs.set_metric(None)
    total = num_warmup + num_samples
    samples = torch.zeros((C, max(num_samples, 1), prog.D), dtype=torch.float32, device=cs.device)
    tr = _engine.make_trace(C, 0, total, cs.device) if trace else None
    cfg = dict(chain_offset=chain_offset, num_warmup=num_warmup, num_samples=num_samples,
               sample_begin=0, sample_capacity=num_samples, seed=seed, step_size=eps,
               target_accept=0.65, adapt_step_size=adapt_step_size, max_tree_depth=depth)
    if metric is None:
        launch = cs.run_nuts
    else:
        launch = lambda **kw: cs.run_nuts_metric_lanes(adapt=adapt, **kw)  # noqa: E731
    for a, b in (chunks or [(0, total)]):
        launch(samples=samples, trace=tr, iter_begin=a, iter_count=b - a, **cfg)
    torch.cuda.synchronize()
    return samples.cpu().numpy(), cs.scalars(), (tr.numpy() if tr else None), cs


# ---------------------------------------------------------------------------
# 1. ones are the identity, bit for bit
# ---------------------------------------------------------------------------
def _identity_model(name):
    """((log_prob, init), register slots, step size, max_tree_depth).  Step
    sizes below twice the smallest scale, so the trees are ordinary ones."""
    ns = W.ns_product()
    if name == "direct_rs1":      # a direct term with constant loc and scale; 32 < D <= 64:
        return W.iso_normal(ns, 50), 1, 0.1, 5    # one slot, one lane per parameter
    if name == "direct_rs2":      # D = 70 plans two slots (the second in lanes 0..5)
        return W.iso_normal(ns, 70), 2, 0.1, 5
    if name == "dscale_rs2":      # a data-scale term, the second slot in lanes 0..35
        return W.illcond_normal(ns, 100), 2, 0.02, 5
    if name == "dscale_rs4":
        s = _decades(200, 1.5)
        return (_diag_normal(ns, s), {"x": np.zeros(200, np.float32)}), 4, 0.02, 5
    if name == "replicated":      # D <= 32: the planner may deal a parameter to several lanes
        s = _decades(10, 2.0)
        return (_diag_normal(ns, s), {"x": (0.5 * s).astype(np.float32)}), 1, 0.005, 5
    # one wave per chain: the draw wave is off above depth 12.  At 0.05 a tree
    # turns after ~pi / 0.05 = 63 leaves along the widest scale: depth 6 or 7
    return W.illcond_normal(ns, 100), 2, 0.05, 13


@pytest.mark.parametrize("name", ["direct_rs1", "direct_rs2", "dscale_rs2", "dscale_rs4",
                                  "replicated", "one_wave"])
def test_ones_reproduce_the_run_without_a_metric(gpu, name):
    from mlx_mcmc_amd import _lib, _trace

    (lp, init), rs, eps, depth = _identity_model(name)
    lib = _lib.load()
    prog = _trace.compile_model(lp, init)             # the automatic plan
    assert prog.nuts_kernel(depth) == "lanes" and prog.nuts_register_only(depth)
    assert lib.mc_program_nuts_metric_lanes(prog.handle, depth) == 1
    assert lib.mc_program_lane_slots(prog.handle) == rs
    assert (lib.mc_program_lane_rep(prog.handle) > 1) == (name == "replicated")
    q0 = prog.layout.flatten(init)
    kw = dict(num_warmup=10, num_samples=10, depth=depth)
    base = _engine_run(prog, 4, q0, eps, metric=None, **kw)
    ones = _engine_run(prog, 4, q0, eps, metric="ones", **kw)
    adapt = _engine_run(prog, 4, q0, eps, metric="ones", adapt=True, **kw)
    assert np.all(np.isfinite(base[0])) and np.ptp(base[0]) > 0
    print(f"{name}: tree depths {sorted(set(base[2]['tree_depth'].ravel().tolist()))}")
    assert base[2]["tree_depth"].max() >= 2            # real trees
    # the adapting run too: 10 warmup iterations are below the schedule's 20
    for run in (ones, adapt):
        assert run[0].tobytes() == base[0].tobytes()
        assert run[1].tobytes() == base[1].tobytes()
        for k, v in base[2].items():
            assert run[2][k].tobytes() == v.tobytes(), k
        assert np.all(run[3].inverse_mass().cpu().numpy() == 1)
        assert not run[3].metric_scalars()["n_updates"].any()


# ---------------------------------------------------------------------------
# 2. a fixed metric against the oracle in whitened coordinates
# ---------------------------------------------------------------------------
def _whitened_case(name):
    """(product log_prob, oracle log_prob, start, minv dict, h_scale, eps): the
    "diag" case of tests/test_gpu_metric.py, and the bench model at D = 100
    built the same way (h_scale: sum_j |log s_j| + D * 0.5 log(2 pi) of
    normalisers plus D for the quadratic and kinetic parts).  Step size 0.3 on
    "diag"; 0.45 at D = 100, where the whitened oracle alone gives every tree
    depth 4 at 0.3 (and at 0.2: 4 and 5, 0.35: 3 once, 0.4: 3 five times) but
    depth 3 and depth 4 fifteen times each at 0.45."""
    if name == "diag":
        D, scales = 10, _decades(10, 2.0)
    else:
        D, scales = 100, W.illcond_scales(100)
    k = np.arange(D)
    start = {"x": (0.5 * scales * np.cos(k)).astype(np.float32)}
    minv = {"x": (scales * (1.0 + 0.3 * np.sin(k))).astype(np.float32) ** 2}
    h_scale = float(np.abs(np.log(scales)).sum() + D * 0.5 * np.log(2 * np.pi) + D)
    return (_diag_normal(W.ns_product(), scales), _diag_normal(W.ns_oracle(), scales), start,
            minv, h_scale, 0.3 if name == "diag" else 0.45)


def _whiten(olp, start, minv):
    """The oracle's problem in q~ = q / s, s = sqrt(minv): log_prob(s * q~) from q0 / s."""
    import torch

    s = {k: np.sqrt(np.asarray(v, np.float32)) for k, v in minv.items()}
    st = {k: torch.as_tensor(v) for k, v in s.items()}
    wlp = lambda p: olp({k: st[k] * p[k] for k in p})  # noqa: E731
    wstart = {k: (np.asarray(v, np.float32) / s[k]).astype(np.float32) for k, v in start.items()}
    flat_s = np.concatenate([np.broadcast_to(s[k], np.shape(start[k])).ravel() for k in start])
    return wlp, wstart, flat_s.astype(np.float32)


_ORACLE = {}


def _oracle_run(name):
    """The whitened oracle run of a case, computed once."""
    if name not in _ORACLE:
        _, olp, start, minv, _, eps = _whitened_case(name)
        wlp, wstart, s = _whiten(olp, start, minv)
        ref = S.nuts(wlp, wstart, seed=11, num_samples=20, num_warmup=10, step_size=eps,
                     max_tree_depth=5, adapt_step_size=False)
        _ORACLE[name] = (ref, s)
    return _ORACLE[name]


@pytest.mark.parametrize("name", ["diag", "illcond100"])
def test_fixed_metric_matches_whitened_oracle(gpu, name):
    """Same seed and chain, fixed step size (0.3; 0.45 at D = 100, see
    _whitened_case), depth 5, 10 + 20 iterations: tree
    depths and leaf counts equal up to the first flip, which must be a near-tie
    the oracle proves (slice gap, divergence gap or relative U-turn margin within
    the bounds of tests/test_gpu_metric.py); positions within rtol 1e-3 before it
    and alpha within rtol 1e-4.  The oracle's trees are of mixed depth (checked
    below on the oracle alone: more than one depth, neither all at the cap of 5
    nor all at 0 or 1)."""
    import mlx_mcmc_amd as m

    plp, _, start, minv, h_scale, eps = _whitened_case(name)
    ref, s = _oracle_run(name)
    n_w, n_s, seed = 10, 20, 11
    rt = {k: np.asarray(v) for k, v in ref.trace.items()}
    depths = sorted(set(rt["depth"].tolist()))
    print(f"metric lanes {name}: oracle depths {depths}")
    assert len(depths) > 1 and not np.all(rt["depth"] == 5) and not np.all(rt["depth"] <= 1)
    samples, _, info = m.nuts(plp, start, key=m.random.key(seed), progress=False,
                              return_info=True, return_trace=True, nuts_kernel="lanes",
                              inverse_mass_matrix=minv, num_samples=n_s, num_warmup=n_w,
                              step_size=eps, max_tree_depth=5, adapt_step_size=False)
    assert info.extra["kernel"] == "lanes" and "kernel_note" not in info.extra
    tr = info.trace
    n, D = n_w + n_s, s.size
    gd, gl = tr["tree_depth"][0], tr["n_leapfrog"][0]
    same = next((i for i in range(n) if gd[i] != rt["depth"][i] or gl[i] != rt["leaves"][i]), n)
    print(f"metric lanes {name}: trees identical for {same} of {n} iterations")
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
    print(f"metric lanes {name}: max relative alpha deviation {dev.max():.3g}")
    np.testing.assert_allclose(tr["accept_stat"][0][:same], rt["alpha"][:same], rtol=1e-4,
                               atol=1e-6)
    k = max(0, same - n_w)
    flat = np.reshape(samples["x"], (n_s, -1))
    np.testing.assert_allclose(flat[:k], s * ref.samples[:k], rtol=1e-3, atol=1e-5)


# ---------------------------------------------------------------------------
# 3. first-window arithmetic
# ---------------------------------------------------------------------------
def test_first_window_update_matches_the_formula(gpu):
    """Fixed step size, depth 4, W = 100: the only window is [15, 90).  Run A
    adapts and is launched exactly through iteration 89; run B (num_warmup = 0,
    a metric of ones) stores the same iterations as samples — draws are a pure
    function of the iteration and A's metric is ones until the update."""
    from mlx_mcmc_amd import _lib, _trace

    D, C, Wm = 7, 3, 100
    ends = (ctypes.c_int64 * 8)()
    assert _lib.load().mc_metric_schedule(Wm, ends, 8) == 1 and ends[0] == 90
    lp, init = W.illcond_normal(W.ns_product(), D)
    prog = _trace.compile_model(lp, init)
    rng = np.random.default_rng(1)
    q0 = (W.illcond_scales(D) * rng.normal(size=(C, D))).astype(np.float32)
    common = dict(seed=9, depth=4, adapt_step_size=False, trace=False)
    _, _, _, A = _engine_run(prog, C, q0, 0.02, metric="ones", adapt=True,
                             chunks=[(0, 40), (40, 90)], num_warmup=Wm, num_samples=0, **common)
    sB, _, _, B = _engine_run(prog, C, q0, 0.02, metric="ones", chunks=[(0, 90)],
                              num_warmup=0, num_samples=90, **common)
    assert A.positions().cpu().numpy().tobytes() == B.positions().cpu().numpy().tobytes()
    x = sB[:, 15:90, :].astype(np.float64)                      # the window's 75 positions
    n = x.shape[1]
    var = x.var(axis=1, ddof=1)
    assert np.all(var > 0)
    want = (n / (n + 5.0)) * var + 1e-3 * (5.0 / (n + 5.0))
    np.testing.assert_allclose(A.inverse_mass().cpu().numpy(), want, rtol=1e-4)
    np.testing.assert_allclose(A._metric_section("msqrt").cpu().numpy(), 1 / np.sqrt(want),
                               rtol=1e-4)
    ms = A.metric_scalars()
    assert ms["n_updates"].tolist() == [1] * C and ms["n_window"].tolist() == [0] * C
    assert not A._metric_section("mean").cpu().numpy().any()    # the accumulator reset
    assert not A._metric_section("m2").cpu().numpy().any()
    assert np.all(B.inverse_mass().cpu().numpy() == 1)          # B never adapted


# ---------------------------------------------------------------------------
# 4. launch and chain splitting
# ---------------------------------------------------------------------------
def test_adapted_run_is_invariant_to_launch_and_chain_splits(gpu):
    """W = 150 (one window, [75, 100)), 20 samples, D = 10, 4 chains, depth 6,
    step size and metric both adapting: one launch, chunks that cut through the
    window, and chains 2 + 2 with chain_offset give the same bits."""
    from mlx_mcmc_amd import _trace

    D, C = 10, 4
    lp, init = W.illcond_normal(W.ns_product(), D)
    prog = _trace.compile_model(lp, init)
    rng = np.random.default_rng(2)
    q0 = (W.illcond_scales(D) * rng.normal(size=(C, D))).astype(np.float32)
    kw = dict(metric="ones", adapt=True, num_warmup=150, num_samples=20, depth=6, seed=21)
    one = _engine_run(prog, C, q0, 0.05, **kw)
    cut = _engine_run(prog, C, q0, 0.05,
                      chunks=[(0, 80), (80, 97), (97, 100), (100, 155), (155, 170)], **kw)
    halves = [_engine_run(prog, 2, q0[o:o + 2], 0.05, chain_offset=o, **kw) for o in (0, 2)]

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
    """Diagonal Gaussian, D = 16, scales over 1.5 decades, W = 1000, 8 chains,
    500 samples (the bounds and their argument: tests/test_gpu_metric.py — the
    last window's 500 draws put a factor of 2 in minv at five sigma, the pooled
    sd of 4000 draws within 10 % of the scale)."""
    import mlx_mcmc_amd as m

    D, C = 16, 8
    scales = _decades(D, 1.5)
    lp = _diag_normal(W.ns_product(), scales)
    init = {"x": np.zeros(D, np.float32)}
    kw = dict(num_samples=500, num_warmup=1000, num_chains=C, key=m.random.key(17),
              progress=False, return_info=True)
    s_ad, _, ad = m.nuts(lp, init, adapt_mass_matrix=True, nuts_kernel="lanes", **kw)
    _, _, ident = m.nuts(lp, init, **kw)                  # "auto": the same kernel, no metric
    assert ad.extra["kernel"] == "lanes" and "kernel_note" not in ad.extra
    assert ident.extra["kernel"] == "lanes" and "inverse_mass_matrix" not in ident.extra
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
                         nuts_kernel="lanes", inverse_mass_matrix=minv)
    np.testing.assert_array_equal(again.extra["inverse_mass_matrix"], minv)
    assert again.extra["metric_updates"].tolist() == [0] * C and again.extra["kernel"] == "lanes"


# ---------------------------------------------------------------------------
# 6. routing
# ---------------------------------------------------------------------------
def test_routing(gpu, monkeypatch):
    import mlx_mcmc_amd as m
    from mlx_mcmc_amd import _engine, _lib, _trace

    kw = dict(num_samples=4, num_warmup=4, progress=False, return_info=True, max_tree_depth=4,
              step_size=0.01)
    # shared parameters: lane-resident, not register-only
    lp, init = W.hierarchical(W.ns_product(), *W.SHAPES["small"])
    prog = _trace.compile_model(lp, init)
    assert prog.nuts_kernel(4) == "lanes" and not prog.nuts_register_only(4)
    assert _lib.load().mc_program_nuts_metric_lanes(prog.handle, 4) == 0
    with pytest.raises(_lib.EngineError, match="broadcast parameters or scalar terms") as e:
        _engine_run(prog, 2, prog.layout.flatten(init), 0.01, metric="ones", num_warmup=2,
                    num_samples=2, depth=4)
    assert e.value.code == _lib.MC_ERR_UNSUPPORTED
    # ... and nuts() says so before any launch
    launches = []
    for name in ("run_nuts", "run_nuts_metric", "run_nuts_metric_lanes"):
        monkeypatch.setattr(_engine.ChainSet, name,
                            lambda self, *a, _n=name, **k: launches.append(_n))
    for mkw in (dict(inverse_mass_matrix={k: np.ones_like(np.asarray(v, np.float32))
                                          for k, v in init.items()}),
                dict(adapt_mass_matrix=True)):
        with pytest.raises(ValueError, match="broadcast parameters or scalar terms") as ve:
            m.nuts(lp, init, nuts_kernel="lanes", **mkw, **kw)
        assert "default" in str(ve.value)
    assert launches == []
    monkeypatch.undo()
    # without a metric "lanes" is refused before anything is traced (an existing
    # test, tests/test_tracer.py, pins that; "auto" runs the lane kernel there)
    with pytest.raises(ValueError, match="nuts_kernel='lanes'.*mass matrix"):
        m.nuts(lp, init, nuts_kernel="lanes", **kw)
    _, _, info = m.nuts(lp, init, **kw)
    assert info.extra["kernel"] == "lanes" and "inverse_mass_matrix" not in info.extra
    # a model on the tape: "lanes" with a metric is an error
    ilp, iinit = W.iso_normal(W.ns_product(), 70)
    assert _trace.compile_model(ilp, iinit, slices=1).nuts_kernel(4) == "tape"
    with pytest.raises(ValueError, match="not planned as one lane-resident slice"):
        m.nuts(ilp, iinit, nuts_kernel="lanes", num_slices=1, adapt_mass_matrix=True, **kw)
    # the default nuts_kernel with a metric still takes the tape
    _, _, info = m.nuts(ilp, iinit, adapt_mass_matrix=True, **kw)
    assert info.extra["kernel"] == "tape" and "tape" in info.extra["kernel_note"]
    _, _, info = m.nuts(ilp, iinit, inverse_mass_matrix=np.ones(70, np.float32), **kw)
    assert info.extra["kernel"] == "tape"
    # and "lanes" takes the same model on the lane kernel
    _, _, info = m.nuts(ilp, iinit, nuts_kernel="lanes", adapt_mass_matrix=True, **kw)
    assert info.extra["kernel"] == "lanes" and info.extra["metric_updates"].tolist() == [0]
