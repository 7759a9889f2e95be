"""Ragged and empty group runs on every hand-written sweep (tests/_ragged.py
PATTERNS): the lane kernels' moment sums (lanes_fast.h lf_moments, lanes.h
lr_moments, nuts_sliced.h nsl_moments, mh_sliced.h msl_sumsq), the term
interpreter's (sliced.h run_moments2) and the tape's segment tiles, against
the closed form in float64 within derived bounds (_ragged.bounds: sharp
enough to see one element, tests/test_ragged_reference.py).

The balanced workloads give every lane a run of 100..143 elements: two
pipelined rounds or more, one remainder, a tail of 0 or 1.  Here runs are
0..7 long (lmin4 = 0, empty lanes), 16..23 (one round, the clamped prefetch
reloads it), 32..54 (remainders 0..3, tails of 0..7 across a float4
boundary), 1..3 beside 301, spread over 2 and 4 register slots with the last
slot part-filled, and split over lane groups of 2, 8 and 16 with members
left empty (plan_lanes.hip plan_lanes).

  * the tape (mc_logp_grad) at 4 perturbed points, sorted and shuffled group
    index;
  * the HMC state (position, gradient, log p) after 6 iterations on k_hmc_lf
    (compile-time and run-time form, 1 / 2 / 3 slices, MC_LANES_REP=1),
    k_hmc_lr's generic path and k_hmc_sl; every chain accepted at least once;
  * HMC trajectories (10 + 10 iterations, L = 7: first, paired, aligning and
    trailing steps) against k_hmc — decisions equal up to a proven near-tie
    (tests/_near_tie.py), step sizes equal, draws rtol 1e-3 / atol 1e-4 —
    against the oracle on tiny / rem1 / skew, and byte-identical launch
    splits on tiny / rem3 / rep8;
  * NUTS (k_nuts_lr plain and generic, k_nuts_sl at 2 slices): the state, and
    the tape k_nuts's tree depths and leaf counts for the first 6 iterations
    at least, energies rtol 1e-5 while they agree;
  * MH (k_mh_sl at 2 slices, 40 iterations): log p, and k_mh's decisions up
    to a near-tie of 8 ulp of |log p|, log p rtol 2e-6 and draws before it,
    three chains of four agreeing over the whole run.

The trajectory comparisons take tests/_near_tie.py's plain bound: 8 ulp of
|H_init|, or of the sum of log p's terms' magnitudes at the start where that
is larger (h_scale; the two are of one size).  `ones` is left out of them:
with one observation per group and theta started on it, sigma runs towards 0
(the funnel), the trajectories are unstable at this step size, and every
kernel — the interpreter and the lanes alike — leaves the tape's log ratios by
up to 3e-3 (|H| ~ 1e2: 8 ulp = 6e-5 .. 1.2e-4) with all decisions equal; the
NUTS energies drift the same way.  No per-iteration bound derived from the
roundings held there, so `ones` keeps its state checks against f64 on every
kernel (HMC, NUTS, MH), its NUTS trees and its MH decisions, and the
trajectory comparisons run the other 14 patterns.

Checked against a mutant: with lf_moments' tail mask off by one (e + k <= len)
every k_hmc_lf state case fails on every pattern but exact32 and ones (no
tail), and the other kernels' cases pass.

Every case asserts the kernel it ran, and the one-slice lane cases the
planned register slots and lane replication (_ragged.PLAN).  No pattern needed shrinking: few_long
(a run of 700) runs on the lanes as planned (rep = 16: 44 elements a lane);
only with MC_LANES_REP=1 would its one-slice tile (64 x 704 floats) exceed the
150 KB LDS budget, and that combination is not among the cases.
"""
import numpy as np
import pytest

import workloads as W
from _near_tie import compare_trace, log_u, tie_bound
from _ragged import PATTERNS, PLAN, _evaluate, check_state, perturbed_points, ragged_hier

pytestmark = pytest.mark.gpu

NAMES = sorted(PATTERNS)
TRAJ = [n for n in NAMES if n != "ones"]     # (the funnel: see the docstring)
REP = ["rep16", "rep2", "rep8"]
C = 4
BIG = {"lf1": "rem2", "lf1_rt": "slots4", "lf2": "tiny", "lf3": "skew", "lr": "slots2",
       "sl2": "rem0"}                      # one 12-chain case per kernel (a part-filled block)

# kernel configurations: (slices, slice_kernel, extra, run-time form, MC_LANES_REP=1)
CONFIGS = {
    "lf1": (1, "lanes", None, False, False),
    "lf1_rt": (1, "lanes", None, True, False),
    "lf2": (2, "lanes", None, False, False),
    "lf3": (3, "lanes", None, False, False),
    "lf1_rep1": (1, "lanes", None, False, True),
    "lr": (1, "lanes", "scalar_mix", False, False),
    "sl2": (2, "interpreter", None, False, False),
    "tape": (1, "auto", None, False, False),
    "tape_mix": (1, "auto", "scalar_mix", False, False),
}
_models = {}
_progs = {}


def _model(name, order="sorted", extra=None):
    key = (name, order, extra)
    if key not in _models:
        _models[key] = ragged_hier(W.ns_product(), PATTERNS[name], order=order, extra=extra)
    return _models[key]


def _program(name, config, monkeypatch, order="sorted"):
    """The planned program of a pattern on a kernel configuration, with the
    kernel an HMC launch will run asserted."""
    from mlx_mcmc_amd import _trace

    slices, kernel, extra, _, rep1 = CONFIGS[config]
    key = (name, config, order)
    if key not in _progs:
        if rep1:
            monkeypatch.setenv("MC_LANES_REP", "1")   # (read when the lanes are planned)
        lp, init, data = _model(name, order, extra)
        prog = _trace.compile_model(lp, init, slices=slices, slice_kernel=kernel)
        _progs[key] = (prog, init, data, extra)
    prog, init, data, extra = _progs[key]
    if config.startswith("tape"):
        assert prog.slice_kernel == "unsliced" and prog.num_slices <= 1
    elif config == "sl2":
        assert prog.slice_kernel == "interpreter" and prog.num_slices == 2
    else:
        assert prog.slice_kernel == "lanes", prog.kernel_note
        assert prog.num_slices == slices or (slices == 1 and prog.num_slices <= 1)
        assert prog.lanes_fast == (config != "lr"), (config, prog.kernel_note)
        if slices == 1:     # the regime the pattern is named for
            rs, rep = PLAN[name]
            assert (prog.lane_slots, prog.lane_rep) == (rs, 1 if rep1 else rep), (name, config)
    return prog, init, data, extra


class _forms:
    """mc_debug_lanes_forms(0) around a launch: k_hmc_lf reads its form at run time."""

    def __init__(self, runtime):
        self.runtime = runtime

    def __enter__(self):
        from mlx_mcmc_amd import _lib

        if self.runtime:
            _lib.load().mc_debug_lanes_forms(0)

    def __exit__(self, *a):
        from mlx_mcmc_amd import _lib

        if self.runtime:
            _lib.load().mc_debug_lanes_forms(1)


def _hmc_state(prog, init, chains, splits=(6,), L=5, eps=0.01, runtime=False):
    """Everything an HMC run of sum(splits) iterations leaves behind."""
    import torch

    from mlx_mcmc_amd import _engine

    n = sum(splits)
    cfg = dict(chain_offset=0, num_warmup=n // 2, num_samples=n - n // 2, sample_begin=0,
               sample_capacity=n - n // 2, seed=5, step_size=eps, target_accept=0.8,
               num_leapfrog_steps=L, adapt_step_size=True)
    with _forms(runtime):
        cs = _engine.ChainSet(prog, chains, prog.layout.flatten(init), eps)
        out = torch.zeros((chains, n - n // 2, prog.D), dtype=torch.float32, device=cs.device)
        it = 0
        for k in splits:
            cs.run_hmc(samples=out, iter_begin=it, iter_count=k, **cfg)
            it += k
        torch.cuda.synchronize()
        cs.check_status()
    sc = cs.scalars()
    return {"samples": out.cpu().numpy(), "q": cs.positions().cpu().numpy(),
            "g": cs.gradients().cpu().numpy(), "logp": sc["logp"].copy(),
            "step_size": sc["step_size"].copy(),
            "n_accept": sc["n_accept"] + sc["warmup_accept"],
            "n_total": sc["n_total"] + sc["warmup_total"]}


# ------------------------------------------------------------------ the tape --
@pytest.mark.parametrize("config,order", [("tape", "sorted"), ("tape", "shuffled"),
                                          ("tape_mix", "sorted")])
@pytest.mark.parametrize("name", NAMES)
def test_tape_at_arbitrary_points(gpu, monkeypatch, name, config, order):
    from mlx_mcmc_amd import _engine

    prog, init, data, extra = _program(name, config, monkeypatch, order)
    pts = perturbed_points(init, n=4)
    assert np.all(pts[:, 1:3] > 0)
    lp, g = _engine.logp_grad(prog, pts)
    check_state(pts, g.cpu().numpy(), lp.cpu().numpy(), data, extra, what=f"tape {name} {order}")


# ------------------------------------------------------------- the HMC state --
def _state_case(name, config, monkeypatch, order="sorted"):
    prog, init, data, extra = _program(name, config, monkeypatch, order)
    chains = 12 if BIG.get(config) == name else C
    r = _hmc_state(prog, init, chains, runtime=CONFIGS[config][3])
    assert np.all(r["n_total"] == 6)
    assert np.all(r["n_accept"] >= 1), "every chain must have moved off k_init's state"
    assert np.all(np.any(r["q"] != prog.layout.flatten(init)[None, :], axis=1))
    check_state(r["q"], r["g"], r["logp"], data, extra, what=f"hmc {config} {name} {order}")


@pytest.mark.parametrize("config", ["lf1", "lf1_rt", "lf2", "lf3", "lr", "sl2"])
@pytest.mark.parametrize("name", NAMES)
def test_hmc_state_against_f64(gpu, monkeypatch, name, config):
    _state_case(name, config, monkeypatch)


@pytest.mark.parametrize("name", NAMES)
def test_hmc_state_shuffled_groups(gpu, monkeypatch, name):
    """An unsorted group index on the one-slice fast-form kernel."""
    _state_case(name, "lf1", monkeypatch, order="shuffled")


@pytest.mark.parametrize("name", REP)
def test_hmc_state_one_lane_per_parameter(gpu, monkeypatch, name):
    """MC_LANES_REP=1 on the patterns the planner replicates (their planned
    rep = 16 / 2 / 8 runs in test_hmc_state_against_f64)."""
    _state_case(name, "lf1_rep1", monkeypatch)


# ------------------------------------------------------- the HMC trajectories --
_traj = {}


def _hmc(name, config, extra=None):
    import mlx_mcmc_amd as m

    slices, kernel, cextra, runtime, _ = CONFIGS[config]
    extra = cextra if cextra is not None else extra
    key = (name, config, extra)
    if key not in _traj:
        lp, init, data = _model(name, "sorted", extra)
        with _forms(runtime):
            s, _, info = m.hmc(lp, init, num_samples=10, num_warmup=10, step_size=0.02,
                               num_leapfrog_steps=7, key=m.random.key(3), num_chains=C,
                               progress=False, return_info=True, return_trace=True,
                               num_slices=slices, slice_kernel=kernel)
        want = {"tape": "unsliced", "tape_mix": "unsliced", "sl2": "interpreter"}.get(config,
                                                                                      "lanes")
        assert info.extra["kernel"] == want, (config, info.extra)
        _traj[key] = (s, info)
    return _traj[key]


def _h_scale(name, extra):
    """The magnitude of log p's summands at the start (tests/_near_tie.py
    h_scale: it replaces |H_init| where a log p near zero makes that smaller)."""
    _, init, data = _model(name, "sorted", extra)
    q0 = perturbed_points(init, n=1)[0]
    return float(_evaluate(data, q0, extra, np.float64, mags=True)[0])


def _same_prefix(got, ref, lu, label, name, extra):
    """compare_trace of every chain: (s, info) pairs of the product API."""
    out = []
    for c in range(C):
        r = {"accepted": ref[1].trace["accepted"][c], "ratio": ref[1].trace["accept_stat"][c],
             "energy": ref[1].trace["energy"][c], "step_size": ref[1].trace["step_size"][c],
             "log_u": lu[c]}
        g = {"accepted": got[1].trace["accepted"][c], "ratio": got[1].trace["accept_stat"][c],
             "energy": got[1].trace["energy"][c], "step_size": got[1].trace["step_size"][c]}
        same = compare_trace(g, r, f"{label} chain {c}", h_scale=_h_scale(name, extra))
        ns = max(0, same - 10)
        for k in ref[0]:
            np.testing.assert_allclose(got[0][k][c, :ns], ref[0][k][c, :ns], rtol=1e-3, atol=1e-4,
                                       err_msg=f"{label} chain {c} {k}")
        out.append(same)
    return out


@pytest.mark.parametrize("config", ["lf1", "lf1_rt", "lf2", "lf3", "lr", "sl2"])
@pytest.mark.parametrize("name", TRAJ)
def test_hmc_trajectory_matches_tape_kernel(gpu, name, config):
    extra = CONFIGS[config][2]
    ref = _hmc(name, "tape_mix" if extra else "tape")
    got = _hmc(name, config)
    lu = [log_u(3, c, 20) for c in range(C)]
    same = _same_prefix(got, ref, lu, f"{config} {name}", name, extra)
    assert ref[1].trace["accepted"].any(), "the chains must move"
    assert sum(s == 20 for s in same) >= C // 2, same


@pytest.mark.parametrize("config", ["lf1", "lf2", "lr", "sl2", "tape"])
@pytest.mark.parametrize("name", ["tiny", "rem1", "skew"])
def test_hmc_trajectory_matches_oracle(gpu, name, config):
    """Chain 0 against oracle.samplers.hmc on the oracle-namespace model (as
    tests/test_gpu_large_parity.py: decisions up to a proven near-tie, ratios
    and H within the tie bound, step sizes equal, draws rtol 1e-4)."""
    from oracle import samplers as S

    extra = CONFIGS[config][2]
    key = ("oracle", name, extra)
    if key not in _traj:
        olp, oinit, _ = ragged_hier(W.ns_oracle(), PATTERNS[name], extra=extra)
        _traj[key] = S.hmc(olp, oinit, num_samples=10, num_warmup=10, step_size=0.02,
                           num_leapfrog_steps=7, seed=3, chain=0)
    ref = _traj[key]
    s, info = _hmc(name, config)
    r = {k: np.asarray(ref.trace[k]) for k in ("accepted", "ratio", "step_size", "energy")}
    r["log_u"] = log_u(3, 0, 20)
    g = {"accepted": info.trace["accepted"][0], "ratio": info.trace["accept_stat"][0],
         "energy": info.trace["energy"][0], "step_size": info.trace["step_size"][0]}
    same = compare_trace(g, r, f"{config} {name} vs oracle", h_scale=_h_scale(name, extra))
    assert same >= 10, same
    _, init, _ = _model(name, "sorted", extra)
    draws = np.concatenate([np.asarray(s[k][0]).reshape(10, -1) for k in init], axis=1)
    np.testing.assert_allclose(draws[:same - 10], ref.samples[:same - 10], rtol=1e-4, atol=1e-5)
    assert r["accepted"][:same].any()


@pytest.mark.parametrize("config", ["lf1", "lf1_rt", "lf2", "lr", "sl2"])
@pytest.mark.parametrize("name", ["tiny", "rem3", "rep8"])
def test_hmc_launch_splits_identical(gpu, monkeypatch, name, config):
    prog, init, _, _ = _program(name, config, monkeypatch)
    rt = CONFIGS[config][3]
    one = _hmc_state(prog, init, C, splits=(6,), L=7, eps=0.02, runtime=rt)
    parts = _hmc_state(prog, init, C, splits=(1, 2, 3), L=7, eps=0.02, runtime=rt)
    assert np.all(one["n_total"] == 6) and np.all(np.isfinite(one["logp"]))
    for k in one:
        assert one[k].tobytes() == parts[k].tobytes(), f"{config} {name}: {k} differs"


# ---------------------------------------------------------------------- NUTS --
NUTS = {"lanes": ("lf1", "lanes"), "lanes_generic": ("lr", "lanes"), "sliced2": ("lf2", "sliced")}
_nuts_tape = {}


def _nuts(prog, init, chains=C):
    import torch

    from mlx_mcmc_amd import _engine

    cfg = dict(chain_offset=0, num_warmup=4, num_samples=6, sample_begin=0, sample_capacity=6,
               seed=3, step_size=0.02, target_accept=0.65, max_tree_depth=6,
               adapt_step_size=False, slice_mode=0)
    cs = _engine.ChainSet(prog, chains, prog.layout.flatten(init), 0.02)
    tr = _engine.make_trace(chains, 0, 10, cs.device)
    smp = torch.zeros((chains, 6, prog.D), dtype=torch.float32, device=cs.device)
    cs.run_nuts(samples=smp, trace=tr, iter_begin=0, iter_count=10, **cfg)
    torch.cuda.synchronize()
    cs.check_status()
    return {"q": cs.positions().cpu().numpy(), "g": cs.gradients().cpu().numpy(),
            "logp": cs.scalars()["logp"].copy(), "trace": tr.numpy()}


@pytest.mark.parametrize("kind", sorted(NUTS))
@pytest.mark.parametrize("name", NAMES)
def test_nuts_state_and_trees(gpu, monkeypatch, name, kind):
    config, want = NUTS[kind]
    prog, init, data, extra = _program(name, config, monkeypatch)
    assert prog.nuts_kernel(6) == want
    chains = 12 if name == "rem1" else C
    r = _nuts(prog, init, chains)
    assert np.all(np.any(r["q"] != prog.layout.flatten(init)[None, :], axis=1)), "chains moved"
    check_state(r["q"], r["g"], r["logp"], data, extra, what=f"nuts {kind} {name}")
    # the tape kernel's trees, as tests/test_gpu_nuts_sliced.py
    # test_sliced_matches_tape_kernel holds them: depth and leaf count
    # identical for the first 6 iterations at least, energies rtol 1e-5 over
    # the agreeing prefix
    tkey = (name, extra, chains)
    if tkey not in _nuts_tape:
        tprog, tinit, _, _ = _program(name, "tape_mix" if extra else "tape", monkeypatch)
        assert tprog.nuts_kernel(6) == "tape"
        _nuts_tape[tkey] = _nuts(tprog, tinit, chains)["trace"]
    ta, tb = r["trace"], _nuts_tape[tkey]
    for c in range(chains):
        n = 0
        while n < 10 and (ta["tree_depth"][c][n] == tb["tree_depth"][c][n]
                          and ta["n_leapfrog"][c][n] == tb["n_leapfrog"][c][n]):
            n += 1
        assert n >= 6, (c, ta["tree_depth"][c], tb["tree_depth"][c])
        m = 1 if name == "ones" else n      # (the funnel: later states drift, see the docstring)
        np.testing.assert_allclose(ta["energy"][c][:m], tb["energy"][c][:m], rtol=1e-5)
    # (that test's depth >= 4 is the medium shape's; these posteriors are wide
    # against the step size, and depth 2 is already a tree with a U-turn check)
    assert tb["tree_depth"].max() >= 2, "real trees"


# ------------------------------------------------------------------------ MH --
def _mh(prog, init, chains, n=40, scale=0.02, seed=7):
    import torch

    from mlx_mcmc_amd import _engine

    cs = _engine.ChainSet(prog, chains, prog.layout.flatten(init), scale)
    tr = _engine.make_trace(chains, 0, n, cs.device)
    smp = torch.zeros((chains, n, prog.D), dtype=torch.float32, device=cs.device)
    cs.run_mh(proposal_scale=scale, samples=smp, trace=tr, chain_offset=0, num_warmup=0,
              num_samples=n, iter_begin=0, iter_count=n, sample_begin=0, sample_capacity=n,
              seed=seed)
    torch.cuda.synchronize()
    cs.check_status()
    return {"q": cs.positions().cpu().numpy(), "logp": cs.scalars()["logp"].copy(),
            "trace": tr.numpy(), "samples": smp.cpu().numpy()}


@pytest.mark.parametrize("name", NAMES)
def test_mh_sliced_logp_and_decisions(gpu, monkeypatch, name):
    from mlx_mcmc_amd import _lib

    lib = _lib.load()
    prog, init, data, extra = _program(name, "lf2", monkeypatch)
    tprog, _, _, _ = _program(name, "tape", monkeypatch)
    assert lib.mc_program_mh_sliced(prog.handle) == 1
    assert lib.mc_program_mh_sliced(tprog.handle) == 0
    chains = 12 if name == "rem2" else C
    a, b = _mh(prog, init, chains), _mh(tprog, init, chains)
    acc = a["trace"]["accepted"].astype(bool)
    assert np.all(acc.any(axis=1)), "every chain must have accepted a proposal"
    check_state(a["q"], None, a["logp"], data, extra, what=f"mh sliced {name}")
    racc = b["trace"]["accepted"].astype(bool)
    full = 0
    for c in range(chains):
        flips = np.nonzero(acc[c] != racc[c])[0]
        same = int(flips[0]) if flips.size else 40
        if same < 40:
            lu = log_u(7, c, 40)
            tie = tie_bound(b["trace"]["energy"][c][same])
            gap = abs(float(lu[same]) - float(b["trace"]["accept_stat"][c][same]))
            assert gap <= tie, f"chain {c}: flip at {same} is no near-tie: {gap} > {tie}"
        # tests/test_gpu_mh_sliced.py's bars before the flip
        full += same == 40
        np.testing.assert_allclose(a["trace"]["energy"][c][:same], b["trace"]["energy"][c][:same],
                                   rtol=2e-6)
        np.testing.assert_allclose(a["samples"][c][:same], b["samples"][c][:same], rtol=1e-5,
                                   atol=1e-6)
    # A near-tie can fall on any iteration, so no chain has a floor of its own
    # (that test's same >= 20 is one chain's).  They are rare: the tie is
    # ~2e-3 wide at |log p| ~ 3e3 against log ratios spread over ~1, some 1e-3
    # per iteration and 4 % per chain of 40 — so all chains but a quarter (one
    # of 4, three of 12) must agree to the end.
    assert full >= chains - max(1, chains // 4), (full, chains)
