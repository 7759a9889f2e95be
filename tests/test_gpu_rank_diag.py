"""Rank-normalised split R-hat, bulk-ESS and tail-ESS on the device
(mc_rank_diag, csrc/rankdiag.h) against the float64 restatement (_rank_diag).

Bars:
  * the five outputs: rtol 1e-9 (the bar of the f64 split R-hat in
    test_gpu_diag.py), on cases whose decision margin in the restatement — the
    smallest |even + odd| the sequence rule tested, the final |even| — is at
    least 1e-6, asserted on the restatement alone: a rounding difference then
    cannot move where the rule stops;
  * z-scores: the ranks are exact, so only the inverse normal CDF differs from
    scipy's ndtri.  Measured on an MI355X at these shapes: the largest
    |z - ndtri(...)| is Z_MEASURED; the gate is four times that (one more ulp
    per operation of another libm);
  * every sort path and batch size gives the same bits, as do two calls, with
    or without the z-scores.
"""
import functools

import numpy as np
import pytest

import _rank_diag as RD

pytestmark = pytest.mark.gpu

# (C, S, D): n = 4, the smallest defined; odd S; N = 108, no multiple of a
# wave; ties; (2, 257, 2); N = 10 400, past what a workgroup's LDS holds
ISSUE_SHAPES = [(1, 8, 1), (2, 9, 3), (3, 37, 5), (4, 130, 7), (2, 257, 2), (8, 1300, 3)]
# N = 8192: the largest column sorted in LDS (more than 64 KB of dynamic LDS), n = 1024 the
# longest split chain the autocovariance kernel holds in LDS; n = 1025: its other path
SHAPES = ISSUE_SHAPES + [(4, 2048, 2), (1, 2050, 2)]
SEED = 100
Z_MEASURED = 1.332e-15     # 3 ulp of a |z| in [2, 4): at (8, 1300, 3) and (4, 2048, 2)
Z_GATE = 4 * Z_MEASURED


@functools.lru_cache(maxsize=None)
def _case(shape):
    """(x, restatement) of a shape: computed once, shared, never written to."""
    x = RD.ar1_chains(SEED, *shape)
    x.setflags(write=False)
    return x, RD.buffer(x)


def _run(x, path=0, z=False):
    import torch

    from mlx_mcmc_amd import _lib
    from mlx_mcmc_amd import diagnostics as Dg

    lib = _lib.load()
    lib.mc_debug_rank_path(path)
    try:
        d = Dg.rank_diagnostics(torch.tensor(np.asarray(x, np.float32), device="cuda"),
                                group=False, z_scores=z)
    finally:
        lib.mc_debug_rank_path(0)
    if z:
        d["z"] = d["z"].cpu().numpy()
    return d


def _same_bits(a, b, what=""):
    for f in RD.FIELDS:
        assert a[f].tobytes() == b[f].tobytes(), (what, f, a[f], b[f])
    assert a["n_constant"] == b["n_constant"], what


def _check_outputs(got, ref, what):
    out, _, n_const, margin = ref
    assert margin >= 1e-6, (what, margin)       # (a condition on the restatement)
    for f in RD.FIELDS:
        with np.errstate(all="ignore"):
            rel = np.abs(got[f] - out[f]) / np.abs(out[f])
        err = np.max(rel[np.isfinite(rel)], initial=0.0)
        print(f"{what} {f}: largest relative difference {err:.2e} (margin {margin:.2e})")
    for f in RD.FIELDS:
        np.testing.assert_allclose(got[f], out[f], rtol=1e-9, atol=0, err_msg=f"{what} {f}")
    assert got["n_constant"] == n_const


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_outputs_and_z_scores_match_the_restatement(gpu, shape):
    x, ref = _case(shape)
    got = _run(x, z=True)
    _check_outputs(got, ref, str(shape))
    C, S, Dn = shape
    assert got["z"].shape == (Dn, 2 * C, S // 2)
    dz = float(np.max(np.abs(got["z"] - ref[1])))
    print(f"{shape} z-scores: largest |device - scipy| {dz:.3e} (gate {Z_GATE:.3e})")
    assert dz <= Z_GATE


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_paths_batches_and_calls_give_the_same_bits(gpu, shape):
    x, _ = _case(shape)
    auto = _run(x, z=True)
    _same_bits(auto, _run(x), "a second call, without z")
    forced = _run(x, path=1, z=True)            # the multi-workgroup sort
    _same_bits(auto, forced, "multi-workgroup sort")
    assert auto["z"].tobytes() == forced["z"].tobytes()
    if shape[2] > 3:                            # batches of 3 elements
        split = _run(x, path=2, z=True)
        _same_bits(auto, split, "batches of 3")
        assert auto["z"].tobytes() == split["z"].tobytes()


def test_batches_of_three_on_the_tie_shape(gpu):
    """(4, 130, 7) under path 2: 7 elements in batches of 3, 3 and 1."""
    from mlx_mcmc_amd import _lib

    lib = _lib.load()
    x, ref = _case((4, 130, 7))
    assert lib.mc_debug_rank_path(2) == 0
    try:
        assert lib.mc_rank_diag_workspace_bytes(4, 130, 7) == \
            lib.mc_rank_diag_workspace_bytes(4, 130, 3)
    finally:
        lib.mc_debug_rank_path(0)
    _check_outputs(_run(x, path=2), ref, "(4, 130, 7) in batches of 3")


def test_a_monotone_map_leaves_the_bulk_outputs_bit_identical(gpu):
    """exp(x) has the ranks of x (x on a grid of 1/64, so that exp merges no two
    values in float32: asserted), hence the same rhat_bulk and ess_bulk bits."""
    from scipy.stats import rankdata

    x, _ = _case((3, 37, 5))
    xg = (np.round(x * 64) / 64).astype(np.float32)
    ex = np.exp(xg.astype(np.float64)).astype(np.float32)
    for d in range(xg.shape[2]):
        np.testing.assert_array_equal(rankdata(RD.split(xg[:, :, d]).ravel()),
                                      rankdata(RD.split(ex[:, :, d]).ravel()))
    a, b = _run(xg), _run(ex)
    for f in ("rhat_bulk", "ess_bulk"):
        assert a[f].tobytes() == b[f].tobytes(), f
    assert np.all(np.isfinite(a["rhat_bulk"])) and np.all(np.isfinite(a["ess_bulk"]))


def test_scale_and_tail_disagreements_the_classic_rhat_misses(gpu):
    """Four N(0, 1) chains of 1000 draws, one scaled by 3; four Cauchy chains,
    one shifted by 2: the classic split R-hat passes both."""
    import torch

    from mlx_mcmc_amd import diagnostics as Dg

    rng = np.random.default_rng(2)
    a = rng.standard_normal((4, 1000)).astype(np.float32)
    a[3] *= 3
    b = rng.standard_cauchy((4, 1000)).astype(np.float32)
    b[3] += 2
    x = np.stack([a, b], axis=2)
    classic = Dg.chain_diagnostics(torch.from_numpy(x).cuda(), group=False)["rhat"]
    got = _run(x)
    print(f"classic split R-hat {classic}, rank-normalised {got['rhat_rank']}, "
          f"tail-ESS {got['ess_tail']}")
    assert np.all(classic < 1.01)
    assert np.all(got["rhat_rank"] > 1.01)
    ref = RD.buffer(x)
    _check_outputs(got, ref, "scaled / shifted")


def test_a_nan_draw_spoils_its_element_alone(gpu):
    x, _ = _case((3, 37, 5))
    base = _run(x)
    y = x.copy()
    y[1, 5, 2] = np.nan
    got = _run(y, z=True)
    for f in RD.FIELDS:
        assert np.isnan(got[f][2]), f
        keep = [0, 1, 3, 4]
        assert got[f][keep].tobytes() == base[f][keep].tobytes(), f
    assert got["n_constant"] == 0
    # a NaN in the dropped middle draw of an odd S is no draw of a split chain
    y = x.copy()
    y[0, 18, 2] = np.nan
    _same_bits(_run(y), base, "NaN in the middle draw")


def test_an_infinite_draw_has_a_rank(gpu):
    x, _ = _case((3, 37, 5))
    y = x.copy()
    y[2, 30, 1] = np.inf
    y[0, 3, 4] = -np.inf
    got = _run(y, z=True)
    ref = RD.buffer(y)
    _check_outputs(got, ref, "+-inf")
    assert float(np.max(np.abs(got["z"] - ref[1]))) <= Z_GATE
    assert np.all(np.isfinite(got["rhat_bulk"])) and np.all(np.isfinite(got["ess_tail"]))


def test_constant_elements_are_nan_and_counted(gpu):
    x, _ = _case((4, 130, 7))
    base = _run(x)
    y = x.copy()
    y[:, :, 1] = 2.5
    y[:, :, 5] = 0.0
    y[::2, ::2, 5] = -0.0           # -0 and +0 are equal: still constant
    got = _run(y)
    assert got["n_constant"] == 2
    for f in RD.FIELDS:
        assert np.isnan(got[f][[1, 5]]).all(), f
        keep = [0, 2, 3, 4, 6]
        assert got[f][keep].tobytes() == base[f][keep].tobytes(), f
    _check_outputs(got, RD.buffer(y), "constant elements")


def test_fewer_than_four_draws_per_half_is_nan(gpu):
    x = RD.ar1_chains(SEED, 2, 7, 3)
    got = _run(x, z=True)
    for f in RD.FIELDS:
        assert got[f].shape == (3,) and np.isnan(got[f]).all(), f
    assert got["n_constant"] == 0
    assert got["z"].shape == (3, 4, 3) and np.isnan(got["z"]).all()


def test_mcmc_diagnostics_facade(gpu):
    import mlx_mcmc_amd as m
    import workloads as W
    from mlx_mcmc_amd import diagnostics as Dg

    G, N = W.SHAPES["small"]
    lp, init = W.hierarchical(W.ns_product(), G, N)
    mc = m.MCMC(lp)
    s = mc.run(init, num_samples=300, num_warmup=200, method="hmc", random_seed=2,
               verbose=False, num_chains=4, progress=False, num_leapfrog_steps=8, step_size=0.05)
    plain = mc.diagnostics()
    full = mc.diagnostics(rank_normalized=True)
    new = {"ess_bulk", "ess_tail", "r_hat_rank", "r_hat_bulk", "r_hat_folded"}
    direct = Dg.rank_diagnostics(mc.info.device_samples, group=False)
    lay = mc.info.layout
    for name, shape, off in zip(lay.names, lay.shapes, lay.offsets):
        assert set(plain[name]) == {"ess", "ess_sum", "r_hat"}     # the default: as before
        assert set(full[name]) == set(plain[name]) | new
        for k in plain[name]:
            np.testing.assert_array_equal(full[name][k], plain[name][k])
        size = int(np.prod(shape)) if shape else 1
        for k, src in (("ess_bulk", "ess_bulk"), ("ess_tail", "ess_tail"),
                       ("r_hat_rank", "rhat_rank"), ("r_hat_bulk", "rhat_bulk"),
                       ("r_hat_folded", "rhat_folded")):
            assert full[name][k].shape == s[name].shape[2:], (name, k)
            assert full[name][k].dtype == np.float64
            np.testing.assert_array_equal(full[name][k].ravel(), direct[src][off:off + size])
        assert np.all(np.isfinite(full[name]["r_hat_rank"]))
        assert np.all(full[name]["ess_bulk"] > 0) and np.all(full[name]["ess_tail"] > 0)
