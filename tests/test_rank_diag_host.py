"""Rank-normalised diagnostics without a device: the library's host statement
of the sequence rule (mc_geyer_ess_host: the code the kernel runs) against the
float64 restatement, the new symbols' declaration, export and binding, and the
facade's refusal of a multi-rank group."""
import ctypes
import os
import re

import numpy as np
import pytest

import _rank_diag as RD
from mlx_mcmc_amd import _lib, diagnostics as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mc_rank_diag_workspace_bytes", "mc_rank_diag", "mc_geyer_ess_host", "mc_debug_rank_path")


def _host_ess(rho, n, N):
    """mc_geyer_ess_host on rho[0 .. n-1] (rho[0] = 1 is not passed)."""
    lib = _lib.load()
    r = np.ascontiguousarray(rho[1:n], np.float64)
    assert r.size == n - 1
    out = ctypes.c_double()
    rc = lib.mc_geyer_ess_host(r.ctypes.data_as(ctypes.c_void_p), n, N, ctypes.byref(out))
    assert rc == _lib.MC_OK, lib.mc_last_error()
    return out.value


def _seq(vals, n):
    """rho[0 .. n-1]: 1, then vals, then zeros."""
    rho = np.zeros(n)
    rho[0] = 1.0
    rho[1:1 + len(vals)] = vals
    return rho


# label -> (rho[0 .. n-1], n, N); test_hand_made_sequences_are_the_cases_named shows on the
# restatement that each is the case its label names
HAND = {
    "first pair negative": (_seq([-1.5, 0.4, 0.3, 0.2], 12), 12, 48),
    "positive to the bound": (0.9 ** np.arange(12), 12, 48),
    "positive to the bound, odd n": (0.9 ** np.arange(13), 13, 26),
    "non-monotone bump": (_seq([0.5, 0.1, 0.05, 0.3, 0.25, 0.2, 0.15, 0.01, 0.005, -0.2, -0.1], 20),
                          20, 80),
    "last even <= 0, pair written": (_seq([0.5, 0.3, 0.2, -0.1, 0.3], 8), 8, 32),
    "last even <= 0, pair not written": (_seq([0.5, 0.3, 0.2, -0.3, 0.1, 0.4, 0.4], 16), 16, 64),
    "n = 4": (_seq([0.3, 0.2, 0.1], 4), 4, 8),
    "n = 5": (_seq([0.3, 0.2, 0.1, 0.05], 5), 5, 10),
    "n = 5, negative": (_seq([-0.3, 0.2, 0.1, 0.05], 5), 5, 10),
    "tau below the floor": (_seq([-0.9, -0.05, -0.02, 0.0, 0.0], 10), 10, 40),
}


@pytest.mark.parametrize("label", sorted(HAND))
def test_host_rule_on_hand_made_sequences(label):
    rho, n, N = HAND[label]
    ref, margin = RD.geyer(rho, n, N)
    got = _host_ess(rho, n, N)
    print(f"{label}: ESS {got:.12g} (restatement {ref:.12g}), margin {margin:.3g}")
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=0)


def test_hand_made_sequences_are_the_cases_named():
    """Conditions on the restatement alone."""
    floor = lambda N: N / (1 / np.log10(N))   # ESS at tau = 1 / log10 N
    assert RD.geyer(*HAND["first pair negative"])[0] == floor(48)
    assert RD.geyer(*HAND["tau below the floor"])[0] == floor(40)
    assert RD.geyer(*HAND["n = 4"])[0] == floor(8)             # tau = -1 + 0 + 1
    rho, n, N = HAND["positive to the bound"]
    # pairs (0,1) .. (6,7) summed, the even of (8,9) added
    tau = -1 + 2 * np.sum(rho[:8]) + rho[8]
    np.testing.assert_allclose(RD.geyer(rho, n, N)[0], N / tau, rtol=1e-14)
    rho, n, N = HAND["non-monotone bump"]
    # the pair (4, 5) = 0.55 is cut to the pair (2, 3) = 0.15, (6, 7) to 0.15 as well
    tau = -1 + 2 * (1.5 + 0.15 + 0.15 + 0.15 + 0.015) + 0.0
    np.testing.assert_allclose(RD.geyer(rho, n, N)[0], N / tau, rtol=1e-14)
    rho, n, N = HAND["last even <= 0, pair written"]
    tau = -1 + 2 * (1.5 + 0.5) + (-0.1)
    np.testing.assert_allclose(RD.geyer(rho, n, N)[0], N / tau, rtol=1e-14)
    rho, n, N = HAND["last even <= 0, pair not written"]
    tau = -1 + 2 * (1.5 + 0.5) + 0.0
    np.testing.assert_allclose(RD.geyer(rho, n, N)[0], N / tau, rtol=1e-14)


@pytest.mark.parametrize("shape", [(1, 8, 4), (2, 9, 4), (3, 37, 4), (4, 130, 4), (2, 257, 4)])
def test_host_rule_on_generated_chains(shape):
    """The rho of the generator's chains — the z-scores and both indicators of
    every element — through the host rule, rtol 1e-12."""
    C, S, Dn = shape
    x = RD.ar1_chains(100, C, S, Dn)
    seen = 0
    for d in range(Dn):
        y = RD.split(x[:, :, d])
        m, n = y.shape
        q05, q95 = np.percentile(y.ravel(), 5.0), np.percentile(y.ravel(), 95.0)
        for series in (RD.zscores(y), (y <= q05).astype(np.float64),
                       (y <= q95).astype(np.float64)):
            rho, W = RD.rhos(series)
            if rho is None:
                continue
            ref, _ = RD.geyer(rho, n, m * n)
            np.testing.assert_allclose(_host_ess(rho, n, m * n), ref, rtol=1e-12, atol=0)
            seen += 1
    assert seen >= 2 * Dn


def test_host_rule_validation():
    lib = _lib.load()
    out = ctypes.c_double()
    r = np.zeros(3)
    p = r.ctypes.data_as(ctypes.c_void_p)
    assert lib.mc_geyer_ess_host(p, 3, 6, ctypes.byref(out)) == _lib.MC_ERR_INVALID
    assert lib.mc_geyer_ess_host(None, 4, 8, ctypes.byref(out)) == _lib.MC_ERR_INVALID
    assert lib.mc_geyer_ess_host(p, 4, 8, None) == _lib.MC_ERR_INVALID


def test_new_symbols_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "mcmc355.h")).read()
    lib = _lib.load()
    bound = {n for n, _, _ in _lib.SIGNATURES}
    for name in NEW:
        assert re.search(r"^\s*[a-z0-9_]+\s+%s\s*\(" % name, text, flags=re.M), name
        assert hasattr(lib, name), name
        assert name in bound, name
    assert re.search(r"#define\s+MC_ABI_VERSION\s+2\b", text)
    assert lib.mc_abi_version() == 2
    for k, f in enumerate(("RHAT_BULK", "RHAT_FOLDED", "RHAT_RANK", "ESS_BULK", "ESS_TAIL",
                           "CONSTANT", "COUNT")):
        assert re.search(r"#define\s+MC_RD_%s\s+%d\b" % (f, k), text), f
        assert getattr(_lib, "MC_RD_" + f) == k


def test_workspace_and_path_switch_without_a_device():
    lib = _lib.load()
    assert lib.mc_rank_diag_workspace_bytes(0, 10, 1) == _lib.MC_ERR_INVALID
    assert lib.mc_rank_diag_workspace_bytes(4, 1 << 30, 1) == _lib.MC_ERR_UNSUPPORTED
    assert b"2^31" in lib.mc_last_error()
    one = lib.mc_rank_diag_workspace_bytes(4, 130, 1)
    seven = lib.mc_rank_diag_workspace_bytes(4, 130, 7)
    assert 0 < one < seven
    # the benchmark's buffer is ranked in batches: the workspace stays under the cap
    assert lib.mc_rank_diag_workspace_bytes(256, 1000, 1000) <= 512 << 20
    assert lib.mc_debug_rank_path(2) == 0
    try:
        assert lib.mc_rank_diag_workspace_bytes(4, 130, 7) == \
            lib.mc_rank_diag_workspace_bytes(4, 130, 3)
    finally:
        assert lib.mc_debug_rank_path(0) == 2
    assert lib.mc_rank_diag(0, 8, 1, None, None, None, None, 0, None) == _lib.MC_ERR_INVALID


def test_rank_diagnostics_refuses_a_multi_rank_group(monkeypatch):
    import torch.distributed as dist

    monkeypatch.setattr(dist, "is_available", lambda: True)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    # (before any launch: no device is needed to be refused)
    monkeypatch.setattr(D, "_as_device", lambda s: pytest.fail("reached the device"))
    with pytest.raises(ValueError, match="every chain's draws"):
        D.rank_diagnostics(np.zeros((2, 8, 1), np.float32))


def test_diagnostics_before_run_raises():
    import mlx_mcmc_amd as m

    mc = m.MCMC(lambda p: m.Normal(0, 1).log_prob(p["x"]))
    with pytest.raises(ValueError, match="Must run sampling first"):
        mc.diagnostics(rank_normalized=True)
