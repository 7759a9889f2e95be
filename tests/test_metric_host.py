"""The diagonal mass matrix without a GPU: the warmup window schedule
(mc_metric_schedule, csrc/metric.h) against a restatement written here, the
validation of mc_metric_init on a host-only program, the metric buffer's
layout, and the shape checks of ``hmc`` / ``nuts`` before any device work."""
import ctypes

import numpy as np
import pytest

import workloads as W
from mlx_mcmc_amd import _lib


def window_ends(W_):
    """Stan's windowed warmup: init 75 / term 50 / base 25 (scaled to 15 % /
    10 % / the rest when they do not fit), windows doubling from `init`, the
    last one stretched to W - term when the next would not fit."""
    if W_ < 20:
        return []
    init, term, base = 75, 50, 25
    if init + term + base > W_:
        init, term = (15 * W_) // 100, W_ // 10
        base = W_ - init - term
    stop = W_ - term
    ends, start, length = [], init, base
    while start < stop:
        end = start + length
        if end + 2 * length > stop:
            end = stop
        ends.append(end)
        start, length = end, 2 * length
    return ends


def lib_ends(W_):
    lib = _lib.load()
    buf = (ctypes.c_int64 * 64)()
    n = lib.mc_metric_schedule(W_, buf, 64)
    assert n == lib.mc_metric_schedule(W_, None, 0)   # the count alone
    return list(buf[:n])


def test_schedule_pinned_values():
    assert window_ends(1000) == [100, 150, 250, 450, 950]
    assert window_ends(19) == []
    assert window_ends(150) == [100]
    assert window_ends(100) == [90]


@pytest.mark.parametrize("num_warmup", [1000, 150, 100, 19, 0, 20, 149, 151, 500, 2000, 12345])
def test_schedule_matches_restatement(num_warmup):
    assert lib_ends(num_warmup) == window_ends(num_warmup)


def _host_program(D=3):
    """An isotropic Normal over D parameters, host tables only."""
    from mlx_mcmc_amd import _trace

    lp, init = W.iso_normal(W.ns_product(), D)
    model = _trace.trace(lp, init)
    lib = _lib.load()
    h = ctypes.c_void_p()
    data = np.ascontiguousarray(model.data, np.float32)
    index = np.ascontiguousarray(model.index, np.int32)
    lib.mc_debug_program_host_only(1)
    try:
        _lib.check(lib.mc_program_create_expr(
            model.c_terms, len(model.terms), model.c_affines, model.n_affines, model.c_exprs,
            model.n_exprs, model.c_nodes, model.n_nodes, model.layout.size, model.lp_const,
            data.ctypes.data_as(ctypes.c_void_p), data.size,
            index.ctypes.data_as(ctypes.c_void_p), index.size, ctypes.byref(h)))
    finally:
        lib.mc_debug_program_host_only(0)
    return h


def _init(h, C, minv, bcast):
    lib = _lib.load()
    buf = np.zeros(lib.mc_metric_bytes(h, C), np.uint8)
    src = None if minv is None else np.ascontiguousarray(minv, np.float32)
    rc = lib.mc_metric_init(h, C, None if src is None else src.ctypes.data_as(ctypes.c_void_p),
                            bcast, buf.ctypes.data_as(ctypes.c_void_p), None)
    return rc, buf


def _sections(h, C, D, buf):
    lib = _lib.load()
    offs = [ctypes.c_int64() for _ in range(4)]
    _lib.check(lib.mc_metric_offsets(h, C, *[ctypes.byref(o) for o in offs]))
    return [buf[o.value:o.value + 4 * C * D].view(np.float32).reshape(C, D) for o in offs]


@pytest.mark.parametrize("bad", [0.0, -1.0, np.nan, np.inf])
def test_metric_init_rejects_bad_entries(bad):
    lib = _lib.load()
    h = _host_program(3)
    try:
        rc, _ = _init(h, 2, [1.0, bad, 2.0], 1)
        assert rc == _lib.MC_ERR_INVALID and b"finite and positive" in lib.mc_last_error()
        full = np.ones((2, 3), np.float32)
        full[1, 2] = bad
        rc, _ = _init(h, 2, full, 0)
        assert rc == _lib.MC_ERR_INVALID and b"chain 1, element 2" in lib.mc_last_error()
    finally:
        lib.mc_program_destroy(h)


def test_metric_init_layout_and_values():
    lib = _lib.load()
    C, D = 3, 5
    h = _host_program(D)
    try:
        offs = [ctypes.c_int64() for _ in range(4)]
        _lib.check(lib.mc_metric_offsets(h, C, *[ctypes.byref(o) for o in offs]))
        o = [x.value for x in offs]
        assert o[0] >= C * ctypes.sizeof(_lib.McMetricScalars)
        assert all(x % 256 == 0 for x in o) and all(b - a >= 4 * C * D for a, b in zip(o, o[1:]))
        assert lib.mc_metric_bytes(h, C) >= o[3] + 4 * C * D
        # NULL: ones
        rc, buf = _init(h, C, None, 0)
        assert rc == 0
        minv, msqrt, mean, m2 = _sections(h, C, D, buf)
        assert np.all(minv == 1) and np.all(msqrt == 1) and not mean.any() and not m2.any()
        assert not buf[:o[0]].any()                     # window count, updates, origin: zero
        # one vector for every chain, and a matrix
        v = np.array([0.25, 1.0, 4.0, 1e-3, 9.0], np.float32)
        rc, buf = _init(h, C, v, 1)
        assert rc == 0
        minv, msqrt, _, _ = _sections(h, C, D, buf)
        np.testing.assert_array_equal(minv, np.broadcast_to(v, (C, D)))
        np.testing.assert_array_equal(msqrt, np.broadcast_to(np.float32(1) / np.sqrt(v), (C, D)))
        m = (np.arange(C * D, dtype=np.float32).reshape(C, D) + 1) / 4
        rc, buf = _init(h, C, m, 0)
        assert rc == 0
        np.testing.assert_array_equal(_sections(h, C, D, buf)[0], m)
    finally:
        lib.mc_program_destroy(h)


def test_metric_scalars_struct_matches_header(tmp_path):
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "lay.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcmc355.h"\n'
                   'int main(void) { printf("%zu %zu %zu\\n", sizeof(mc_metric_scalars), '
                   'offsetof(mc_metric_scalars, n_updates), offsetof(mc_metric_scalars, '
                   'da_origin)); return 0; }\n')
    exe = tmp_path / "lay"
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)],
                   check=True)
    size, o1, o2 = map(int, subprocess.run([str(exe)], capture_output=True,
                                           text=True).stdout.split())
    assert size == ctypes.sizeof(_lib.McMetricScalars)
    assert o1 == _lib.McMetricScalars.n_updates.offset
    assert o2 == _lib.McMetricScalars.da_origin.offset


@pytest.mark.parametrize("sampler", ["hmc", "nuts"])
@pytest.mark.parametrize("bad", [
    np.ones(4, np.float32),                       # D is 5
    np.ones((3, 5), np.float32),                  # num_chains is 2
    np.ones((2, 5, 1), np.float32),
    {"x": np.ones(4, np.float32)},                # the parameter's shape is (5,)
    {"y": np.ones(5, np.float32)},                # not a parameter
])
def test_wrong_shape_is_a_value_error_before_the_device(sampler, bad, monkeypatch):
    import mlx_mcmc_amd as m

    def no_device():
        raise AssertionError("the device was touched before the shape check")

    monkeypatch.setattr(_lib, "require_device", no_device)
    lp, init = W.iso_normal(W.ns_product(), 5)
    with pytest.raises(ValueError, match="inverse_mass_matrix"):
        getattr(m, sampler)(lp, init, num_samples=5, num_warmup=5, num_chains=2, progress=False,
                            inverse_mass_matrix=bad)


def test_non_positive_entry_is_a_value_error_before_the_device(monkeypatch):
    import mlx_mcmc_amd as m

    monkeypatch.setattr(_lib, "require_device", lambda: (_ for _ in ()).throw(AssertionError()))
    lp, init = W.iso_normal(W.ns_product(), 5)
    with pytest.raises(ValueError, match="finite and positive"):
        m.nuts(lp, init, num_samples=5, num_warmup=5, progress=False,
               inverse_mass_matrix=np.array([1, 1, 0, 1, 1], np.float32))


def test_shard_metric_cuts_per_chain_rows():
    from mlx_mcmc_amd import distributed as dist

    m = np.arange(5 * 3, dtype=np.float32).reshape(5, 3) + 1
    rows = [dist.shard_metric(m, True, 5, 2, r)["inverse_mass_matrix"] for r in range(2)]
    np.testing.assert_array_equal(np.concatenate(rows), m)
    assert rows[0].shape[0] == 3
    v = np.ones(3, np.float32)
    kw = dist.shard_metric(v, False, 5, 2, 1)
    assert kw["inverse_mass_matrix"] is v and kw["adapt_mass_matrix"] is False
    assert dist.shard_metric(None, True, 5, 2, 0) == {"inverse_mass_matrix": None,
                                                      "adapt_mass_matrix": True}
    with pytest.raises(ValueError):
        dist.shard_metric(m, True, 6, 2, 0)
