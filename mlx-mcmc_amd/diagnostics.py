"""Sample diagnostics on the device.

Every statistic is computed by libmcmc355.so kernels (csrc/diag.h) on the
[C, S, D] sample buffer the samplers write; only per-element results (D
values) or a handful of order statistics come back to the host.

* ``compute_ess(samples)`` — the reference helper
  (examples/06_nuts_comparison.py:22-41) for one series: n / (1 + 2 sum rho_k)
  over lags 1 .. min(n//2, 100) - 1, stopping at (and including) the first
  rho < 0.05; n for a constant series.
* ``chain_diagnostics(samples)`` — per-series ESS (the same rule), ESS summed
  over chains and split R-hat (BDA3 eq. 11.4; the reference lists R-hat on its
  roadmap, README.md:214, without code) per element.  Under torch.distributed
  with chains sharded over ranks the reductions are two all-reduces of
  [2, D] f64 blocks — no sample leaves its GPU.
* ``summarize(samples, layout)`` — ``MCMC.summary`` (mcmc.py:191-227): pooled
  mean / std from per-series moments, median and percentiles from exact
  device order statistics, interpolated with numpy's own rule.

* ``pointwise_log_likelihood(log_likelihood, samples, layout)`` — for every
  observation of a likelihood traced like ``log_prob``, six mergeable
  statistics of its log-likelihood over the kept draws (mc_pointwise_stats,
  csrc/pointwise.h): the C x S x M matrix is never stored.  ``waic`` forms
  WAIC from them (Vehtari, Gelman and Gabry 2017); ``merge_pointwise`` is the
  host statement of the merge the device and the ranks apply.  Out of scope:
  the expression JIT for likelihoods (expression terms run the node
  interpreter).
* ``loo(log_likelihood, samples, layout)`` — PSIS-LOO of the same kind of
  likelihood (mc_psis_loo, csrc/psis.h): per observation an exact selection of
  the smallest log-likelihood values over all draws, a generalized Pareto fit
  and the smoothed leave-one-out estimate with its khat diagnostic, without
  the matrix.  ``compare`` differences two results observation by observation.
* ``posterior_predictive(log_likelihood, samples, layout)`` — for every
  observation of the same kind of likelihood, one replicate per kept draw from
  the term's own distribution at that draw (mc_predictive, csrc/predictive.h),
  reduced on the device to mergeable statistics: predictive mean and variance,
  and the fraction of replicates below the observation (a PIT value).  The
  C x S x M replicates are stored only on request.  ``merge_predictive`` is
  the host statement of the merge.

* ``rank_diagnostics(samples)`` — rank-normalised split R-hat (bulk, folded
  and the larger of the two), bulk-ESS and tail-ESS per element (Vehtari,
  Gelman, Simpson, Carpenter and Buerkner 2021; mc_rank_diag,
  csrc/rankdiag.h): exact pooled average ranks from a device radix sort, a
  multi-chain autocovariance with Geyer's truncation.  Pooled ranks need every
  chain on one device.

No CPU fallback: without the library these raise ``EngineUnavailable``
(``merge_pointwise``, ``merge_predictive``, ``waic_from_stats`` and ``compare``
are pure host arithmetic).
"""
from __future__ import annotations

import ctypes
from typing import Dict

import numpy as np

from . import _lib

MAX_LAG = 100   # examples/06_nuts_comparison.py:33


def _as_device(samples):
    """[C, S, D] f32 contiguous device tensor from a tensor or array of
    shape [S], [S, D] (one chain) or [C, S, D]."""
    import torch

    dev = _lib.require_device()
    t = samples if isinstance(samples, torch.Tensor) else torch.from_numpy(
        np.array(samples, dtype=np.float32, copy=True))
    t = t.to(device=dev, dtype=torch.float32)
    if t.dim() == 1:
        t = t[None, :, None]
    elif t.dim() == 2:
        t = t[None]
    elif t.dim() != 3:
        raise ValueError("samples must be [S], [S, D] or [C, S, D]")
    return t.contiguous()


def series_stats(samples, max_lag: int = MAX_LAG):
    """mc_series_stats: [MC_ST_COUNT, C*D] f64 device tensor (fields in _lib.MC_ST_*)."""
    import torch

    x = _as_device(samples)
    C, S, D = x.shape
    st = torch.empty((_lib.MC_ST_COUNT, C * D), dtype=torch.float64, device=x.device)
    lib = _lib.load()
    _lib.check(lib.mc_series_stats(C, S, D, _lib.ptr(x), int(max_lag), _lib.ptr(st),
                                   _lib.stream_handle()))
    return st


def compute_ess(samples) -> float:
    """Reference ``compute_ess`` of one 1-D series, evaluated on the device."""
    x = np.asarray(samples)
    if x.ndim != 1:
        raise ValueError("compute_ess takes one 1-D series")
    if len(x) == 0:
        raise ValueError("empty series")
    return float(series_stats(x)[_lib.MC_ST_ESS, 0].item())


def ess(samples, max_lag: int = MAX_LAG):
    """Per-series ESS, [C, D] f64 numpy (reference rule for every chain and element)."""
    x = _as_device(samples)
    C, S, D = x.shape
    return series_stats(x, max_lag)[_lib.MC_ST_ESS].view(C, D).cpu().numpy()


def _all_reduce(t, group):
    import torch.distributed as dist

    if group is not False and dist.is_available() and dist.is_initialized() \
            and dist.get_world_size(group) > 1:
        if dist.get_backend(group) == "gloo" and t.is_cuda:
            # gloo (a CPU rehearsal of the RCCL path): reduce a host copy
            h = t.cpu()
            dist.all_reduce(h, group=group)
            t.copy_(h)
        else:
            dist.all_reduce(t, group=group)
    return t


def chain_diagnostics(samples, max_lag: int = MAX_LAG, group=None) -> Dict[str, np.ndarray]:
    """ESS and split R-hat per element of a [C, S, D] buffer.

    Returns ``ess`` [C, D] (this rank's chains), ``ess_sum`` [D] (summed over
    every chain of every rank), ``rhat`` [D] (NaN unless S >= 4),
    ``n_constant`` (series of zero variance over all ranks) and
    ``n_nonpositive_ess`` (per-chain ESS values <= 0 over all ranks).  With an
    initialised process group (pass ``group=False`` to stay local) the chain
    sums are all-reduced over the ranks' shards.
    """
    import torch

    x = _as_device(samples)
    C, S, D = x.shape
    lib = _lib.load()
    stream = _lib.stream_handle()
    # a rank whose shard holds no chain (e.g. every one of its chains was
    # left out as frozen) still joins the all-reduces with zero blocks
    st = series_stats(x, max_lag) if C > 0 else torch.zeros(
        (_lib.MC_ST_COUNT, 0), dtype=torch.float64, device=x.device)
    red = torch.zeros((2, D), dtype=torch.float64, device=x.device)
    if C > 0:
        _lib.check(lib.mc_stats_reduce(C, S, D, _lib.ptr(st), None, 0, _lib.ptr(red), stream))
    # [split chains, constant series]: a constant series scores ESS = n by
    # the reference rule, so callers need to know how many there are
    # and non-positive per-chain ESS values (the reference rule on antithetic
    # draws): every rank's count, so every rank takes the same branch on them
    counts = torch.stack([torch.tensor(2.0 * C, dtype=torch.float64, device=x.device),
                          (st[_lib.MC_ST_M2] == 0).sum().to(torch.float64),
                          (st[_lib.MC_ST_ESS] <= 0).sum().to(torch.float64)])
    _all_reduce(red, group)
    _all_reduce(counts, group)
    ess_sum = red[1].clone()
    rhat = torch.full((D,), float("nan"), dtype=torch.float64, device=x.device)
    m_total, n_const, n_nonpos = (int(v) for v in counts.tolist())
    m = m_total
    if S >= 4 and m >= 2:
        center = red[0].contiguous()
        spread = torch.zeros((2, D), dtype=torch.float64, device=x.device)
        if C > 0:
            _lib.check(lib.mc_stats_reduce(C, S, D, _lib.ptr(st), _lib.ptr(center), m,
                                           _lib.ptr(spread), stream))
        _all_reduce(spread, group)
        _lib.check(lib.mc_rhat(D, m, S, _lib.ptr(spread), _lib.ptr(rhat), stream))
    return {"ess": st[_lib.MC_ST_ESS].view(C, D).cpu().numpy(),
            "ess_sum": ess_sum.cpu().numpy(), "rhat": rhat.cpu().numpy(),
            "n_constant": n_const, "n_nonpositive_ess": n_nonpos}


RANK_FIELDS = ("rhat_bulk", "rhat_folded", "rhat_rank", "ess_bulk", "ess_tail")


def rank_diagnostics(samples, group=None, *, z_scores=False) -> Dict[str, np.ndarray]:
    """Rank-normalised split R-hat, bulk-ESS and tail-ESS per element of a
    [C, S, D] buffer (Vehtari et al. 2021; the definition is stated in
    include/mcmc355.h, mc_rank_diag).

    Every chain is split in halves of n = S // 2 draws (the middle draw of an
    odd S is dropped); the N = 2 C n split draws of an element are ranked
    (average ranks) and mapped to normal scores z.  Returns float64 [D] arrays
    ``rhat_bulk`` (split R-hat of z), ``rhat_folded`` (of the z of
    |y - median|), ``rhat_rank`` (the larger), ``ess_bulk`` (Stan's ESS of z)
    and ``ess_tail`` (the smaller ESS of the indicators y <= q05, y <= q95),
    plus ``n_constant``, the count of constant elements.  NaN where nothing is
    defined: S < 8, an element with a NaN draw, a constant element or
    indicator.  ``z_scores=True`` adds ``z``, the [D, 2C, n] float64 device
    tensor of the bulk z-scores (small problems only).

    Pooled ranks need every chain's draws on one device: with an initialised
    process group of more than one rank this raises ``ValueError`` unless
    ``group=False`` (this rank's chains alone)."""
    import torch

    _refuse_sharded_draws(group, "rank-normalised diagnostics are not mergeable over shards of "
                          "chains: an element's ranks are taken over every chain's draws; gather "
                          "the chains on one rank, or pass group=False for this rank's chains "
                          "alone")
    x = _as_device(samples)
    C, S, D = x.shape
    lib = _lib.load()
    nb = lib.mc_rank_diag_workspace_bytes(C, S, D)
    if nb < 0:
        _lib.check(int(nb))
    n = S // 2
    out = torch.empty((_lib.MC_RD_COUNT, D), dtype=torch.float64, device=x.device)
    z = torch.empty((D, 2 * C, n), dtype=torch.float64, device=x.device) if z_scores else None
    ws = torch.empty(max(int(nb), 8), dtype=torch.uint8, device=x.device)
    _lib.check(lib.mc_rank_diag(C, S, D, _lib.ptr(x), _lib.ptr(out), _lib.ptr(z), _lib.ptr(ws),
                                nb, _lib.stream_handle()))
    host = out.cpu().numpy()   # (synchronises: x and ws outlive the launch)
    res = {f: host[k].copy() for k, f in enumerate(RANK_FIELDS)}
    res["n_constant"] = int(host[_lib.MC_RD_CONSTANT].sum())
    if z_scores:
        res["z"] = z
    return res


# ------------------------------------------------------------ summary -----
def order_statistics(x, off: int, length: int, ranks):
    """Exact k-th smallest pooled values of elements [off, off+length) of a
    device [C, S, D] buffer (mc_select), as float32; NaN if any value is NaN."""
    import torch

    C, S, D = x.shape
    ranks = [int(r) for r in ranks]
    lib = _lib.load()
    out = torch.empty(len(ranks), dtype=torch.float32, device=x.device)
    for i in range(0, len(ranks), 8):
        chunk = ranks[i:i + 8]
        nb = lib.mc_select_workspace_bytes(len(chunk))
        ws = torch.empty(nb, dtype=torch.uint8, device=x.device)
        karr = (ctypes.c_int64 * len(chunk))(*chunk)
        o = out[i:i + len(chunk)]
        _lib.check(lib.mc_select(C, S, D, _lib.ptr(x), off, length, len(chunk), karr,
                                 _lib.ptr(o), _lib.ptr(ws), nb, _lib.stream_handle()))
    return out.cpu().numpy()


def _percentile_ranks(n: int, q: float):
    """numpy's 'linear' percentile (np.percentile, numpy 2.x): the virtual
    index (n - 1) * (q / 100) is formed in the data dtype (float32 here)."""
    q32 = np.true_divide(np.asarray(q, np.float32), np.float32(100))
    vi = np.asarray((n - 1) * q32)
    if vi >= n - 1:      # _get_indexes: above the last index -> the maximum
        return n - 1, n - 1, np.asarray(0.0, vi.dtype)
    prev = np.floor(vi)
    gamma = np.asarray(vi - prev, dtype=vi.dtype)
    return int(prev), int(prev) + 1, gamma


def _lerp(a, b, t):
    """numpy's _lerp (numpy/lib/_function_base_impl.py) on float32 bounds."""
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    diff = np.subtract(b, a)
    r = np.add(a, diff * t)
    if t >= 0.5:
        r = np.subtract(b, diff * (1 - t))
    return r[()]


def quantiles_from_order_stats(n: int, lower_pct: float, upper_pct: float, fetch):
    """(median, lower, upper) exactly as np.median / np.percentile return them
    for n float32 values, given ``fetch(ranks) -> values`` of the sorted pool."""
    lo = _percentile_ranks(n, lower_pct)
    hi = _percentile_ranks(n, upper_pct)
    mid = [(n - 1) // 2, n // 2]
    ranks = sorted({lo[0], lo[1], hi[0], hi[1], *mid})
    vals = dict(zip(ranks, fetch(ranks)))
    a, b = np.float32(vals[mid[0]]), np.float32(vals[mid[1]])
    median = a if n % 2 else np.float32(np.float32(a + b) / 2)   # np.median: f32 mean of two
    return (median, _lerp(vals[lo[0]], vals[lo[1]], lo[2]),
            _lerp(vals[hi[0]], vals[hi[1]], hi[2]))


def summarize(samples, layout=None, credible_interval: float = 0.95) -> Dict[str, dict]:
    """``MCMC.summary`` (mcmc.py:191-227) from device statistics.

    ``samples``: a [C, S, D] device tensor with ``layout`` (names, shapes,
    offsets of the flattened elements), or a dict name -> array as
    ``MCMC.samples`` holds it.  Every value of a parameter (all chains, draws
    and vector elements) is pooled, exactly as np.mean(s) etc. pool them.
    """
    import torch

    alpha = 1 - credible_interval
    lower_pct = 100 * alpha / 2
    upper_pct = 100 * (1 - alpha / 2)
    if isinstance(samples, dict):
        # the pool is every value; its columns (last axis) become the series
        items = []
        for name, a in samples.items():
            a = np.asarray(a, np.float32)
            w = a.shape[-1] if a.ndim >= 2 else 1
            items.append((name, _as_device(a.reshape(1, -1, w)), 0, w))
    else:
        if layout is None:
            raise ValueError("a [C, S, D] buffer needs its layout")
        x = _as_device(samples)
        items = [(name, x, int(off), int(np.prod(shape)) if shape else 1)
                 for name, shape, off in zip(layout.names, layout.shapes, layout.offsets)]
    out: Dict[str, dict] = {}
    lib = _lib.load()
    for name, x, off, length in items:
        C, S, D = x.shape
        st = series_stats(x)
        mom = torch.empty(2, dtype=torch.float64, device=x.device)
        _lib.check(lib.mc_pool_moments(C, S, D, _lib.ptr(st), off, length, _lib.ptr(mom),
                                       _lib.stream_handle()))
        mean, std = mom.cpu().numpy().tolist()
        med, lo, hi = quantiles_from_order_stats(
            C * S * length, lower_pct, upper_pct,
            lambda ranks: order_statistics(x, off, length, ranks))
        out[name] = {
            'mean': float(mean),
            'std': float(std),
            'median': float(med),
            f'{lower_pct:.1f}%': float(lo),
            f'{upper_pct:.1f}%': float(hi),
        }
    return out


# ------------------------------------------------- pointwise / WAIC -----
PW_FIELDS = ("max", "sumexp", "n", "mean", "m2", "nonfinite")


def merge_pointwise(parts):
    """Merge pointwise partials (dicts of the six [M] float64 arrays of
    ``pointwise_log_likelihood``, each over its own shard of draws) in order.

    max / rescale for ``max`` and ``sumexp``, Chan's update for ``mean`` and
    ``m2``; where a side holds a non-finite draw, ``mean`` is the sum of the
    sides' non-finite means (-inf, +inf or NaN, as np.mean of the whole gives)
    and ``m2`` is NaN (as np.var gives).  The device merge (csrc/pointwise.h
    pw_merge) and the rank merge apply the same rules."""
    parts = list(parts)
    if not parts:
        raise ValueError("merge_pointwise needs at least one partial")
    acc = {f: np.array(parts[0][f], dtype=np.float64, copy=True) for f in PW_FIELDS}
    with np.errstate(all="ignore"):
        for p in parts[1:]:
            b = {f: np.asarray(p[f], np.float64) for f in PW_FIELDS}
            am, bm = acc["max"], b["max"]
            m = np.where((bm > am) | np.isnan(bm), bm, am)
            sa = np.where(am == m, acc["sumexp"], acc["sumexp"] * np.exp(am - m))
            sb = np.where(bm == m, b["sumexp"], b["sumexp"] * np.exp(bm - m))
            na, nb = acc["n"], b["n"]
            n = na + nb
            anf, bnf = acc["nonfinite"] > 0, b["nonfinite"] > 0
            d = b["mean"] - acc["mean"]
            r = 1.0 / n
            mean = acc["mean"] + d * (nb * r)
            m2 = acc["m2"] + (b["m2"] + d * d * (na * nb * r))
            cls = np.where(anf, np.where(bnf, acc["mean"] + b["mean"], acc["mean"]), b["mean"])
            nf = anf | bnf
            acc = {"max": m, "sumexp": sa + sb, "n": n,
                   "mean": np.where(nf, cls, mean), "m2": np.where(nf, np.nan, m2),
                   "nonfinite": acc["nonfinite"] + b["nonfinite"]}
    return acc


def _gather_parts(part, group):
    """Every rank's partial, in rank order (one rank: the partial itself)."""
    import torch.distributed as dist

    if group is False or not (dist.is_available() and dist.is_initialized()) \
            or dist.get_world_size(group) <= 1:
        return [part]
    out = [None] * dist.get_world_size(group)
    dist.all_gather_object(out, part, group=group)
    return out


def _pointwise_inputs(samples, layout):
    """([C, S, D] device tensor, layout) from a device buffer with its layout,
    or from a dict name -> array as ``MCMC.samples`` holds it: [C, S, *shape],
    or [S, *shape] for one chain.  Without a layout the parameter shapes are
    what follows the leading axes: one chain when some array is 1-D, else
    [C, S, ...] (pass the run's layout for one chain of vector parameters)."""
    from . import _trace

    if not isinstance(samples, dict):
        if layout is None:
            raise ValueError("a [C, S, D] buffer needs its layout")
        x = _as_device(samples)
        if x.shape[2] != layout.size:
            raise ValueError(f"samples have {x.shape[2]} elements per draw, the layout "
                             f"{layout.size}")
        return x, layout
    arrs = {k: np.asarray(_trace._to_numpy(v), np.float32) for k, v in samples.items()}
    if not arrs:
        raise ValueError("samples is empty")
    if layout is not None:
        lead = {a.ndim - len(shp) for a, shp in
                ((arrs[n], s) for n, s in zip(layout.names, layout.shapes))}
        if len(lead) != 1 or lead not in ({1}, {2}):
            raise ValueError("samples do not match the layout's parameter shapes")
        lead = lead.pop()
        names = layout.names
    else:
        lead = 1 if min(a.ndim for a in arrs.values()) == 1 else 2
        names = list(arrs)
    first = arrs[names[0]]
    C, S = (1, first.shape[0]) if lead == 1 else first.shape[:2]
    cols = []
    for n in names:
        a = arrs[n]
        if a.shape[:lead] != first.shape[:lead]:
            raise ValueError(f"parameter '{n}' has leading shape {a.shape[:lead]}, expected "
                             f"{first.shape[:lead]}")
        cols.append(a.reshape(C, S, -1))
    lay = _trace.layout_of({n: np.zeros(arrs[n].shape[lead:], np.float32) for n in names})
    if layout is not None and list(lay.shapes) != [tuple(s) for s in layout.shapes]:
        raise ValueError("samples do not match the layout's parameter shapes")
    return _as_device(np.concatenate(cols, axis=2)), lay


def _pointwise_launch(prog, x, matrix=False):
    """mc_pointwise_stats of a pointwise program on the [C, S, D] device
    buffer: (this rank's partial, the matrix tensor or None)."""
    import torch

    C, S, D = x.shape
    lib = _lib.load()
    M = prog.num_elements
    st = torch.empty((_lib.MC_PW_COUNT, M), dtype=torch.float64, device=x.device)
    mat = torch.empty((C, S, M), dtype=torch.float32, device=x.device) if matrix else None
    nb = lib.mc_pointwise_workspace_bytes(prog.handle, C, S)
    if nb < 0:
        _lib.check(int(nb))
    ws = torch.empty(max(int(nb), 1), dtype=torch.uint8, device=x.device)
    _lib.check(lib.mc_pointwise_stats(prog.handle, C, S, _lib.ptr(x), _lib.ptr(st),
                                      _lib.ptr(mat), _lib.ptr(ws), nb, _lib.stream_handle()))
    host = st.cpu().numpy()   # (synchronises: prog, x and ws outlive the launch)
    return {f: host[k].copy() for k, f in enumerate(PW_FIELDS)}, mat


def pointwise_log_likelihood(log_likelihood_fn, samples, layout=None, *, matrix=False,
                             group=None):
    """Per-observation log-likelihood statistics over the kept draws.

    ``log_likelihood_fn(params)`` is written and traced exactly like
    ``log_prob`` and returns a scalar, normally
    ``mx.sum(Dist(...).log_prob(y))``.  Every element of every term of that
    trace is one observation, term by term in trace order and inside a term in
    the user's element order (M in all); the value of element i of term t is
    ``weight_t * lp_{t,i}`` as one f32 product (``mx.mean`` scales every
    observation by 1 / n).  Constants added to the likelihood belong to no
    observation and are left out; nothing guesses which terms of a ``log_prob``
    are observed — pass the likelihood alone.

    ``samples``: a [C, S, D] device tensor with its ``layout``, or a dict name
    -> array as ``MCMC.samples`` holds it.  Returns the six statistics
    (``max``, ``sumexp`` = sum exp(x - max), ``n``, ``mean``, ``m2``,
    ``nonfinite``) as float64 NumPy [M] arrays — a partial ``merge_pointwise``
    can combine with other shards of draws — plus ``matrix``, the [C, S, M]
    float32 device tensor of every value, when ``matrix=True`` (small problems
    only).  With an initialised process group (``group=False`` stays local)
    the ranks' partials are gathered and merged in rank order; the matrix
    stays this rank's."""
    import torch

    from . import _trace

    x, lay = _pointwise_inputs(samples, layout)
    part, mat = _pointwise_launch(_trace.pointwise_program(log_likelihood_fn, lay), x, matrix)
    out = merge_pointwise(_gather_parts(part, group))
    if matrix:
        out["matrix"] = mat
    return out


def waic_from_stats(stats) -> dict:
    """WAIC (Vehtari, Gelman and Gabry 2017) from the pointwise statistics:
    lppd_i = log(sumexp) + max - log n, p_waic_i = m2 / (n - 1) (the sample
    variance, NaN for one draw), elpd_i = lppd_i - p_waic_i."""
    with np.errstate(all="ignore"):
        n = np.asarray(stats["n"], np.float64)
        lppd_i = np.log(stats["sumexp"]) + stats["max"] - np.log(n)
        p_i = np.asarray(stats["m2"], np.float64) / (n - 1.0)
        elpd_i = lppd_i - p_i
        m = elpd_i.size
        elpd = float(np.sum(elpd_i))
        return {"elpd_waic": elpd, "p_waic": float(np.sum(p_i)), "waic": -2.0 * elpd,
                "se": float(np.sqrt(m * np.var(elpd_i))), "lppd": float(np.sum(lppd_i)),
                "pointwise": {"lppd": lppd_i, "p_waic": p_i, "elpd_waic": elpd_i},
                "n_obs": int(m), "n_draws": int(n.max()) if m else 0,
                "n_high_p_waic": int(np.sum(p_i > 0.4)),
                "n_nonfinite": int(np.sum(stats["nonfinite"]))}


def waic(log_likelihood_fn, samples, layout=None, *, group=None) -> dict:
    """WAIC of a likelihood over the kept draws (``pointwise_log_likelihood``'s
    arguments): ``elpd_waic``, ``p_waic``, ``waic`` (= -2 elpd), ``se``
    (= sqrt(M var_i elpd_i)), ``lppd``, the ``pointwise`` terms, ``n_obs``,
    ``n_draws``, ``n_high_p_waic`` (observations with p_waic_i > 0.4, where
    WAIC is unreliable) and ``n_nonfinite`` (draws outside an observation's
    support: reported, never raised)."""
    return waic_from_stats(pointwise_log_likelihood(log_likelihood_fn, samples, layout,
                                                    group=group))


# ------------------------------------------------------------ PSIS-LOO -----
def _refuse_sharded_draws(group, why=None):
    import torch.distributed as dist

    if group is not False and dist.is_available() and dist.is_initialized() \
            and dist.get_world_size(group) > 1:
        raise ValueError(why or
                         "PSIS-LOO is not mergeable over shards of draws: an observation's "
                         "tail is taken over all draws; gather the draws on one rank, or pass "
                         "group=False for this rank's draws alone")


def loo(log_likelihood_fn, samples, layout=None, *, r_eff=1.0, tail=False, group=None) -> dict:
    """PSIS-LOO (Vehtari, Gelman and Gabry 2017) of a likelihood over the kept
    draws, on the device (``pointwise_log_likelihood``'s arguments;
    mc_psis_loo, csrc/psis.h; the definition is stated in include/mcmc355.h).

    Per observation the ``tail_len`` smallest log-likelihood values over all
    draws are selected exactly, a generalized Pareto distribution is fitted to
    the importance ratios they imply and the tail's weights are replaced by
    its quantiles; the C x S x M matrix is never stored.  ``r_eff`` is the
    relative efficiency of the draws (a positive scalar) and only sets the
    tail length.

    Returns ``elpd_loo``, ``p_loo`` (= lppd - elpd_loo), ``looic``
    (= -2 elpd_loo), ``se`` (= sqrt(M var_i elpd_loo_i)), ``lppd``, the
    ``pointwise`` terms (``elpd_loo``, ``p_loo``, ``lppd``, ``khat``),
    ``n_obs``, ``n_draws``, ``tail_len``, ``n_high_k`` (observations with
    khat > 0.7, where the estimate is unreliable; +inf, a tail of at most four
    distinct values, included) and ``n_nonfinite`` (draws outside an
    observation's support: that observation's terms are NaN; reported, never
    raised).  ``tail=True`` adds ``tail``, the [M, tail_len] float32 device
    tensor of every observation's tail in ascending order (NaN past its
    length), with ``cutoff``, ``min``, ``sigma`` and ``tail_n`` per observation.

    PSIS is not mergeable over shards of draws: with an initialised process
    group of more than one rank this raises ``ValueError`` unless
    ``group=False`` (this rank's draws alone)."""
    import torch

    from . import _trace

    _refuse_sharded_draws(group)
    r_eff = float(r_eff)
    if not (r_eff > 0.0 and np.isfinite(r_eff)):
        raise ValueError("r_eff must be a positive finite scalar")
    x, lay = _pointwise_inputs(samples, layout)
    C, S, D = x.shape
    prog = _trace.pointwise_program(log_likelihood_fn, lay)
    stats, _ = _pointwise_launch(prog, x)
    lib = _lib.load()
    M = prog.num_elements
    nb = lib.mc_psis_workspace_bytes(prog.handle, C, S, r_eff)
    if nb < 0:   # (a tail beyond the kernel's capacity is reported here: nothing is launched)
        _lib.check(int(nb))
    mt = int(lib.mc_psis_tail_len(C * S, r_eff))
    out = torch.empty((_lib.MC_PSIS_COUNT, M), dtype=torch.float64, device=x.device)
    tl = torch.empty((M, mt), dtype=torch.float32, device=x.device) if tail else None
    ws = torch.empty(max(int(nb), 8), dtype=torch.uint8, device=x.device)
    _lib.check(lib.mc_psis_loo(prog.handle, C, S, r_eff, _lib.ptr(x), _lib.ptr(out),
                               _lib.ptr(tl), _lib.ptr(ws), nb, _lib.stream_handle()))
    host = out.cpu().numpy()   # (synchronises: prog, x and ws outlive the launch)
    with np.errstate(all="ignore"):
        lppd_i = np.log(stats["sumexp"]) + stats["max"] - np.log(stats["n"])
        elpd_i = host[_lib.MC_PSIS_ELPD].copy()
        khat = host[_lib.MC_PSIS_KHAT].copy()
        p_i = lppd_i - elpd_i
        elpd, lppd = float(np.sum(elpd_i)), float(np.sum(lppd_i))
        res = {"elpd_loo": elpd, "p_loo": lppd - elpd, "looic": -2.0 * elpd,
               "se": float(np.sqrt(M * np.var(elpd_i))), "lppd": lppd,
               "pointwise": {"elpd_loo": elpd_i, "p_loo": p_i, "lppd": lppd_i, "khat": khat},
               "n_obs": int(M), "n_draws": int(C * S), "tail_len": mt,
               "n_high_k": int(np.sum(khat > 0.7)),
               "n_nonfinite": int(np.sum(stats["nonfinite"]))}
    if tail:
        res.update(tail=tl, cutoff=host[_lib.MC_PSIS_CUTOFF].copy(),
                   min=host[_lib.MC_PSIS_MIN].copy(), sigma=host[_lib.MC_PSIS_SIGMA].copy(),
                   tail_n=host[_lib.MC_PSIS_TAILN].astype(np.int64))
    return res


def compare(a, b) -> dict:
    """Difference of two ``loo`` (or two ``waic``) results on the same
    observations: ``elpd_diff`` = sum_i (elpd_a_i - elpd_b_i) and ``se_diff``
    = sqrt(M var_i(diff_i)) (the population variance, as ``se``).  Pure host
    arithmetic."""
    key = "elpd_loo" if "elpd_loo" in a["pointwise"] else "elpd_waic"
    if key not in b["pointwise"]:
        raise ValueError("compare takes two loo results or two waic results")
    if a["n_obs"] != b["n_obs"]:
        raise ValueError(f"the results cover {a['n_obs']} and {b['n_obs']} observations")
    with np.errstate(all="ignore"):
        d = np.asarray(a["pointwise"][key], np.float64) - np.asarray(b["pointwise"][key],
                                                                     np.float64)
        return {"elpd_diff": float(np.sum(d)), "se_diff": float(np.sqrt(d.size * np.var(d))),
                "n_obs": int(d.size)}


# ------------------------------------------------- posterior predictive -----
PP_FIELDS =("n", "mean", "m2", "below", "nonfinite")


def merge_predictive(parts):
    """Merge posterior predictive partials (dicts of the five [M] float64
    arrays ``n``, ``mean``, ``m2``, ``below``, ``nonfinite`` of
    ``posterior_predictive``, each over its own shard of draws) in order.

    ``mean`` and ``m2`` are moments of the finite replicates: Chan's update
    over the finite counts ``n - nonfinite`` (a side without finite replicates
    leaves the other's moments; both without: NaN), the three counts added.
    The device merge (csrc/predictive.h k_pp_merge) and the rank merge apply
    the same rules.  When every partial carries ``equal`` (the finite
    replicates equal to the observation: likelihoods with a count term), it is
    added too; otherwise the result has none."""
    parts = list(parts)
    if not parts:
        raise ValueError("merge_predictive needs at least one partial")
    equal = None
    if all("equal" in p for p in parts):
        equal = sum(np.asarray(p["equal"], np.float64) for p in parts)
    acc = {f: np.array(parts[0][f], dtype=np.float64, copy=True) for f in PP_FIELDS}
    with np.errstate(all="ignore"):
        for p in parts[1:]:
            b = {f: np.asarray(p[f], np.float64) for f in PP_FIELDS}
            na, nb = acc["n"] - acc["nonfinite"], b["n"] - b["nonfinite"]
            d = b["mean"] - acc["mean"]
            r = 1.0 / (na + nb)
            mean = acc["mean"] + d * (nb * r)
            m2 = acc["m2"] + (b["m2"] + d * d * (na * nb * r))
            keep, take = nb == 0, na == 0
            acc = {"n": acc["n"] + b["n"],
                   "mean": np.where(keep, acc["mean"], np.where(take, b["mean"], mean)),
                   "m2": np.where(keep, acc["m2"], np.where(take, b["m2"], m2)),
                   "below": acc["below"] + b["below"],
                   "nonfinite": acc["nonfinite"] + b["nonfinite"]}
    if equal is not None:
        acc["equal"] = np.array(equal, dtype=np.float64, copy=True)
    return acc


def posterior_predictive(log_likelihood_fn, samples, layout=None, *, seed=0, thin=1,
                         replicates=False, chain_offset=0, iter_offset=0, group=None):
    """Posterior predictive replicates and per-observation checks over the
    kept draws, on the device.

    ``log_likelihood_fn`` and ``samples`` / ``layout`` are those of
    ``pointwise_log_likelihood``: every element of every term of the traced
    likelihood is one observation.  For every processed draw (iterations 0,
    ``thin``, 2 ``thin``, ... of every chain: S' = ceil(S / thin)) and
    observation, one replicate is drawn from the term's distribution — Normal,
    HalfNormal, Exponential, Gamma or Beta, or the count distribution of a
    ``Bernoulli(logits=)`` / ``Binomial(n, logits=)`` / ``Poisson(log_rate=)``
    likelihood term, or the ``StudentT`` / ``Cauchy`` / ``HalfStudentT`` /
    ``HalfCauchy`` of such a term — with the operand values of that draw.  A replicate is a pure function of (``seed``, chain index +
    ``chain_offset``, iteration index + ``iter_offset``, observation) and those
    operand values (include/mcmc355.h), so shards of chains or iterations and
    thinned runs reproduce the rows of the whole.  A term's weight (``mx.mean``,
    a tempering factor) is ignored: replicates come from the untempered
    observation model.  Identity terms and every other expression term have no
    sampling distribution: ``EngineError`` (MC_ERR_UNSUPPORTED) before any
    launch.

    Returns float64 NumPy [M] arrays ``n`` (draws processed), ``mean`` and
    ``m2`` (moments of the finite replicates), ``below`` (finite replicates
    below the observation, the term's value at that draw), ``nonfinite``
    (replicates of a draw with an invalid scale, rate or shape: NaN, counted,
    never raised) — a partial ``merge_predictive`` combines with other shards —
    and the derived ``var`` = m2 / (n_finite - 1) and ``pit`` = below /
    n_finite, n_finite = n - nonfinite.  A likelihood with a count term also
    returns ``equal`` (finite replicates equal to the observation) and the
    mid-rank ``pit_mid`` = (below + equal / 2) / n_finite, the PIT of a
    discrete outcome; ``pit`` stays as it is.  ``replicates=True`` adds
    ``replicates``, the [C, S', M] float32 device tensor (small problems only).
    With an initialised process group (``group=False`` stays local) the ranks'
    partials are gathered and merged in rank order; the replicates stay this
    rank's."""
    import torch

    from . import _trace

    thin = int(thin)
    if thin < 1:
        raise ValueError("thin must be >= 1")
    x, lay = _pointwise_inputs(samples, layout)
    C, S, D = x.shape
    prog = _trace.pointwise_program(log_likelihood_fn, lay)
    lib = _lib.load()
    M = prog.num_elements
    nb = lib.mc_predictive_workspace_bytes(prog.handle, C, S, thin)
    if nb < 0:   # (an unsupported term is reported here: nothing is launched)
        _lib.check(int(nb))
    Sp = (S + thin - 1) // thin
    st = torch.empty((_lib.MC_PP_COUNT, M), dtype=torch.float64, device=x.device)
    eq = (torch.empty(M, dtype=torch.float64, device=x.device)
          if lib.mc_program_num_count_terms(prog.handle) > 0 else None)
    rep = torch.empty((C, Sp, M), dtype=torch.float32, device=x.device) if replicates else None
    ws = torch.empty(max(int(nb), 1), dtype=torch.uint8, device=x.device)
    _lib.check(lib.mc_predictive_eq(prog.handle, C, S, thin, int(seed) & 0xFFFFFFFFFFFFFFFF,
                                    int(chain_offset), int(iter_offset), _lib.ptr(x),
                                    _lib.ptr(st), _lib.ptr(eq), _lib.ptr(rep), _lib.ptr(ws), nb,
                                    _lib.stream_handle()))
    host = st.cpu().numpy()   # (synchronises: prog, x and ws outlive the launch)
    part = {f: host[k].copy() for k, f in enumerate(PP_FIELDS)}
    if eq is not None:
        part["equal"] = eq.cpu().numpy()
    out = merge_predictive(_gather_parts(part, group))
    with np.errstate(all="ignore"):
        nfin = out["n"] - out["nonfinite"]
        out["var"] = out["m2"] / (nfin - 1.0)
        out["pit"] = out["below"] / nfin
        if "equal" in out:
            out["pit_mid"] = (out["below"] + 0.5 * out["equal"]) / nfin
    if replicates:
        out["replicates"] = rep
    return out
