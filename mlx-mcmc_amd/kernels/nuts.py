"""No-U-Turn Sampler on MI355X — drop-in for mlx_mcmc/kernels/nuts.py:16-358.

Same signature, defaults, return value and progress output as the
reference's ``nuts()`` (slice NUTS, Hoffman & Gelman 2014 Alg. 3, dual
averaging).  Tree building runs iteratively inside a persistent HIP kernel:
``k_nuts_lr`` (csrc/nuts_lanes.h, one chain per wave, lane-resident state)
when the model plans as one lane-resident slice, else ``k_nuts`` (csrc/nuts.h,
one chain per chain group on the gradient tape), or ``k_nuts_sl``
(csrc/nuts_sliced.h) when it plans as several fast-form data slices.

``nuts_kernel``: "auto" runs the lane-resident kernel ``k_nuts_lr``
(csrc/nuts_lanes.h: chain state in registers, tree arena in LDS) when the
model plans as one lane-resident slice, the sliced kernel ``k_nuts_sl``
(csrc/nuts_sliced.h: one wave per chain and data slice, one record exchange
per leaf) when it plans as several fast-form slices (the README "Large"
row), else ``k_nuts``; "tape" keeps ``k_nuts``; "lanes" is accepted with a mass
matrix only (below: the metric on ``k_nuts_lr``, or a ``ValueError``) — without one
it raises ``ValueError`` before anything is traced, as an unknown value does
("auto" already picks ``k_nuts_lr`` where the model plans onto it).
``num_slices``: data slices per chain (0: the automatic plan, as ``hmc()``).

``slice_mode="reference"`` (default) reproduces the reference's float32
slice variable: u = f32 exp(log u) rounds to the smallest denormal (log u =
~-103.28, SURVEY Q7's ~-103.3) down to ln 2^-150 ~ -103.97 and to 0 below it,
which switches the slice test off (log u = -inf)
(nuts.py:236-237); ``"exact"`` keeps log u in double precision.
Keyword-only additions as for ``hmc()``, ``inverse_mass_matrix`` and
``adapt_mass_matrix`` among them: a per-chain diagonal metric, adapted during
warmup in Stan's windows with dual averaging restarted at each update
(csrc/metric.h); such a run takes ``k_nuts`` as ``nuts_kernel="tape"`` does.
``nuts_kernel="lanes"`` opts such a run onto ``k_nuts_lr`` instead (several times
the leaf rate) when the model is register-only — no shared parameter, no scalar
term, one Normal term with one element per parameter (theta_i ~ N(m, s_i)); any
other model raises ``ValueError`` before a launch and keeps the default route.
(On a model with constrained parameters the restart's first, ~15x longer step
can meet the reference's NaN -> alpha = 1 rule and run the step size away —
DESIGN section 4; adapt with ``adapt_step_size=False``, or pass a metric adapted
earlier as ``inverse_mass_matrix``.)
"""
from __future__ import annotations

from ._driver import run_sampler

DELTA_MAX = 1000.0  # nuts.py:13 (the kernel uses the same constant)


def nuts(log_prob_fn, initial_params, num_samples=1000, num_warmup=1000, step_size=0.1,
         max_tree_depth=10, adapt_step_size=True, target_accept=0.65, key=None, *,
         num_chains=1, chain_offset=0, slice_mode="reference", progress=True,
         return_info=False, return_trace=False, keep_on_device=False,
         initial_positions=None, nuts_kernel="auto", num_slices=0,
         inverse_mass_matrix=None, adapt_mass_matrix=False):
    """No-U-Turn Sampler (NUTS) for efficient HMC sampling.

    Returns ``(samples, acceptance_rate)`` like the reference, where the rate
    is the fraction of sampling iterations whose mean acceptance statistic
    exceeds 0.5 (nuts.py:347).
    """
    if nuts_kernel not in ("auto", "tape", "lanes"):
        raise ValueError(f"nuts_kernel must be 'auto', 'tape' or 'lanes', not {nuts_kernel!r}")
    if nuts_kernel == "lanes" and inverse_mass_matrix is None and not adapt_mass_matrix:
        raise ValueError("nuts_kernel='lanes' chooses the kernel of a run with a mass matrix: "
                         "pass inverse_mass_matrix= or adapt_mass_matrix=True with it. Without "
                         "one, nuts_kernel='auto' already runs the lane-resident kernel "
                         "wherever the model plans onto it")
    samples, rate, info = run_sampler(
        "nuts", log_prob_fn, initial_params, num_samples=num_samples, num_warmup=num_warmup,
        step_size=step_size, target_accept=target_accept, adapt_step_size=adapt_step_size,
        key=key, max_tree_depth=max_tree_depth, num_chains=num_chains,
        chain_offset=chain_offset, slice_mode=slice_mode, progress=progress,
        return_trace=return_trace, keep_on_device=keep_on_device,
        initial_positions=initial_positions,
        num_slices=1 if nuts_kernel == "tape" else int(num_slices),
        inverse_mass_matrix=inverse_mass_matrix, adapt_mass_matrix=adapt_mass_matrix,
        nuts_kernel=nuts_kernel)
    if return_info:
        return samples, rate, info
    return samples, rate
