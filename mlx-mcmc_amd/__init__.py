"""mlx_mcmc_amd — MI355X-native HMC/NUTS engine with the mlx-mcmc API.

Drop-in for the sampling hot path of korentomas/mlx-mcmc
(mlx_mcmc/__init__.py:24-46): ``Normal``, ``HalfNormal``, ``Exponential``,
``Gamma``, ``Beta``, ``Distribution``, the count likelihoods ``Bernoulli``,
``Binomial``, ``Poisson`` (not in the reference), ``Categorical``, the
Student-t family ``StudentT``, ``Cauchy``, ``HalfStudentT``, ``HalfCauchy`` (not
in the reference),
``hmc``, ``nuts``, ``metropolis_hastings``, ``MCMC``; ``mlx_mcmc_amd.core`` replaces ``mlx.core`` in
user models (``import mlx_mcmc_amd.core as mx``).  Sampling runs in the HIP
kernels of libmcmc355.so (csrc/); there is no CPU fallback.
"""
from . import core, random
from .distributions import (Bernoulli, Beta, Binomial, Categorical, Cauchy, Distribution,
                            Exponential, Gamma, HalfCauchy, HalfNormal, HalfStudentT, Normal,
                            Poisson, StudentT)
from .kernels import hmc, metropolis_hastings, nuts
from .inference import MCMC
from .diagnostics import compute_ess

__version__ = "0.1.0"

__all__ = ["Distribution", "Normal", "HalfNormal", "Exponential", "Gamma", "Beta", "Bernoulli",
           "Binomial", "Poisson", "Categorical", "StudentT", "Cauchy", "HalfStudentT",
           "HalfCauchy", "hmc", "nuts", "metropolis_hastings", "MCMC", "core", "random",
           "compute_ess"]
