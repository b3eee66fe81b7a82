"""``conditional_counts`` -- occupancy and the real detections of a fitted ``occu_cop`` GIVEN the counts, per posterior draw.

BUILDER-DEFINED, no counterpart in the reference: biolith/utils/predict.py withholds the observations (predict.py:78-80), so the ``z``
of ``predict(occu_cop, ...)`` is a draw from the prior and a site where the species was counted twelve times can come back unoccupied.
occu_cop (Pautrel et al. 2024; occu_cop.py:150-255) counts detections, ``y_j ~ Poisson(d_j (z lambda_j + (1 - z) f_u + f_c))``.  Here, per
posterior draw and (period, site), the engine returns what the sampler's density kernel forms at every leapfrog and discards
(``include/biolith_hip.h``: ``bl_count_posterior``): over the cell's unmasked visits, with f the sampled false-positive rate, f1 = f in
"constant" mode (else 0) and ``c_j = y_j log d_j - lgamma(y_j + 1)``,
``A = log psi + sum_j [y_j log(lambda_j + f1) - d_j (lambda_j + f1) + c_j]``, ``B = log(1 - psi) + sum_j [y_j log f - d_j f + c_j]``
(Poisson(0) without a rate), ``log_lik = logaddexp(A, B)`` and ``z_prob = sigmoid(A - B)``.  The visit level is the Poisson thinning
of the count: given z = 1 the real detections among the ``y_j`` counted ones are ``Binomial(y_j, rho_j)``,
``rho_j = lambda_j / (lambda_j + f1)``.  No NumPyro/JAX, no CPU fallback.
"""
from __future__ import annotations

from typing import Callable, Optional

import numpy as np

from ._conditional import SERVED_BY, plate_last, prepare
from .mcmc import LazySamples


def conditional_counts(
    model_fn: Callable,
    mcmc,
    site_covs=None,
    obs_covs=None,
    obs=None,
    session_duration=None,
    random_seed: int = 0,
    timeout: Optional[int] = None,
    **kwargs,
) -> LazySamples:
    """Conditional occupancy and true detections of a fitted ``occu_cop`` model for every posterior draw.

    The data are passed exactly as to :func:`biolith_amd.utils.fit` (``obs`` holds the counts); the model's options
    (``false_positives_*``, ``*_random_effects``, priors) and ``device=`` go through ``kwargs``; ``mcmc`` is the ``FitResult.mcmc`` of
    that fit.

    Returns
    -------
    LazySamples
        species plate last, n = posterior draws:
        ``psi`` (n, T, N, S) float32; ``z_prob`` (n, T, N, S) float32 = P(z = 1 | the cell's counts, theta);
        ``z`` (n, T, N, S) int32 ~ Bernoulli(z_prob); ``log_lik`` (n, T, N, S) float32, the log-likelihood of the cell's unmasked counts
        with z summed out, the Poisson pmf's parameter-free part included (its sum over cells is the model's log-likelihood);
        ``n_obs`` (T, N, S) int32, the unmasked visits behind each cell;
        ``true_mean`` (n, J, T, N, S) float32 = z_prob y_j rho_j, the expected number of visit j's counted detections that were real;
        ``true_count`` (n, J, T, N, S) int32, drawn JOINTLY with ``z``: ``z Binomial(y_j, rho_j)``, so ``true_count <= z y``
        elementwise.  ``rho_j`` is 1 unless ``false_positives_constant``.  A masked visit has no count: both are 0 there.  A cell
        with ``n_obs == 0`` has ``log_lik == 0`` and ``z_prob == psi``; without a rate a cell with a positive count has
        ``z_prob == 1``.  ``z`` and ``true_count`` are functions of (random_seed, draw, period, site, species).  The two visit-level
        arrays are materialised on first access, by one second call per species with the same seeds.  ``log_lik`` and ``n_obs`` feed
        :func:`biolith_amd.evaluation.lppd_marginal` / ``waic_marginal``, ``z`` feeds ``finite_sample_occupancy``, ``true_mean`` feeds
        ``expected_true_detections``.  Several species (no rate is sampled then) are served species by species, as ``fit`` runs them.

    Examples
    --------
    >>> from biolith_amd.models import simulate_cop, occu_cop
    >>> from biolith_amd.utils import fit, conditional_counts
    >>> data, _ = simulate_cop()
    >>> results = fit(occu_cop, **data, num_samples=10, num_warmup=10, num_chains=1)
    >>> lat = conditional_counts(occu_cop, results.mcmc, **data)
    """
    c = prepare("conditional_counts", "occu_cop with or without a false-positive rate / random effects",
                tuple(m for m in SERVED_BY if m != "occu_cop"), model_fn, mcmc, site_covs, obs_covs, obs, kwargs,
                session_duration=session_duration)

    def body(ds, draws, sp, seed):
        psi = ds.deterministic(draws, psi=True, prob_detection=False)[0]
        log_lik, z_prob, z, _, _ = ds.count_posterior(draws, seed=seed, visits=False)
        return psi, z_prob, z, log_lik

    psi, z_prob, z, log_lik = c.per_species(random_seed, timeout, body)   # (n, T, N, S)
    out = LazySamples(psi=psi, z_prob=z_prob, z=z.astype(np.int32), log_lik=log_lik, n_obs=plate_last(c.n_obs))
    pair = {}

    def visit_level(key):   # one pass over the species fills both: true_count is drawn jointly with the z above (same seeds, same generator)
        if not pair:
            true_mean, true_count = c.per_species(random_seed, timeout, lambda ds, draws, sp, seed: ds.count_posterior(draws, seed=seed)[3:])
            pair.update(true_mean=true_mean, true_count=true_count)   # (n, J, T, N, S)
        return pair.pop(key)

    out.set_lazy("true_mean", lambda: visit_level("true_mean"))
    out.set_lazy("true_count", lambda: visit_level("true_count"))
    return out
