"""``conditional_scores`` -- which recordings were real detections: the two enumerated layers of a fitted ``occu_cs`` GIVEN the scores,
per posterior draw.

BUILDER-DEFINED, no counterpart in the reference: biolith/utils/predict.py withholds the observations (predict.py:78-80), so the ``z``
and ``f`` of ``predict(occu_cs, ...)`` are draws from the prior and a site whose scores sit at ``mu1`` can come back unoccupied with
``f = 0`` throughout.  occu_cs (Rhinehart et al. 2022; occu_cs.py:185-223) has the site-period state ``z`` and, per recording,
``f_j ~ Bernoulli(z p_j)``: whether score ``s_j`` came from the true-positive ``Normal(mu1, sigma1)`` or the background
``Normal(mu0, sigma0)``.  Here, per posterior draw and (period, site), the engine returns what the sampler's density kernel forms at
every leapfrog and discards (``include/biolith_hip.h``: ``bl_score_posterior``): over the cell's unmasked visits, with
``mix_j = logaddexp(log p_j + n1_j, log(1 - p_j) + n0_j)``, ``A = log psi + sum mix_j`` and ``B = log(1 - psi) + sum n0_j``,
``log_lik = logaddexp(A, B)``, ``z_prob = exp(A - log_lik)``, ``r_j = exp(log p_j + n1_j - mix_j) = P(f_j = 1 | z = 1, s_j)`` and
``f_prob_j = z_prob r_j``.  No NumPyro/JAX, no CPU fallback.
"""
from __future__ import annotations

from typing import Callable, Optional

import numpy as np

from ._conditional import plate_last, prepare
from .data import species_dataset
from .layout import draws_from_sites
from .mcmc import LazySamples


def conditional_scores(
    model_fn: Callable,
    mcmc,
    site_covs=None,
    obs_covs=None,
    obs=None,
    random_seed: int = 0,
    timeout: Optional[int] = None,
    **kwargs,
) -> LazySamples:
    """Conditional occupancy and true-positive indicators of a fitted ``occu_cs`` model for every posterior draw.

    The data are passed exactly as to :func:`biolith_amd.utils.fit` (``obs`` holds the scores); the model's options (priors) and
    ``device=`` go through ``kwargs``; ``mcmc`` is the ``FitResult.mcmc`` of that fit.

    Returns
    -------
    LazySamples
        species plate last (one species), n = posterior draws:
        ``psi`` (n, T, N, 1) float32; ``z_prob`` (n, T, N, 1) float32 = P(z = 1 | the cell's scores, theta);
        ``z`` (n, T, N, 1) int32 ~ Bernoulli(z_prob); ``log_lik`` (n, T, N, 1) float32, the log-likelihood of the cell's unmasked scores
        with z and every f summed out (its sum over cells is the model's log-likelihood); ``n_obs`` (T, N, 1) int32, the unmasked
        visits behind each cell;
        ``f_prob`` (n, J, T, N, 1) float32 = P(f_j = 1 | the cell's scores, theta), the probability that recording j was a true
        positive; ``f`` (n, J, T, N, 1) int32, drawn JOINTLY with ``z``: ``f_j = z Bernoulli(r_j)``, so ``f <= z`` elementwise.
        A masked visit has no score to condition on: its ``f_prob`` is ``z_prob p_j``.  A cell with ``n_obs == 0`` has
        ``log_lik == 0`` and ``z_prob == psi``.  ``z`` and ``f`` are functions of (random_seed, draw, period, site).  The two
        replicate-level arrays are materialised on first access, by a second call with the same seed.  ``log_lik`` and ``n_obs`` feed
        :func:`biolith_amd.evaluation.lppd_marginal` / ``waic_marginal``, ``z`` feeds ``finite_sample_occupancy``, ``f_prob`` feeds
        ``expected_true_positives``.

    Examples
    --------
    >>> from biolith_amd.models import simulate_cs, occu_cs
    >>> from biolith_amd.utils import fit, conditional_scores
    >>> data, _ = simulate_cs()
    >>> results = fit(occu_cs, **data, num_samples=10, num_warmup=10, num_chains=1)
    >>> lat = conditional_scores(occu_cs, results.mcmc, **data)
    """
    c = prepare("conditional_scores", "occu_cs, the one model with a per-recording indicator",
                ("occu", "occu_comb", "occu_rn", "nmixture", "occu_dyn", "occu_cop"), model_fn, mcmc, site_covs, obs_covs, obs, kwargs)

    def body(ds, draws, sp, seed):
        psi = ds.deterministic(draws, psi=True, prob_detection=False)[0]
        log_lik, z_prob, z, _, _ = ds.score_posterior(draws, seed=seed, visits=False)
        return psi, z_prob, z, log_lik

    psi, z_prob, z, log_lik = c.per_species(random_seed, timeout, body)   # (n, T, N, 1)
    out = LazySamples(psi=psi, z_prob=z_prob, z=z.astype(np.int32), log_lik=log_lik, n_obs=plate_last(c.n_obs))
    pair = {}

    def visit_level(key):   # one call fills both: f is drawn jointly with the z above (same seed, same generator)
        if not pair:
            ds, draws = species_dataset(c.spec, 0, c.device), draws_from_sites(c.layout, c.posterior, 0)
            try:
                _, _, _, f_prob, f = ds.score_posterior(draws, seed=int(random_seed) & (2 ** 64 - 1))
            finally:
                ds.close()
            pair.update(f_prob=f_prob[..., None], f=f[..., None].astype(np.int32))   # (n, J, T, N, 1)
        return pair.pop(key)

    out.set_lazy("f_prob", lambda: visit_level("f_prob"))
    out.set_lazy("f", lambda: visit_level("f"))
    return out
