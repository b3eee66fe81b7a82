"""``conditional_abundance`` -- the site abundance GIVEN the data, per posterior draw.

BUILDER-DEFINED, no counterpart in the reference: biolith/utils/predict.py withholds the observations (predict.py:78-80), so its
``N_i`` is a draw from the prior Poisson(lambda) and a site with three detections can come back with N = 0.  Here, per posterior draw
and (period, site), the engine returns what the sampler's density kernels form and discard (``include/biolith_hip.h``:
``bl_abundance_posterior``).  With l_n the log of the n-th addend of the model's own marginal likelihood over that cell's unmasked
replicates and K = ``max_abundance``:

occu_rn   l_n = log Categorical(Poisson(lambda) pmf renormalised on 0..K)(n) + sum_j log Bernoulli(y_j; 1 - (1 - p_nj)(1 - f)),
          p_nj = 1 - (1 - r_j)^n, f the false-positive rate or 0, NumPyro's probability clamp as the sampler's potential applies it;
nmixture  l_n = log Poisson(lambda)(n) + sum_j log Binomial(y_j; n, p_j) for max_j y_j <= n <= K, -inf below (the untruncated
          Poisson cut at K: the model's ``N_i_trunc_norm`` factor puts the normaliser back);

``log_lik = logsumexp_n l_n``, ``N_pmf(n) = exp(l_n - log_lik)``, ``N_mean = sum_n n N_pmf(n)``, ``occ_prob = 1 - N_pmf(0)`` and ``N_i`` one
draw from ``N_pmf``.  Served: ``occu_rn`` (with ``false_positives_constant`` and / or ``*_random_effects``) and ``nmixture`` (with
``*_random_effects``).  No NumPyro/JAX, no CPU fallback.
"""
from __future__ import annotations

from typing import Callable, Optional

import numpy as np

from ._conditional import plate_last, prepare
from .mcmc import LazySamples


def conditional_abundance(
    model_fn: Callable,
    mcmc,
    site_covs=None,
    obs_covs=None,
    obs=None,
    random_seed: int = 0,
    timeout: Optional[int] = None,
    **kwargs,
) -> LazySamples:
    """Conditional abundance of a fitted ``occu_rn`` / ``nmixture`` model for every posterior draw.

    The data are passed exactly as to :func:`biolith_amd.utils.fit` for that model; the model's options (``max_abundance``,
    ``false_positives_constant``, ``*_random_effects``, priors) and ``device=`` go through ``kwargs``; ``mcmc`` is the
    ``FitResult.mcmc`` of that fit.

    Returns
    -------
    LazySamples
        species plate last, n = posterior draws:
        ``abundance`` (n, T, N, S) float32, lambda as ``predict()`` names it; ``N_mean`` (n, T, N, S) float32 = E[N | the cell's data,
        theta]; ``occ_prob`` (n, T, N, S) float32 = P(N > 0 | the cell's data, theta); ``N_i`` (n, T, N, S) int32, one draw of N given
        the cell's data, a function of (random_seed, draw, period, site); ``log_lik`` (n, T, N, S) float32, the N-marginalised
        log-likelihood of the cell's unmasked observations (its sum over cells is the model's log-likelihood); ``n_obs`` (T, N, S)
        int32, the unmasked observations behind each cell.  A cell with ``n_obs == 0`` returns the prior: for ``occu_rn``
        ``log_lik == 0`` and the renormalised truncated Poisson; for ``nmixture`` ``log_lik == log P(N <= K)``, which is not zero.
        ``log_lik`` and ``n_obs`` feed :func:`biolith_amd.evaluation.lppd_marginal` / ``waic_marginal``.

    Examples
    --------
    >>> from biolith_amd.models import simulate_rn, occu_rn
    >>> from biolith_amd.utils import fit, conditional_abundance
    >>> data, _ = simulate_rn()
    >>> results = fit(occu_rn, **data, num_samples=10, num_warmup=10, num_chains=1)
    >>> lat = conditional_abundance(occu_rn, results.mcmc, **data)
    """
    c = prepare("conditional_abundance", "occu_rn with or without a false-positive rate / random effects, and nmixture with or without "
                "random effects", ("occu", "occu_comb", "occu_cs", "occu_cop"), model_fn, mcmc, site_covs, obs_covs, obs, kwargs)

    def body(ds, draws, sp, seed):
        lam = ds.deterministic(draws, psi=True, prob_detection=False)[0]
        log_lik, n_mean, occ_prob, n_draw = ds.abundance_posterior(draws, seed=seed)
        return lam, n_mean, occ_prob, n_draw, log_lik

    lam, n_mean, occ_prob, n_draw, log_lik = c.per_species(random_seed, timeout, body)   # (n, T, N, S)
    return LazySamples(abundance=lam, N_mean=n_mean, occ_prob=occ_prob, N_i=n_draw.astype(np.int32), log_lik=log_lik, n_obs=plate_last(c.n_obs))
