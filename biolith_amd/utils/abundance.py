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

from .data import prepare_data, species_dataset
from .latent import _unmasked
from .layout import draws_from_sites, layout_for
from .mcmc import LazySamples
from .misc import time_limit

SERVED = ("occu_rn", "nmixture")


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
    name = getattr(model_fn, "__biolith_amd_model__", None) if callable(model_fn) else None
    if name is None:
        raise TypeError("conditional_abundance(): model_fn must be a biolith_amd model (biolith_amd.models.occu_rn / nmixture)")
    if name not in SERVED:
        hint = "; use conditional_occupancy" if name in ("occu", "occu_comb") else ""
        raise NotImplementedError(f"conditional_abundance(): not built for {name} (built: occu_rn with or without a false-positive rate / "
                                  f"random effects, and nmixture with or without random effects){hint}")
    device = int(kwargs.pop("device", 0))
    site_covs, obs_covs, obs, _, _, _ = prepare_data(site_covs, obs_covs, obs, None)
    valid = {k: v for k, v in dict(site_covs=site_covs, obs_covs=obs_covs, obs=obs).items() if v is not None}
    spec = model_fn(**valid, **kwargs)
    posterior = mcmc.get_samples()
    beta = np.asarray(posterior["beta"], dtype=np.float32)    # (n, S, Ks+1)
    n_species = beta.shape[1]
    if n_species != spec.obs.shape[0] or beta.shape[2] != spec.site_covs.shape[1] + 1:
        raise ValueError("conditional_abundance(): the data differ from the fitted model's (species or site covariate count)")
    if np.asarray(posterior["alpha"]).shape[2] != spec.obs_covs.shape[3] + 1:
        raise ValueError("conditional_abundance(): covariate counts differ from the fitted model's coefficients")

    X = np.asarray(spec.site_covs, dtype=np.float32)
    n_obs = _unmasked(spec.obs, spec.obs_covs, np.isnan(X).any(-1))
    N, T, J, Ko = spec.obs_covs.shape
    layout = layout_for(spec, N=N, T=T, J=J, Ks=X.shape[1], Ko=Ko)

    lam, ll, mean, occ, draw = [], [], [], [], []
    with time_limit(timeout):
        for sp in range(n_species):
            ds, draws = species_dataset(spec, sp, device), draws_from_sites(layout, posterior, sp)
            lam.append(ds.deterministic(draws, psi=True, prob_detection=False)[0])
            out = ds.abundance_posterior(draws, seed=(int(random_seed) + (sp << 32)) & (2 ** 64 - 1))
            for acc, a in zip((ll, mean, occ, draw), out):
                acc.append(a)
            ds.close()
    out = LazySamples()
    out["abundance"] = np.stack(lam, axis=-1)                             # (n, T, N, S)
    out["N_mean"] = np.stack(mean, axis=-1)
    out["occ_prob"] = np.stack(occ, axis=-1)
    out["N_i"] = np.stack(draw, axis=-1).astype(np.int32)
    out["log_lik"] = np.stack(ll, axis=-1)
    out["n_obs"] = np.ascontiguousarray(n_obs.transpose(2, 1, 0)).astype(np.int32)   # (S, N, T) -> (T, N, S)
    return out
