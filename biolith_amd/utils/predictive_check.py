"""``predictive_check`` -- the posterior predictive check of biolith/evaluation/posterior_predictive_check.py:17-160, fused on the HIP engine.

``evaluation.posterior_predictive_check`` reduces ``predict()``'s replicate-level arrays ``y`` and ``prob_detection``, each
(n, J, T, N, S), in float64 on the host: O(n J T N) memory for one number.  All of it is a function of (seed, draw, period, site) that the
device regenerates, so here one C-ABI call per species -- ``bl_predictive_check`` (``include/biolith_hip.h``) -- redraws ``predict()``'s
replicate, forms ``E = psi * prob_detection``, groups, applies the discrepancy and reduces, and returns four float64 per draw.  Nothing
of size (n, J, T, N) exists on the device or on the host.  Served: ``occu`` (with ``false_positives_*`` and / or ``*_random_effects``).
No NumPyro/JAX, no CPU fallback.
"""
from __future__ import annotations

from typing import Callable, Optional

import numpy as np

from .data import prepare_data, species_dataset
from .layout import draws_from_sites, layout_for
from .misc import time_limit

_STATISTICS = ["freeman-tukey", "chi-squared"]   # (the columns of the entry's result: ft_obs, ft_rep, chi_obs, chi_rep)


def predictive_check(
    model_fn: Callable,
    mcmc,
    site_covs=None,
    obs_covs=None,
    obs=None,
    group_by: str = "site",
    statistic: str = "freeman-tukey",
    random_seed: int = 0,
    timeout: Optional[int] = None,
    **kwargs,
) -> dict:
    """Bayesian p-value ``P(T(y_rep, theta) > T(y, theta) | y)`` of a fitted ``occu`` model, with detections grouped by site or by
    revisit and the Freeman-Tukey or chi-squared discrepancy against ``E = psi * p``.

    The data are passed exactly as to :func:`biolith_amd.utils.fit`; the model's options (``false_positives_*``,
    ``*_random_effects``, priors) and ``device=`` go through ``kwargs``; ``mcmc`` is the ``FitResult.mcmc`` of that fit.  ``obs`` holds
    0, 1 or NaN (not observed); a visit counts where its observation is present, whatever its covariates.

    The contract::

        predictive_check(m, mcmc, **data, group_by=g, statistic=s, random_seed=r)["p_value"]
            == posterior_predictive_check(predict(m, mcmc, **data, random_seed=r), data["obs"], g, s)

    The replicate is ``predict()``'s ``y`` for the same ``random_seed``, bit for bit; ``E`` is the exact float64 product of its float32
    ``psi`` and ``prob_detection``; only the order of the float64 additions differs.  As the reference notes, the check is valid
    without false positives: with a false-positive rate ``E`` is still ``psi * p``.

    Returns
    -------
    dict
        ``p_value`` float = ``mean(d_rep > d_obs)``; ``d_obs`` and ``d_rep`` (n,) float64, the discrepancy of the observed and of the
        replicate data per posterior draw, summed over the species plate.

    Examples
    --------
    >>> from biolith_amd.models import simulate, occu
    >>> from biolith_amd.utils import fit, predictive_check
    >>> data, _ = simulate()
    >>> results = fit(occu, **data, num_samples=100, num_warmup=100, num_chains=1)
    >>> predictive_check(occu, results.mcmc, **data, group_by="revisit", statistic="chi-squared")["p_value"]
    """
    name = getattr(model_fn, "__biolith_amd_model__", None) if callable(model_fn) else None
    if name is None:
        raise TypeError("predictive_check(): model_fn must be a biolith_amd model (biolith_amd.models.occu)")
    if name != "occu":
        raise NotImplementedError(f"predictive_check(): not built for {name} (built: occu with or without false positives / random "
                                  "effects); posterior_predictive_check on predict()'s output is the host path")
    if statistic not in _STATISTICS:
        raise ValueError(f"`statistic` must be one of {_STATISTICS}")
    if group_by not in ("site", "revisit"):
        raise ValueError("`group_by` must be either 'site' or 'revisit'")
    if obs is None:
        raise ValueError("predictive_check(): obs is required (the observed data the replicates are compared with)")
    device = int(kwargs.pop("device", 0))
    kwargs.pop("session_duration", None)   # (occu takes none; predict() accepts and ignores it)

    site_covs, obs_covs, obs, _, _, _ = prepare_data(site_covs, obs_covs, obs, None)
    if obs.ndim != 4 or obs.shape[1:] != np.shape(obs_covs)[:3]:
        raise ValueError("predictive_check(): obs must be of shape (n_species, n_sites, n_periods, n_replicates) matching obs_covs")
    posterior = mcmc.get_samples()
    beta = np.asarray(posterior["beta"], dtype=np.float32)    # (n, S, Ks+1)
    alpha = np.asarray(posterior["alpha"], dtype=np.float32)  # (n, S, Ko+1)
    n, n_species = beta.shape[0], beta.shape[1]
    if obs.shape[0] != n_species:
        raise ValueError(f"predictive_check(): obs has {obs.shape[0]} species, the posterior {n_species}")

    # the handles are predict()'s: the model is called with the observations withheld (an all-missing array of the fitted species count)
    blank = np.full(obs.shape, np.nan, dtype=np.float32)
    spec = model_fn(site_covs=site_covs, obs_covs=obs_covs, obs=blank, **kwargs)
    if beta.shape[2] != spec.site_covs.shape[1] + 1 or alpha.shape[2] != spec.obs_covs.shape[3] + 1:
        raise ValueError("predictive_check(): covariate counts differ from the fitted model's coefficients")
    N, T, J = spec.obs_covs.shape[:3]
    layout = layout_for(spec, N=N, T=T, J=J, Ks=beta.shape[2] - 1, Ko=alpha.shape[2] - 1)

    by_site = group_by == "site"
    col = 2 * _STATISTICS.index(statistic)
    d_obs, d_rep = np.zeros(n), np.zeros(n)
    with time_limit(timeout):
        for sp in range(n_species):
            ds, draws = species_dataset(spec, sp, device), draws_from_sites(layout, posterior, sp)
            res = ds.predictive_check(draws, obs[sp], seed=(int(random_seed) + (sp << 32)) & (2 ** 64 - 1),
                                      by_site=by_site, by_revisit=not by_site)[0 if by_site else 1]
            ds.close()
            d_obs += res[:, col]
            d_rep += res[:, col + 1]
    return {"p_value": float(np.mean(d_rep > d_obs)), "d_obs": d_obs, "d_rep": d_rep}
