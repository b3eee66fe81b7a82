"""``predictive_check_counts`` -- the posterior predictive check for the abundance and count models (``occu_rn``, ``nmixture``,
``occu_cop``), fused on the HIP engine.  BUILDER-DEFINED: the reference's check (posterior_predictive_check.py:17-160) is stated for
``occu``, against ``E = psi * p``; here ``E`` is the model's own mean of ``y`` with the latent state summed out.

``evaluation.posterior_predictive_check_counts`` reduces ``predict()``'s replicate-level arrays, each (n, J, T, N, S), in float64 on the
host.  All of it is a function of (seed, draw, period, site) that the device regenerates, so here one C-ABI call per species --
``bl_predictive_check_counts`` (``include/biolith_hip.h``) -- redraws ``predict()``'s replicate, forms ``E``, groups, applies the
discrepancy and reduces, and returns four float64 per draw.  Nothing of size (n, J, T, N) exists on the device or on the host.
No NumPyro/JAX, no CPU fallback.
"""
from __future__ import annotations

from typing import Callable, Optional

import numpy as np

from .data import prepare_data, species_dataset
from .layout import draws_from_sites, layout_for
from .misc import time_limit

_STATISTICS = ["freeman-tukey", "chi-squared"]   # (the columns of the entry's result: ft_obs, ft_rep, chi_obs, chi_rep)
_SERVED = ("occu_rn", "nmixture", "occu_cop")


def predictive_check_counts(
    model_fn: Callable,
    mcmc,
    site_covs=None,
    obs_covs=None,
    obs=None,
    session_duration=None,
    group_by: str = "site",
    statistic: str = "freeman-tukey",
    random_seed: int = 0,
    timeout: Optional[int] = None,
    **kwargs,
) -> dict:
    """Bayesian p-value ``P(T(y_rep, theta) > T(y, theta) | y)`` of a fitted ``occu_rn``, ``nmixture`` or ``occu_cop`` model, with the
    data grouped by site or by revisit and the Freeman-Tukey or chi-squared discrepancy against the model's expected value of ``y``.

    The data are passed exactly as to :func:`biolith_amd.utils.fit`; the model's options (``max_abundance``, ``false_positives_*``,
    ``*_random_effects``, priors) and ``device=`` go through ``kwargs``; ``mcmc`` is the ``FitResult.mcmc`` of that fit.  ``obs`` holds
    whole counts (``occu_rn``: 0 / 1) or NaN (not observed); a visit counts where its observation is present, whatever its covariates.

    With ``lambda`` = ``abundance``, ``p`` = ``prob_detection``, ``K`` = ``max_abundance`` and ``pi`` the pmf of Poisson(lambda)
    restricted to 0..K::

        nmixture   E = p * sum_n n pi_n
        occu_rn    E = 1 - (1 - prob_fp_constant) * sum_n pi_n (1 - p)^n
        occu_cop   E = session_duration * (psi * rate_detection + (1 - psi) * rate_fp_unoccupied + rate_fp_constant)

    The contract::

        predictive_check_counts(m, mcmc, **data, group_by=g, statistic=s, random_seed=r)["p_value"]
            == posterior_predictive_check_counts(m, predict(m, mcmc, **data, random_seed=r), data["obs"], g, s, ...)

    The replicate is ``predict()``'s ``y`` for the same ``random_seed``, bit for bit; ``E`` is formed in float64 from its float32
    deterministic sites; what differs is libm in the truncated sums and the order of the float64 additions.

    Returns
    -------
    dict
        ``p_value`` float = ``mean(d_rep > d_obs)``; ``d_obs`` and ``d_rep`` (n,) float64, the discrepancy of the observed and of the
        replicate data per posterior draw, summed over the species plate.

    Examples
    --------
    >>> from biolith_amd.models import simulate_nmixture, nmixture
    >>> from biolith_amd.utils import fit, predictive_check_counts
    >>> data, _ = simulate_nmixture()
    >>> results = fit(nmixture, **data, num_samples=100, num_warmup=100, num_chains=1)
    >>> predictive_check_counts(nmixture, results.mcmc, **data, group_by="site", statistic="chi-squared")["p_value"]
    """
    name = getattr(model_fn, "__biolith_amd_model__", None) if callable(model_fn) else None
    if name is None:
        raise TypeError("predictive_check_counts(): model_fn must be a biolith_amd model (biolith_amd.models.occu_rn / nmixture / occu_cop)")
    if name not in _SERVED:
        hint = "; use predictive_check" if name == "occu" else ""
        raise NotImplementedError(f"predictive_check_counts(): not built for {name} (built: {', '.join(_SERVED)}){hint}")
    if statistic not in _STATISTICS:
        raise ValueError(f"`statistic` must be one of {_STATISTICS}")
    if group_by not in ("site", "revisit"):
        raise ValueError("`group_by` must be either 'site' or 'revisit'")
    if obs is None:
        raise ValueError("predictive_check_counts(): obs is required (the observed data the replicates are compared with)")
    device = int(kwargs.pop("device", 0))

    site_covs, obs_covs, obs, session_duration, _, _ = prepare_data(site_covs, obs_covs, obs, session_duration)
    if obs.ndim != 4 or obs.shape[1:] != np.shape(obs_covs)[:3]:
        raise ValueError("predictive_check_counts(): obs must be of shape (n_species, n_sites, n_periods, n_replicates) matching obs_covs")
    posterior = mcmc.get_samples()
    beta = np.asarray(posterior["beta"], dtype=np.float32)    # (n, S, Ks+1)
    alpha = np.asarray(posterior["alpha"], dtype=np.float32)  # (n, S, Ko+1)
    n, n_species = beta.shape[0], beta.shape[1]
    if obs.shape[0] != n_species:
        raise ValueError(f"predictive_check_counts(): obs has {obs.shape[0]} species, the posterior {n_species}")

    # the handles are predict()'s: the model is called with the observations withheld (an all-missing array of the fitted species count)
    arguments = dict(site_covs=site_covs, obs_covs=obs_covs, session_duration=session_duration)
    valid = {k: v for k, v in arguments.items() if v is not None}
    blank = np.full(obs.shape, np.nan, dtype=np.float32)
    spec = model_fn(**valid, obs=blank, **kwargs)
    if beta.shape[2] != spec.site_covs.shape[1] + 1 or alpha.shape[2] != spec.obs_covs.shape[3] + 1:
        raise ValueError("predictive_check_counts(): covariate counts differ from the fitted model's coefficients")
    N, T, J = spec.obs_covs.shape[:3]
    layout = layout_for(spec, N=N, T=T, J=J, Ks=beta.shape[2] - 1, Ko=alpha.shape[2] - 1)

    by_site = group_by == "site"
    col = 2 * _STATISTICS.index(statistic)
    d_obs, d_rep = np.zeros(n), np.zeros(n)
    with time_limit(timeout):
        for sp in range(n_species):
            ds, draws = species_dataset(spec, sp, device), draws_from_sites(layout, posterior, sp)
            res = ds.predictive_check_counts(draws, obs[sp], seed=(int(random_seed) + (sp << 32)) & (2 ** 64 - 1),
                                             by_site=by_site, by_revisit=not by_site)[0 if by_site else 1]
            ds.close()
            d_obs += res[:, col]
            d_rep += res[:, col + 1]
    return {"p_value": float(np.mean(d_rep > d_obs)), "d_obs": d_obs, "d_rep": d_rep}
