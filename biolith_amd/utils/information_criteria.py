"""``information_criteria`` -- WAIC, lppd and deviance of biolith/evaluation/{waic,lppd,deviance}.py, fused on the HIP engine.

``evaluation.waic`` / ``lppd`` / ``deviance`` (and their ``*_manual`` forms) build an (n, J, T, N, S) log-likelihood from ``predict()``'s
arrays on the host and reduce it with ``logsumexp`` and ``var`` over the draws: O(n J T N) memory for four numbers.  Every term is a
function of (seed, draw, period, site, visit) that the device regenerates, so here one C-ABI call per species --
``bl_predictive_density`` (``include/biolith_hip.h``) -- forms the log-likelihood in float64 and reduces it both ways: over the points per
draw, and over the draws per point with a streaming log-sum-exp and a streaming variance.  Nothing of size (n, J, T, N) exists on the
device or on the host.  Served: ``occu`` (with ``false_positives_*`` and / or ``*_random_effects``).  No NumPyro/JAX, no CPU fallback.
"""
from __future__ import annotations

from typing import Callable, Optional

import numpy as np
from scipy.special import logsumexp

from ..evaluation.predictive_density import _valid_obs
from .data import prepare_data, species_dataset
from .layout import draws_from_sites, layout_for
from .misc import time_limit

_FORMS = ["conditional", "marginal"]


def information_criteria(
    model_fn: Callable,
    mcmc,
    site_covs=None,
    obs_covs=None,
    obs=None,
    form: str = "conditional",
    pointwise: bool = False,
    random_seed: int = 0,
    timeout: Optional[int] = None,
    **kwargs,
) -> dict:
    """WAIC, lppd, the effective number of parameters and the deviance of a fitted ``occu`` model over its valid observations.

    The data are passed exactly as to :func:`biolith_amd.utils.fit`; the model's options (``false_positives_*``,
    ``*_random_effects``, priors) and ``device=`` go through ``kwargs``; ``mcmc`` is the ``FitResult.mcmc`` of that fit.  ``obs`` holds
    0, 1 or NaN.  A point is valid as for ``evaluation.waic``: its observation, all of its visit's ``obs_covs`` and all of its site's
    ``site_covs`` are finite.

    ``form="conditional"`` is the log-likelihood of ``evaluation.log_likelihood``: per draw, ``Bernoulli(prob).log_prob(y)`` at the
    latent ``z`` that ``predict()`` draws for the same ``random_seed``, with ``prob = z * prob_detection`` -- or, with a false-positive
    rate, ``1 - (1 - z p)(1 - f_c)(1 - (1 - z) f_u)`` -- clamped to float32's ``[tiny, 1 - eps]``.  ``form="marginal"`` is
    ``log_likelihood_manual``'s: ``y log(psi p) + (1 - y) log(1 - psi p)`` with both arguments clipped to ``[1e-10, 1 - 1e-10]``; it
    needs no generator and ignores a false-positive rate, as on the host.  Either is evaluated in float64 from the float32 ``psi``,
    ``prob_detection`` and rate.

    The contract::

        ic = information_criteria(m, mcmc, **data, random_seed=r)
        preds = predict(m, mcmc, **data, random_seed=r)
        ic["waic"], ic["lppd"], ic["p_waic"]  ~  evaluation.waic(m, preds, **data)
        ic["deviance"]                        ~  evaluation.deviance(m, preds, **data)
        form="marginal"  ~  waic_manual(preds, data) / lppd_manual(preds, data) / deviance_manual(preds, data)

    ``z`` is ``predict()``'s bit for bit, and ``psi`` and ``prob_detection`` are its float32 values.  The conditional form differs from
    the host path only by the host's float32 evaluation of ``log``: each term by at most about 1e-5, the totals by about 1e-5 relative.
    With a false-positive rate the host forms ``prob_detection_fp`` in float32 and the device in float64, which near ``prob = 1 - eps``
    is a visible difference, so those handles are not promised to the same tolerance.  (The rate itself is the float32 site value of the
    engine's coordinate ``logit(rate)``, which a float32 posterior site reproduces to about 1e-7.)  The marginal form is float64 on
    both sides and agrees to the order of the additions.

    Returns
    -------
    dict
        ``lppd`` = ``sum_i log mean_q p(y_i | theta_q)``, ``p_waic`` = ``sum_i var_q log p(y_i | theta_q)`` (ddof 1; NaN for a single
        draw), ``waic`` = ``-2 (lppd - p_waic)`` and ``deviance`` = ``-2 (logsumexp(log_lik_draw) - log n)``, floats; ``n_points`` int,
        the number of valid observations; ``log_lik_draw`` (n,) float64, the sum of the valid points' log-likelihood per draw, summed
        over the species plate.  With ``pointwise=True`` also ``lppd_i`` and ``p_waic_i``, (S, N, T, J) float64, NaN where the point
        is not valid.  Sums run in a fixed order: the same call returns the same bytes.

    Examples
    --------
    >>> from biolith_amd.models import simulate, occu
    >>> from biolith_amd.utils import fit, information_criteria
    >>> data, _ = simulate()
    >>> results = fit(occu, **data, num_samples=100, num_warmup=100, num_chains=1)
    >>> information_criteria(occu, results.mcmc, **data)["waic"]
    """
    name = getattr(model_fn, "__biolith_amd_model__", None) if callable(model_fn) else None
    if name is None:
        raise TypeError("information_criteria(): model_fn must be a biolith_amd model (biolith_amd.models.occu)")
    if name != "occu":
        raise NotImplementedError(f"information_criteria(): not built for {name} (built: occu with or without false positives / random "
                                  "effects); evaluation.waic / lppd / deviance on predict()'s output is the host path")
    if form not in _FORMS:
        raise ValueError(f"`form` must be one of {_FORMS}")
    if obs is None:
        raise ValueError("information_criteria(): obs is required (the observations whose likelihood is scored)")
    device = int(kwargs.pop("device", 0))
    kwargs.pop("session_duration", None)   # (occu takes none; predict() accepts and ignores it)

    site_covs, obs_covs, obs, _, _, _ = prepare_data(site_covs, obs_covs, obs, None)
    if obs.ndim != 4 or obs.shape[1:] != np.shape(obs_covs)[:3]:
        raise ValueError("information_criteria(): obs must be of shape (n_species, n_sites, n_periods, n_replicates) matching obs_covs")
    posterior = mcmc.get_samples()
    beta = np.asarray(posterior["beta"], dtype=np.float32)    # (n, S, Ks+1)
    alpha = np.asarray(posterior["alpha"], dtype=np.float32)  # (n, S, Ko+1)
    n, n_species = beta.shape[0], beta.shape[1]
    if obs.shape[0] != n_species:
        raise ValueError(f"information_criteria(): obs has {obs.shape[0]} species, the posterior {n_species}")

    # the handles are predict()'s: the model is called with the observations withheld (an all-missing array of the fitted species count)
    blank = np.full(obs.shape, np.nan, dtype=np.float32)
    spec = model_fn(site_covs=site_covs, obs_covs=obs_covs, obs=blank, **kwargs)
    if beta.shape[2] != spec.site_covs.shape[1] + 1 or alpha.shape[2] != spec.obs_covs.shape[3] + 1:
        raise ValueError("information_criteria(): covariate counts differ from the fitted model's coefficients")
    N, T, J = spec.obs_covs.shape[:3]
    layout = layout_for(spec, N=N, T=T, J=J, Ks=beta.shape[2] - 1, Ko=alpha.shape[2] - 1)

    valid = _valid_obs(site_covs, obs_covs, obs)                             # (S, N, T, J)
    points = np.where(valid, np.asarray(obs, dtype=np.float32), np.nan)      # the mask folded into the observations: NaN = not a point
    log_lik_draw = np.zeros(n)
    lppd_i, p_waic_i = np.full(obs.shape, np.nan), np.full(obs.shape, np.nan)
    with time_limit(timeout):
        for sp in range(n_species):
            ds, draws = species_dataset(spec, sp, device), draws_from_sites(layout, posterior, sp)
            per_draw, lse, var = ds.predictive_density(draws, points[sp], seed=(int(random_seed) + (sp << 32)) & (2 ** 64 - 1),
                                                       marginal=form == "marginal")
            ds.close()
            log_lik_draw += per_draw
            lppd_i[sp][valid[sp]] = lse[valid[sp]]
            p_waic_i[sp][valid[sp]] = var[valid[sp]] if n > 1 else np.nan   # (np.var(ddof=1) of one draw)
    lppd = float(np.sum(lppd_i[valid]))
    p_waic = float(np.sum(p_waic_i[valid]))
    out = {"lppd": lppd, "p_waic": p_waic, "waic": -2 * (lppd - p_waic),
           "deviance": float(-2.0 * (logsumexp(log_lik_draw) - np.log(n))), "n_points": int(valid.sum()), "log_lik_draw": log_lik_draw}
    if pointwise:
        out["lppd_i"], out["p_waic_i"] = lppd_i, p_waic_i
    return out
