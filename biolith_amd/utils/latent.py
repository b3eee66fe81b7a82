"""``conditional_occupancy`` -- the occupancy state GIVEN the data, per posterior draw.

BUILDER-DEFINED, no counterpart in the reference: biolith/utils/predict.py withholds the observations (predict.py:78-80), so its
``z`` is a draw from the prior Bernoulli(psi) and a site with detections can come back unoccupied.  Here, per posterior draw and
(period, site), the engine returns what the sampler's density kernels form and discard (``include/biolith_hip.h``:
``bl_site_posterior``): with A = log psi + log p(obs | z = 1) and B = log(1 - psi) + log p(obs | z = 0) over that cell's unmasked
observations, ``log_lik = logaddexp(A, B)``, ``z_prob = exp(A - log_lik) = P(z = 1 | obs, theta)`` and ``z ~ Bernoulli(z_prob)``.
Served: ``occu`` (with ``false_positives_*`` and / or ``*_random_effects``) and ``occu_comb``.  No NumPyro/JAX, no CPU fallback.
"""
from __future__ import annotations

from typing import Callable, Optional

import numpy as np

from .data import prepare_data, species_dataset
from .layout import draws_from_sites, layout_for
from .mcmc import LazySamples
from .misc import time_limit

SERVED = ("occu", "occu_comb")


def _unmasked(obs, covs, site_nan):
    """(S, N, T) count of a block's replicates that enter the likelihood: y, its covariates and the site's covariates all present."""
    ok = ~(np.isnan(obs) | np.isnan(covs).any(-1)[None] | site_nan[None, :, None, None])
    return ok.sum(-1)


def conditional_occupancy(
    model_fn: Callable,
    mcmc,
    site_covs=None,
    obs_covs=None,
    obs=None,
    random_seed: int = 0,
    timeout: Optional[int] = None,
    **kwargs,
) -> LazySamples:
    """Conditional occupancy of a fitted ``occu`` / ``occu_comb`` model for every posterior draw.

    The data are passed exactly as to :func:`biolith_amd.utils.fit` for that model (``occu_comb``: the ``PC_*`` / ``ARU_*`` /
    ``scores_obs`` keywords); the model's options (``false_positives_*``, ``*_random_effects``, priors) and ``device=`` go through
    ``kwargs``; ``mcmc`` is the ``FitResult.mcmc`` of that fit.

    Returns
    -------
    LazySamples
        species plate last, n = posterior draws:
        ``psi`` (n, T, N, S) float32; ``z_prob`` (n, T, N, S) float32 = P(z = 1 | the cell's data, theta);
        ``z`` (n, T, N, S) int32 ~ Bernoulli(z_prob), a function of (random_seed, draw, period, site);
        ``log_lik`` (n, T, N, S) float32, the z-marginalised log-likelihood of the cell's unmasked observations (its sum over cells is
        the model's log-likelihood); ``n_obs`` (T, N, S) int32, the unmasked observations behind each cell.  A cell with
        ``n_obs == 0`` has ``log_lik == 0`` and ``z_prob == psi``.  ``z`` and ``psi`` carry ``predict()``'s names and shapes:
        ``residuals({**preds, "z": lat["z"]}, obs)`` gives Wright et al.'s occupancy residual with z drawn given y.

    Examples
    --------
    >>> from biolith_amd.models import simulate, occu
    >>> from biolith_amd.utils import fit, conditional_occupancy
    >>> data, _ = simulate()
    >>> results = fit(occu, **data, num_samples=10, num_warmup=10, num_chains=1)
    >>> lat = conditional_occupancy(occu, results.mcmc, **data)
    """
    name = getattr(model_fn, "__biolith_amd_model__", None) if callable(model_fn) else None
    if name is None:
        raise TypeError("conditional_occupancy(): model_fn must be a biolith_amd model (biolith_amd.models.occu / occu_comb)")
    if name not in SERVED:
        hint = "; use conditional_dynamics" if name == "occu_dyn" else ""
        raise NotImplementedError(f"conditional_occupancy(): not built for {name} (built: occu with or without false positives / random "
                                  f"effects, and occu_comb){hint}")
    device = int(kwargs.pop("device", 0))
    site_covs, obs_covs, obs, _, _, _ = prepare_data(site_covs, obs_covs, obs, None)
    valid = {k: v for k, v in dict(site_covs=site_covs, obs_covs=obs_covs, obs=obs).items() if v is not None}
    spec = model_fn(**valid, **kwargs)
    posterior = mcmc.get_samples()
    beta = np.asarray(posterior["beta"], dtype=np.float32)    # (n, S, Ks+1)
    n, n_species = beta.shape[0], beta.shape[1]
    if n_species != spec.obs.shape[0] or beta.shape[2] != spec.site_covs.shape[1] + 1:
        raise ValueError("conditional_occupancy(): the data differ from the fitted model's (species or site covariate count)")

    X = np.asarray(spec.site_covs, dtype=np.float32)
    site_nan = np.isnan(X).any(-1)
    n_obs = _unmasked(spec.obs, spec.obs_covs, site_nan)
    ex = spec.extras
    if spec.model == "occu_comb":
        sc_ok = ~(np.isnan(ex["scores_obs"]) | site_nan[None, :, None, None])
        n_obs = n_obs + _unmasked(ex["ARU_obs"], ex["ARU_obs_covs"], site_nan) + sc_ok.sum(-1)
    elif np.asarray(posterior["alpha"]).shape[2] != spec.obs_covs.shape[3] + 1:
        raise ValueError("conditional_occupancy(): covariate counts differ from the fitted model's coefficients")
    N, T, J, Ko = spec.obs_covs.shape
    layout = layout_for(spec, N=N, T=T, J=J, Ks=X.shape[1], Ko=Ko, Ka=ex["ARU_obs_covs"].shape[3] if spec.model == "occu_comb" else None)

    psi, ll, q, z = [], [], [], []
    with time_limit(timeout):
        for sp in range(n_species):
            ds, draws = species_dataset(spec, sp, device), draws_from_sites(layout, posterior, sp)
            if spec.model == "occu_comb":   # (bl_deterministic does not serve occu_comb: psi as fit forms it, from the beta block)
                blk = layout["beta"]
                coef = draws[:, blk.offset: blk.offset + blk.width]
                p = (1.0 / (1.0 + np.exp(-(coef[:, :1] + coef[:, 1:] @ np.nan_to_num(X).T)))).astype(np.float32)
                psi.append(np.ascontiguousarray(np.broadcast_to(p[:, None], (n, ds.T, ds.N))))
            else:
                psi.append(ds.deterministic(draws, psi=True, prob_detection=False)[0])
            log_lik, z_prob, z_draw = ds.site_posterior(draws, seed=(int(random_seed) + (sp << 32)) & (2 ** 64 - 1))
            ll.append(log_lik)
            q.append(z_prob)
            z.append(z_draw)
            ds.close()
    out = LazySamples()
    out["psi"] = np.stack(psi, axis=-1)                                   # (n, T, N, S)
    out["z_prob"] = np.stack(q, axis=-1)
    out["z"] = np.stack(z, axis=-1).astype(np.int32)
    out["log_lik"] = np.stack(ll, axis=-1)
    out["n_obs"] = np.ascontiguousarray(n_obs.transpose(2, 1, 0)).astype(np.int32)   # (S, N, T) -> (T, N, S)
    return out
