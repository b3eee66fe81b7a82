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

from ._conditional import _unmasked, plate_last, prepare
from .mcmc import LazySamples


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
    c = prepare("conditional_occupancy", "occu with or without false positives / random effects, and occu_comb",
                ("occu_dyn", "occu_cs", "occu_cop"), model_fn, mcmc, site_covs, obs_covs, obs, kwargs)
    comb, ex, n_obs = c.spec.model == "occu_comb", c.spec.extras, c.n_obs
    if comb:
        sc_ok = ~(np.isnan(ex["scores_obs"]) | c.site_nan[None, :, None, None])
        n_obs = n_obs + _unmasked(ex["ARU_obs"], ex["ARU_obs_covs"], c.site_nan) + sc_ok.sum(-1)

    def body(ds, draws, sp, seed):
        if comb:   # (bl_deterministic does not serve occu_comb: psi as fit forms it, from the beta block)
            blk = c.layout["beta"]
            coef = draws[:, blk.offset: blk.offset + blk.width]
            p = (1.0 / (1.0 + np.exp(-(coef[:, :1] + coef[:, 1:] @ np.nan_to_num(c.X).T)))).astype(np.float32)
            psi = np.ascontiguousarray(np.broadcast_to(p[:, None], (len(draws), ds.T, ds.N)))
        else:
            psi = ds.deterministic(draws, psi=True, prob_detection=False)[0]
        log_lik, z_prob, z = ds.site_posterior(draws, seed=seed)
        return psi, z_prob, z, log_lik

    psi, z_prob, z, log_lik = c.per_species(random_seed, timeout, body)   # (n, T, N, S)
    return LazySamples(psi=psi, z_prob=z_prob, z=z.astype(np.int32), log_lik=log_lik, n_obs=plate_last(n_obs))
