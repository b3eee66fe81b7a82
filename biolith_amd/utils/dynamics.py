"""``conditional_dynamics`` -- the occupancy trajectory of a fitted ``occu_dyn`` GIVEN the data, per posterior draw.

BUILDER-DEFINED, like the model (models/occu_dyn.py): ``predict()`` draws the path z_1..T ancestrally without the observations, so a
site-season with a detection can come back unoccupied.  The seasons of a site are dependent, so the conditional is not a cell-by-cell
quantity: the engine runs a forward filter, a backward smoother and forward-filtering backward-sampling per posterior draw and site
(``include/biolith_hip.h``: ``bl_path_posterior``) and returns what the sampler's backward pass forms for its gradient and discards --
the smoothed marginals ``P(z_t = 1 | y_1..T, theta)``, the pairwise terms of colonisation and extinction, the site's path-marginalised
log-likelihood -- and one joint draw of the path.  No NumPyro/JAX, no CPU fallback.
"""
from __future__ import annotations

from typing import Callable, Optional

import numpy as np

from ._conditional import plate_last, prepare
from .mcmc import LazySamples


def conditional_dynamics(
    model_fn: Callable,
    mcmc,
    site_covs=None,
    obs_covs=None,
    obs=None,
    random_seed: int = 0,
    timeout: Optional[int] = None,
    **kwargs,
) -> LazySamples:
    """Conditional occupancy dynamics of a fitted ``occu_dyn`` model for every posterior draw.

    The data are passed exactly as to :func:`biolith_amd.utils.fit`; the model's options (priors) and ``device=`` go through
    ``kwargs``; ``mcmc`` is the ``FitResult.mcmc`` of that fit.

    Returns
    -------
    LazySamples
        species plate last, n = posterior draws:
        ``psi``, ``gamma``, ``epsilon`` (n, N, S) float32 as the fit's sites;
        ``z_prob`` (n, T, N, S) float32 = P(z_t = 1 | all seasons' data, theta), the smoothed marginal;
        ``z`` (n, T, N, S) int32, one JOINT draw of the path per posterior draw (forward filtering, backward sampling), a function of
        (random_seed, draw, period, site);
        ``col_prob`` / ``ext_prob`` (n, T - 1, N, S) float32 = P(z_t = 0, z_t+1 = 1 | data, theta) / P(z_t = 1, z_t+1 = 0 | data, theta);
        ``log_lik`` (n, N, S) float32, the site's path-marginalised log-likelihood -- the SITE is the pointwise unit, the level at
        which the dynamic likelihood factorises (its sum over sites is the model's log-likelihood);
        ``n_obs`` (N, S) int32, the site's unmasked visits over all seasons; ``n_obs_period`` (T, N, S) int32, per season.
        A site with ``n_obs == 0`` has ``log_lik == 0`` and ``z_prob`` = the propagated prior; a season with an unmasked detection
        has ``z == 1`` in every draw.  ``log_lik`` and ``n_obs`` feed :func:`biolith_amd.evaluation.lppd_marginal` /
        ``waic_marginal``, ``z`` feeds ``finite_sample_occupancy`` and ``finite_sample_turnover``.

    Examples
    --------
    >>> from biolith_amd.models import simulate_dyn, occu_dyn
    >>> from biolith_amd.utils import fit, conditional_dynamics
    >>> data, _ = simulate_dyn()
    >>> results = fit(occu_dyn, **data, num_samples=10, num_warmup=10, num_chains=1)
    >>> lat = conditional_dynamics(occu_dyn, results.mcmc, **data)
    """
    c = prepare("conditional_dynamics", "occu_dyn, the one model with a latent trajectory",
                ("occu", "occu_comb", "occu_rn", "nmixture", "occu_cs", "occu_cop"), model_fn, mcmc, site_covs, obs_covs, obs, kwargs, coef=("beta", "beta_col", "beta_ext"))
    Xc = np.nan_to_num(c.X)

    def site(block, sp):   # (n, N): the fit's own deterministic sites (utils/fit.py: _assemble_dyn)
        b = block[:, sp, :]
        return (1.0 / (1.0 + np.exp(-(b[:, :1] + b[:, 1:] @ Xc.T)))).astype(np.float32)

    def body(ds, draws, sp, seed):
        log_lik, z_prob, col, ext, z = ds.path_posterior(draws, seed=seed)
        return tuple(site(c.coef[k], sp) for k in ("beta", "beta_col", "beta_ext")) + (z_prob, z, col, ext, log_lik)

    # rates (n, N, S); z_prob, z (n, T, N, S); the pairs (n, T - 1, N, S); log_lik (n, N, S)
    psi, gamma, eps, z_prob, z, col, ext, log_lik = c.per_species(random_seed, timeout, body)
    return LazySamples(psi=psi, gamma=gamma, epsilon=eps, z_prob=z_prob, z=z.astype(np.int32), col_prob=col, ext_prob=ext, log_lik=log_lik,
                       n_obs=np.ascontiguousarray(c.n_obs.sum(-1).T).astype(np.int32),   # (S, N) -> (N, S)
                       n_obs_period=plate_last(c.n_obs))
