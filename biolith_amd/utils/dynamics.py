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

from .data import prepare_data, species_dataset
from .latent import _unmasked
from .layout import draws_from_sites, layout_for
from .mcmc import LazySamples
from .misc import time_limit

SERVED = ("occu_dyn",)


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
    name = getattr(model_fn, "__biolith_amd_model__", None) if callable(model_fn) else None
    if name is None:
        raise TypeError("conditional_dynamics(): model_fn must be a biolith_amd model (biolith_amd.models.occu_dyn)")
    if name not in SERVED:
        hint = ("; use conditional_occupancy" if name in ("occu", "occu_comb") else
                "; use conditional_abundance" if name in ("occu_rn", "nmixture") else "")
        raise NotImplementedError(f"conditional_dynamics(): not built for {name} (built: occu_dyn, the one model with a latent trajectory){hint}")
    device = int(kwargs.pop("device", 0))
    site_covs, obs_covs, obs, _, _, _ = prepare_data(site_covs, obs_covs, obs, None)
    valid = {k: v for k, v in dict(site_covs=site_covs, obs_covs=obs_covs, obs=obs).items() if v is not None}
    spec = model_fn(**valid, **kwargs)
    posterior = mcmc.get_samples()
    coef = {k: np.asarray(posterior[k], dtype=np.float32) for k in ("beta", "beta_col", "beta_ext")}     # (n, S, Ks+1)
    n, n_species = coef["beta"].shape[0], coef["beta"].shape[1]
    if n_species != spec.obs.shape[0] or any(c.shape[2] != spec.site_covs.shape[1] + 1 for c in coef.values()):
        raise ValueError("conditional_dynamics(): the data differ from the fitted model's (species or site covariate count)")
    if np.asarray(posterior["alpha"]).shape[2] != spec.obs_covs.shape[3] + 1:
        raise ValueError("conditional_dynamics(): covariate counts differ from the fitted model's coefficients")

    X = np.asarray(spec.site_covs, dtype=np.float32)
    n_obs_period = _unmasked(spec.obs, spec.obs_covs, np.isnan(X).any(-1))                                # (S, N, T)
    N, T, J, Ko = spec.obs_covs.shape
    layout = layout_for(spec, N=N, T=T, J=J, Ks=X.shape[1], Ko=Ko)
    Xc = np.nan_to_num(X)

    def site(block, sp):   # (n, N): the fit's own deterministic sites (utils/fit.py: _assemble_dyn)
        b = block[:, sp, :]
        return (1.0 / (1.0 + np.exp(-(b[:, :1] + b[:, 1:] @ Xc.T)))).astype(np.float32)

    rates = {k: [] for k in coef}
    ll, q, col, ext, z = [], [], [], [], []
    with time_limit(timeout):
        for sp in range(n_species):
            ds, draws = species_dataset(spec, sp, device), draws_from_sites(layout, posterior, sp)
            for k in coef:
                rates[k].append(site(coef[k], sp))
            out = ds.path_posterior(draws, seed=(int(random_seed) + (sp << 32)) & (2 ** 64 - 1))
            for acc, a in zip((ll, q, col, ext, z), out):
                acc.append(a)
            ds.close()
    out = LazySamples()
    out["psi"], out["gamma"], out["epsilon"] = (np.stack(rates[k], axis=-1) for k in ("beta", "beta_col", "beta_ext"))   # (n, N, S)
    out["z_prob"] = np.stack(q, axis=-1)                                  # (n, T, N, S)
    out["z"] = np.stack(z, axis=-1).astype(np.int32)
    out["col_prob"] = np.stack(col, axis=-1)                              # (n, T - 1, N, S)
    out["ext_prob"] = np.stack(ext, axis=-1)
    out["log_lik"] = np.stack(ll, axis=-1)                                # (n, N, S)
    out["n_obs"] = np.ascontiguousarray(n_obs_period.sum(-1).T).astype(np.int32)                  # (S, N) -> (N, S)
    out["n_obs_period"] = np.ascontiguousarray(n_obs_period.transpose(2, 1, 0)).astype(np.int32)  # (S, N, T) -> (T, N, S)
    return out
