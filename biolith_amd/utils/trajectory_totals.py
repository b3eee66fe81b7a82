"""``trajectory_totals`` -- the posterior of a fitted ``occu_dyn``'s occupancy over the seasons, totalled over sets of sites, fused on the
HIP engine.

What a dynamic-occupancy study reports are totals over cells of a T-step recursion per posterior draw and cell: the proportion of area
occupied per season, per stratum or for a whole prediction grid; the area colonised and lost between seasons; turnover and growth
rate; the equilibrium occupancy; a forecast past the last surveyed season.  ``conditional_dynamics`` gives the path GIVEN the data, for
surveyed sites; ``predict()`` draws the path on the host and forms (n, T, N) arrays, which a grid of 10^6 cells and thousands of draws
does not allow.  Here one C-ABI call -- ``bl_trajectory_totals`` (``include/biolith_hip.h``) -- runs the recursion per (draw, site) in
float64 and reduces every step in place: ``n_draws x T x n_regions`` doubles come back.  BUILDER-DEFINED, like the model.  No
NumPyro/JAX, no CPU fallback.
"""
from __future__ import annotations

from typing import Callable, Optional, Sequence

import numpy as np

from .data import prepare_data, species_dataset
from .layout import draws_from_sites, layout_for
from .misc import time_limit
from .regional_totals import checked_weights, region_index, region_sizes, summarise
from .site_summary import _checked_probs

EXPECTED = ("occupancy", "colonised", "extinct", "equilibrium")
REALISED = ("z", "z_colonised", "z_extinct")


def _ratio(num, den):
    """``num / den`` in float64, NaN where ``den`` is zero, without a warning."""
    out = np.full(np.broadcast(num, den).shape, np.nan)
    np.divide(num, den, out=out, where=den != 0)
    return out


def trajectory_totals(
    model_fn: Callable,
    mcmc,
    site_covs=None,
    obs_covs=None,
    obs=None,
    n_periods: Optional[int] = None,
    regions=None,
    weights=None,
    probs: Sequence[float] = (0.05, 0.5, 0.95),
    latent: bool = True,
    random_seed: int = 0,
    timeout: Optional[int] = None,
    **kwargs,
) -> dict:
    """Posterior of a fitted ``occu_dyn``'s occupancy trajectory, totalled over regions: per posterior draw, season and region the
    weighted total of the expected occupancy, of the area colonised and lost, the equilibrium, growth rate and turnover and, with
    ``latent``, the same totals of one realised path per draw, with their mean, standard deviation and quantiles over the draws.

    ``mcmc`` is the ``FitResult.mcmc`` of an ``occu_dyn`` fit; the model's options (priors) and ``device=`` go through ``kwargs``.
    ``site_covs`` (N, Ks) are the sites to report on: the fitted sites or a new grid.  The observations are withheld and the kernel
    reads no visit: ``obs`` is accepted and ignored, and of ``obs_covs`` (N, T, J, Ko) only its shape is used -- ``n_periods``, the
    number of seasons T to run, defaults to its T.  ``n_periods`` may exceed the fitted number of seasons: the model is homogeneous
    in time, so that is the forecast.  With ``obs_covs=None``, ``n_periods`` is required.  Either way the device handle is opened on
    the site covariates, an all-zero ``obs_covs`` of shape (N, 1, 1, Ko) and all-missing observations.

    ``regions``, ``weights`` and ``probs`` mean what they mean in :func:`biolith_amd.utils.regional_totals`: labels of any dtype
    ``np.unique`` takes (``None``: one region ``"all"``; a masked or NaN label: in no region), finite float64 weights that may be zero
    or negative (``None`` = 1), and the quantiles' probabilities.

    Per posterior draw and site ``i``, with ``psi_i``, ``gamma_i``, ``eps_i`` the logistic of the three site predictors (coefficients
    ``beta``, ``beta_col``, ``beta_ext``)::

        pi_i1 = psi_i,        pi_i,t+1 = pi_it (1 - eps_i) + (1 - pi_it) gamma_i

        occupancy[n, t, g]   = sum_{i in g} w_i pi_it                           (n, T, G, 1)
        colonised[n, t, g]   = sum_{i in g} w_i (1 - pi_it) gamma_i             (n, T - 1, G, 1)
        extinct[n, t, g]     = sum_{i in g} w_i pi_it eps_i                     (n, T - 1, G, 1)
        equilibrium[n, g]    = sum_{i in g} w_i gamma_i / (gamma_i + eps_i)     (n, G, 1)
        growth_rate[n, t, g] = occupancy[n, t + 1, g] / occupancy[n, t, g]      (n, T - 1, G, 1)
        turnover[n, t, g]    = colonised[n, t, g] / occupancy[n, t + 1, g]      (n, T - 1, G, 1)

    and with ``latent`` one ancestral path per draw, ``z_i1 ~ Bernoulli(psi_i)``, ``z_i,t+1 ~ Bernoulli(z_it ? 1 - eps_i : gamma_i)``::

        z[n, t, g]           = sum_{i in g} w_i z_it                            (n, T, G, 1)
        z_colonised[n, t, g] = sum_{i in g} w_i [z_it = 0, z_i,t+1 = 1]         (n, T - 1, G, 1)
        z_extinct[n, t, g]   = sum_{i in g} w_i [z_it = 1, z_i,t+1 = 0]         (n, T - 1, G, 1)

    The arithmetic is float64 throughout on the device (covariates and coefficients are promoted from float32); ``growth_rate`` and
    ``turnover`` are formed on the host from the draws, in float64, NaN where the denominator is zero.  ``T = 1`` gives per-pair arrays
    of length 0 on their period axis.  The path is drawn by the device's generator -- cell (draw, period, site) takes one uniform of
    ``bl_cell_rng(seed, draw, T, period, N, site)`` -- and not by ``predict()``'s NumPy one: ``z`` here and ``predict()``'s ``z`` share
    a distribution and NOT their values.  The cell's index holds T, so the first seasons of ``occupancy``, ``colonised`` and ``extinct``
    do not depend on ``n_periods`` while the path does.

    A region's rows depend on its own sites, their weights and the draws alone: not on how the other sites are labelled.  The same
    call returns the same bytes: there are no atomics and the order of every sum is fixed.  Nothing of size (n, N) is formed on
    either side; one region per site is served but wasteful (a 64-lane wave per region at the least).

    Returns
    -------
    dict
        ``regions`` (G,) the labels, ``n_sites`` (G,) int, ``weight`` (G,) the regions' sums of weights, ``probs``, ``n_draws``,
        ``n_periods``; under each name above ``{"draws", "mean", "sd", "quantiles"}`` float64 as ``regional_totals`` returns them, the
        species plate (S = 1) last: ``draws`` in the shape given above, ``mean`` and ``sd`` without the draw axis, ``quantiles`` with a
        leading ``len(probs)`` axis.  ``sd`` uses ddof 1 (NaN for one draw), ``quantiles`` NumPy's linear method.

    Raises
    ------
    TypeError
        ``model_fn`` is not a biolith_amd model.
    NotImplementedError
        any model but ``occu_dyn`` (``regional_totals`` serves the static ones).
    ValueError
        ``n_periods < 1``; neither ``n_periods`` nor ``obs_covs`` given; ``probs`` outside [0, 1] or empty; ``regions`` / ``weights``
        of another length than the sites; a non-finite weight; no site in any region; covariate counts that differ from the fitted
        coefficients; an empty posterior.

    Examples
    --------
    >>> from biolith_amd.models import simulate_dyn, occu_dyn
    >>> from biolith_amd.utils import fit, trajectory_totals
    >>> data, _ = simulate_dyn()
    >>> results = fit(occu_dyn, **data, num_samples=100, num_warmup=100, num_chains=1)
    >>> r = trajectory_totals(occu_dyn, results.mcmc, **data, n_periods=10)     # four seasons past the six surveyed
    >>> r["occupancy"]["quantiles"][:, :, 0, 0] / r["weight"][0]                # proportion of area occupied: 5 %, median, 95 %
    """
    name = getattr(model_fn, "__biolith_amd_model__", None) if callable(model_fn) else None
    if name is None:
        raise TypeError("trajectory_totals(): model_fn must be a biolith_amd model (biolith_amd.models.occu_dyn)")
    if name != "occu_dyn":
        raise NotImplementedError(f"trajectory_totals(): not built for {name} (built: occu_dyn, the one model with a latent trajectory); "
                                  "regional_totals serves the static models")
    q = _checked_probs(probs)
    device = int(kwargs.pop("device", 0))

    site_covs, obs_covs, _, _, _, _ = prepare_data(site_covs, obs_covs, None, None)
    if site_covs is None or site_covs.ndim != 2:
        raise ValueError("trajectory_totals(): site_covs (n_sites, n_site_covs) are the sites to report on")
    if n_periods is None and obs_covs is None:
        raise ValueError("trajectory_totals(): give n_periods, or obs_covs whose number of periods to run")
    T = int(np.shape(obs_covs)[1] if n_periods is None else n_periods)
    if T < 1:
        raise ValueError(f"trajectory_totals(): n_periods={T}, at least 1")
    n_sites = int(site_covs.shape[0])
    if obs_covs is not None and np.shape(obs_covs)[0] != n_sites:
        raise ValueError(f"trajectory_totals(): obs_covs holds {np.shape(obs_covs)[0]} sites, site_covs {n_sites}")
    labels, index = region_index(regions, n_sites)
    w = checked_weights(weights, n_sites)
    counts, weight = region_sizes(index, w, labels.size)

    posterior = mcmc.get_samples()
    blocks = [np.asarray(posterior[k], dtype=np.float32) for k in ("beta", "beta_col", "beta_ext")]   # (n, 1, Ks+1)
    alpha = np.asarray(posterior["alpha"], dtype=np.float32)                                            # (n, 1, Ko+1)
    n, Ko = blocks[0].shape[0], alpha.shape[2] - 1
    if n == 0:
        raise ValueError("trajectory_totals(): the posterior holds no draws")
    if any(b.shape[1] != 1 for b in blocks + [alpha]):
        raise ValueError("trajectory_totals(): the posterior holds several species; occu_dyn fits one")
    if any(b.shape[2] != site_covs.shape[1] + 1 for b in blocks) or (obs_covs is not None and np.shape(obs_covs)[3] != Ko):
        raise ValueError("trajectory_totals(): covariate counts differ from the fitted model's coefficients")

    # the handle: the kernel reads the site covariates and no visit, so one all-masked visit per site is all it holds
    spec = model_fn(site_covs=site_covs, obs_covs=np.zeros((n_sites, 1, 1, Ko), dtype=np.float32),
                    obs=np.full((1, n_sites, 1, 1), np.nan, dtype=np.float32), **kwargs)
    layout = layout_for(spec, N=n_sites, T=1, J=1, Ks=site_covs.shape[1], Ko=Ko)
    with time_limit(timeout):
        ds, draws = species_dataset(spec, 0, device), draws_from_sites(layout, posterior, 0)
        res = ds.trajectory_totals(draws, index, labels.size, T, weight=w, seed=int(random_seed) & (2 ** 64 - 1),
                                   outputs=EXPECTED + (REALISED if latent else ()))
        ds.close()

    res = {k: v[..., None] for k, v in res.items()}   # the species plate
    res["growth_rate"] = _ratio(res["occupancy"][:, 1:], res["occupancy"][:, :-1])
    res["turnover"] = _ratio(res["colonised"], res["occupancy"][:, 1:])
    out = {"regions": labels, "n_sites": counts, "weight": weight, "probs": q, "n_draws": int(n), "n_periods": T}
    out.update({k: summarise(v, q) for k, v in res.items()})
    return out
