"""``species_richness`` -- the posterior of the number of species a cell holds, across the species of one fit, fused on the HIP engine.

``fit(occu, ...)`` samples several species under one chain (the ``species`` plate), and every other post-fit product keeps them apart:
one handle per species, a species axis whose columns never meet.  The question a multi-species fit exists to answer is about the
community -- how many species does a cell hold, where are the rich cells, how much of a stratum holds at least *k* species, and how
sure are we.  Per draw the number of species at a site is Poisson-binomial in the site's ``psi_s``; over the draws the species are
coupled (one chain, perhaps a shared false-positive rate or random-effect sds), so the sd of expected richness, the pmf of richness
and the area with at least *k* species need the joint draws, not the marginals ``regional_totals`` and ``site_summary`` return.  On
the host that is ``predict()``'s (n, T, N, S) ``psi`` followed by a recursion over the species per draw and site.  Here one C-ABI call
-- ``bl_species_richness`` (``include/biolith_hip.h``) -- on ONE handle recomputes every ``psi`` and runs the recursion in registers.
BUILDER-DEFINED: the reference has no counterpart.  No NumPyro/JAX, no CPU fallback.
"""
from __future__ import annotations

from typing import Callable, Optional, Sequence

import numpy as np

from .. import _ffi
from .data import prepare_data, species_dataset
from .layout import draws_from_sites, layout_for
from .misc import time_limit
from .regional_totals import checked_weights, region_index, region_sizes, summarise
from .site_summary import _checked_probs


def pmf_quantiles(pmf, q):
    """The integer quantiles of pmfs (..., S + 1) over 0 .. S: per ``q`` the smallest ``r`` with ``cumsum(pmf)[r] >= q``, clipped to
    ``S`` (a cumulative sum that rounding leaves below ``q``) -> (len(q), ...) int64."""
    cum = np.cumsum(np.asarray(pmf, dtype=np.float64), axis=-1)
    S = cum.shape[-1] - 1
    return np.stack([np.minimum((cum < qq).sum(axis=-1), S) for qq in np.asarray(q, dtype=np.float64).reshape(-1)]).astype(np.int64)


def species_richness(
    model_fn: Callable,
    mcmc,
    site_covs=None,
    obs_covs=None,
    obs=None,
    regions=None,
    weights=None,
    probs: Sequence[float] = (0.05, 0.5, 0.95),
    per_site: bool = True,
    timeout: Optional[int] = None,
    **kwargs,
) -> dict:
    """Posterior of species richness across the S species of one ``fit(occu, ...)``: per site the pmf of the number of species
    present, per posterior draw and region the weighted area that holds exactly / at least ``r`` species, and the total expected
    richness, with their mean, standard deviation and quantiles over the draws.

    The data and the model's options are passed exactly as to :func:`biolith_amd.utils.predict` /
    :func:`biolith_amd.utils.regional_totals` -- typically a prediction grid of new, unsurveyed sites; ``obs`` is accepted and
    ignored, ``device=`` goes through ``kwargs``; ``mcmc`` is the ``FitResult.mcmc`` of the fit.  ``regions``, ``weights`` and
    ``probs`` are ``regional_totals``'.  One handle is opened whatever S is; at most 32 species.

    The definition, per draw ``n`` and site ``i``, with ``psi = predict(...)["psi"][n, 0, i, :]`` (float32, bit for bit) widened to
    float64: the species are present independently with probability ``psi_s``, so the number present has the Poisson-binomial pmf::

        pi = [1, 0, ..., 0]                                     # S + 1 entries
        for s in range(S): pi[1:], pi[0] = pi[1:] * (1 - psi[s]) + pi[:-1] * psi[s], pi[0] * (1 - psi[s])

    and ``E = psi.sum()``.  ``site["pmf"]`` is the mean of ``pi`` over the draws, ``site["expected"]`` the mean and sd (ddof 1) of
    ``E`` over the draws -- the sd is the posterior uncertainty of the expected richness, which the pmf's own sd (``site["sd"]``, the
    spread of the realised number) does not separate.  ``area["draws"][n, r, g] = sum_{i in g} w_i pi[n, i, r]``, float64 products
    summed in ``regional_totals``' fixed order without atomics.  The same call returns the same bytes; nothing of size (n, N) is
    formed.

    This is richness with the observations WITHHELD.  Richness given the data at surveyed sites -- ``P(z_s = 1 | y, theta)`` in place
    of ``psi`` -- needs every species' observations in one launch and is not built; ``conditional_occupancy`` gives that probability
    per species.  ``predict()``'s ``z`` summed over the species axis remains the realised count.

    Returns
    -------
    dict
        ``n_species``, ``n_draws``, ``probs``, ``regions`` (G,) the labels, ``n_sites`` (G,) int, ``weight`` (G,) the regions' sums of
        weights; with ``per_site`` ``site``: ``{"pmf": (N, S + 1), "mean": (N,) = sum_r r pmf, "sd": (N,) of the pmf, "quantiles":
        (len(probs), N) int -- the smallest r with cumsum(pmf) >= q --, "expected": {"mean": (N,), "sd": (N,)}}``; and three
        summaries ``{"draws", "mean", "sd", "quantiles"}`` over the draws (``sd`` ddof 1, NaN for one draw; ``quantiles`` NumPy's
        linear method): ``area`` with ``draws`` (n, S + 1, G), ``at_least`` with ``draws`` (n, S + 1, G), row ``r`` the area with at
        least ``r`` species (the reversed cumulative sum of ``area`` over ``r``, on the host), and ``richness`` with ``draws`` (n, G)
        ``= sum_r r area``, the total expected richness -- divided by ``weight`` the mean per unit.

    Raises
    ------
    TypeError
        ``model_fn`` is not a biolith_amd model.
    NotImplementedError
        every model but ``occu``: the count models fit one species per call, ``occu_comb`` and ``occu_dyn`` are not served.
    ValueError
        the posterior holds no draws or non-finite ones; more than 32 species; covariate counts that differ from the fitted
        coefficients; ``probs`` outside [0, 1] or empty; ``regions`` / ``weights`` of another length than the sites; a non-finite
        weight; no site in any region.

    Examples
    --------
    >>> from biolith_amd.models import simulate, occu
    >>> from biolith_amd.utils import fit, species_richness
    >>> data, _ = simulate(n_species=3)
    >>> results = fit(occu, **data, num_samples=100, num_warmup=100, num_chains=1)
    >>> out = species_richness(occu, results.mcmc, **data)
    >>> out["at_least"]["quantiles"][:, 2, 0]     # sites holding at least two of the three species: 5 %, median, 95 %
    """
    name = getattr(model_fn, "__biolith_amd_model__", None) if callable(model_fn) else None
    if name is None:
        raise TypeError("species_richness(): model_fn must be a biolith_amd model (biolith_amd.models.occu)")
    if name != "occu":
        raise NotImplementedError(f"species_richness(): built for occu alone, not for {name}: the count models fit one species per call "
                                  "and have no richness across species; occu_comb and occu_dyn are not served")
    q = _checked_probs(probs)
    device = int(kwargs.pop("device", 0))

    site_covs, obs_covs, obs, _, _, _ = prepare_data(site_covs, obs_covs, obs, None)
    n_sites = int(np.shape(obs_covs)[0])
    labels, index = region_index(regions, n_sites)
    w = checked_weights(weights, n_sites)
    counts, weight = region_sizes(index, w, labels.size)

    posterior = mcmc.get_samples()
    beta = np.asarray(posterior["beta"], dtype=np.float32)    # (n, S, Ks+1)
    alpha = np.asarray(posterior["alpha"], dtype=np.float32)  # (n, S, Ko+1)
    n, S = beta.shape[0], beta.shape[1]
    if n == 0:
        raise ValueError("species_richness(): the posterior holds no draws")
    if S > _ffi.RICHNESS_MAX_SPECIES:
        raise ValueError(f"species_richness(): {S} species, at most {_ffi.RICHNESS_MAX_SPECIES}")

    # the handle is species 0's, made as regional_totals makes it: the model is called with the observations withheld
    valid = {k: v for k, v in dict(site_covs=site_covs, obs_covs=obs_covs).items() if v is not None}
    blank = np.full((S,) + np.shape(obs_covs)[:3], np.nan, dtype=np.float32)
    spec = model_fn(**valid, obs=blank, **kwargs)
    if beta.shape[2] != spec.site_covs.shape[1] + 1 or alpha.shape[2] != spec.obs_covs.shape[3] + 1:
        raise ValueError("species_richness(): covariate counts differ from the fitted model's coefficients")
    N, T, J = spec.obs_covs.shape[:3]
    layout = layout_for(spec, N=N, T=T, J=J, Ks=beta.shape[2] - 1, Ko=alpha.shape[2] - 1)
    draws = np.ascontiguousarray(np.stack([draws_from_sites(layout, posterior, sp) for sp in range(S)], axis=1), dtype=np.float32)   # (n, S, D)
    if not np.isfinite(draws).all():
        raise ValueError("species_richness(): the posterior holds non-finite draws")

    with time_limit(timeout):
        ds = species_dataset(spec, 0, device)
        try:
            pmf, e_mean, e_sd, area = ds.species_richness(draws, index, labels.size, weight=w, site=bool(per_site), area=True)
        finally:
            ds.close()

    out = {"n_species": int(S), "n_draws": int(n), "probs": q, "regions": labels, "n_sites": counts, "weight": weight}
    r = np.arange(S + 1, dtype=np.float64)
    if per_site:
        mean = pmf @ r
        out["site"] = {"pmf": pmf, "mean": mean, "sd": np.sqrt(np.maximum(pmf @ (r * r) - mean * mean, 0.0)),
                       "quantiles": pmf_quantiles(pmf, q), "expected": {"mean": e_mean, "sd": e_sd}}
    out["area"] = summarise(area, q)                                                      # (n, S + 1, G)
    out["at_least"] = summarise(np.cumsum(area[:, ::-1], axis=1)[:, ::-1].copy(), q)      # (n, S + 1, G)
    out["richness"] = summarise(np.einsum("r,nrg->ng", r, area), q)                       # (n, G)
    return out
