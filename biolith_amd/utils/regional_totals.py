"""``regional_totals`` -- the posterior of totals over sets of sites, fused on the HIP engine.

The figure an occupancy or abundance study reports is the posterior of a total over a set of cells: the proportion of area occupied,
the occupied area per stratum or reserve, the total abundance per region, the difference between two regions.  The spread and the
quantiles of a sum need the joint draws, not the per-cell marginals of ``site_summary``; on the host that is ``predict()`` followed by
``(w * preds["psi"]).sum(...)`` per draw and region -- an (n, T, N) array per site, which on a prediction grid of 10^6 cells and
thousands of draws cannot be formed.  A term is a handful of FMAs and one transcendental, so here one C-ABI call per species --
``bl_regional_totals`` (``include/biolith_hip.h``) -- recomputes every term and reduces it in place: ``n_draws x n_regions`` doubles
come back.  BUILDER-DEFINED: the reference has no counterpart.  No NumPyro/JAX, no CPU fallback.
"""
from __future__ import annotations

from typing import Callable, Optional, Sequence

import numpy as np

from .data import prepare_data, species_dataset
from .layout import draws_from_sites, layout_for
from .misc import time_limit
from .site_summary import _checked_probs

_HOST_PATH = "predict() followed by (weights * preds[site]).sum over each region's sites per draw is the host path"


def total_names(name: str):
    """The model's first deterministic site and its latent site under ``predict()``'s names."""
    return ("abundance", "N_i") if name in ("occu_rn", "nmixture") else ("psi", "z")


def region_index(regions, n_sites: int):
    """``regions`` -> (labels (G,), index (N,) int32): the labels in ``np.unique`` order and every site's position among them, -1 for a
    site in no region -- one whose label is masked (``np.ma``) or NaN.  ``None``: every site in the one region ``"all"``."""
    if regions is None:
        return np.array(["all"]), np.zeros(n_sites, dtype=np.int32)
    out = np.ma.getmaskarray(regions).reshape(-1).copy() if isinstance(regions, np.ma.MaskedArray) else None
    lab = np.asarray(np.ma.getdata(regions)).reshape(-1)
    if lab.size != n_sites:
        raise ValueError(f"regional_totals(): `regions` holds {lab.size} labels for {n_sites} sites")
    if out is None:
        out = np.zeros(n_sites, dtype=bool)
    if lab.dtype.kind in "fc":
        out |= np.isnan(lab)
    labels, inverse = np.unique(lab[~out], return_inverse=True)
    if labels.size == 0:
        raise ValueError("regional_totals(): every site's label is masked or NaN: no site is in any region")
    index = np.full(n_sites, -1, dtype=np.int32)
    index[~out] = inverse.reshape(-1)
    return labels, index


def checked_weights(weights, n_sites: int):
    """``weights`` -> (N,) float64, ``None`` -> ``None`` (every weight 1)."""
    if weights is None:
        return None
    w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).reshape(-1))
    if w.size != n_sites:
        raise ValueError(f"regional_totals(): `weights` holds {w.size} values for {n_sites} sites")
    if not np.isfinite(w).all():
        bad = int(np.flatnonzero(~np.isfinite(w))[0])
        raise ValueError(f"regional_totals(): weights[{bad}]={w[bad]} is not finite")
    return w


def region_sizes(index, w, n_regions: int):
    """``n_sites`` (G,) int64 and ``weight`` (G,) float64 of the regions: how many sites each holds and the sum of their weights."""
    inside = index >= 0
    counts = np.bincount(index[inside], minlength=n_regions).astype(np.int64)
    weight = np.bincount(index[inside], weights=None if w is None else w[inside], minlength=n_regions).astype(np.float64)
    return counts, weight


def summarise(draws, q):
    """``{"draws", "mean", "sd", "quantiles"}`` over the leading (draw) axis: sd with ddof 1 (NaN for one draw), quantiles by NumPy's
    linear method with a leading ``len(q)`` axis."""
    n = draws.shape[0]
    sd = draws.std(axis=0, ddof=1) if n > 1 else np.full(draws.shape[1:], np.nan)
    return {"draws": draws, "mean": draws.mean(axis=0), "sd": sd, "quantiles": np.quantile(draws, q, axis=0)}


def regional_totals(
    model_fn: Callable,
    mcmc,
    site_covs=None,
    obs_covs=None,
    obs=None,
    session_duration=None,
    regions=None,
    weights=None,
    probs: Sequence[float] = (0.05, 0.5, 0.95),
    latent: bool = True,
    random_seed: int = 0,
    timeout: Optional[int] = None,
    **kwargs,
) -> dict:
    """Posterior of weighted totals over regions: per posterior draw and region, the total of the model's first deterministic site
    (``psi``; ``occu_rn`` / ``nmixture``: ``abundance``) and, with ``latent``, of the latent site ``predict()`` draws for the same
    ``random_seed`` (``z``; ``N_i``), with their mean, standard deviation and quantiles over the draws.

    The data and the model's options are passed exactly as to :func:`biolith_amd.utils.predict` -- typically a prediction grid of new,
    unsurveyed sites; ``obs`` is accepted and ignored, ``device=`` goes through ``kwargs``; ``mcmc`` is the ``FitResult.mcmc`` of the
    fit.  For *surveyed* sites the totals given the data -- ``conditional_occupancy`` / ``conditional_abundance`` with
    ``evaluation.finite_sample_occupancy`` / ``finite_sample_abundance`` -- remain the right tool: here the observations are withheld.

    ``regions`` is an (N,) array of labels of any dtype ``np.unique`` takes (integers, strings, bools); the regions are its distinct
    labels in ``np.unique`` order.  ``None``: every site in the one region ``"all"``.  A site whose label is masked (``np.ma``) or NaN is
    in no region (there is no ``exclude=`` sentinel).  ``weights`` is (N,) finite float64 -- a cell's area, an inclusion weight --, may
    be zero or negative, ``None`` = 1.

    The contract, with ``idx[g]`` the sites of region ``g`` in site order and ``w`` the weights::

        preds = predict(m, mcmc, **data, random_seed=seed)
        r = regional_totals(m, mcmc, **data, regions=R, weights=w, random_seed=seed)
        r["psi"]["draws"][:, g, :] ~ np.einsum("i,nis->ns", w[idx[g]], preds["psi"][:, 0][:, idx[g]].astype(np.float64))
        r["z"]["draws"][:, :, g, :] ~ np.einsum("i,ntis->nts", w[idx[g]], preds["z"][:, :, idx[g]].astype(np.float64))

    The terms are ``predict()``'s values bit for bit; the products and the sums are float64 in one fixed order without atomics, so
    the two differ by the rounding of two float64 sums -- at most ``2 (N_g - 1) 2^-53 sum_i |w_i v_i|`` -- and with ``weights=None`` the
    latent totals, integers, are equal.  A region's totals depend on its own sites, their weights and the draws alone: not on how the
    other sites are labelled.  The same call returns the same bytes.  Nothing of size (n, N) is formed; one region per site is served
    but wasteful (a 64-lane wave per region at the least).

    Returns
    -------
    dict
        ``regions`` (G,) the labels, ``n_sites`` (G,) int, ``weight`` (G,) the regions' sums of weights, ``probs``, ``n_draws``; under
        the first site's name ``{"draws": (n, G, S), "mean": (G, S), "sd": (G, S), "quantiles": (len(probs), G, S)}`` float64, the
        species plate last; with ``latent`` the same under the latent site's name with ``draws`` (n, T, G, S).  ``sd`` uses ddof 1
        (NaN for one draw), ``quantiles`` NumPy's linear method; both are computed on the host from ``draws``.

    Raises
    ------
    TypeError
        ``model_fn`` is not a biolith_amd model.
    NotImplementedError
        ``occu_comb`` and ``occu_dyn`` (their sites are formed on the host).
    ValueError
        ``probs`` outside [0, 1] or empty; ``regions`` / ``weights`` of another length than the sites; a non-finite weight; no site in
        any region; covariate counts that differ from the fitted coefficients.

    Examples
    --------
    >>> from biolith_amd.models import simulate, occu
    >>> from biolith_amd.utils import fit, regional_totals
    >>> data, _ = simulate()
    >>> results = fit(occu, **data, num_samples=100, num_warmup=100, num_chains=1)
    >>> regional_totals(occu, results.mcmc, **data)["z"]["quantiles"][:, 0, 0, 0]     # sites occupied: 5 %, median, 95 %
    """
    name = getattr(model_fn, "__biolith_amd_model__", None) if callable(model_fn) else None
    if name is None:
        raise TypeError("regional_totals(): model_fn must be a biolith_amd model (biolith_amd.models.occu / occu_rn / ...)")
    if name in ("occu_comb", "occu_dyn"):
        raise NotImplementedError(f"regional_totals(): not built for {name} (its sites are formed on the host); {_HOST_PATH}")
    q = _checked_probs(probs)
    device = int(kwargs.pop("device", 0))

    site_covs, obs_covs, obs, session_duration, _, _ = prepare_data(site_covs, obs_covs, obs, session_duration)
    n_sites = int(np.shape(obs_covs)[0])
    labels, index = region_index(regions, n_sites)
    w = checked_weights(weights, n_sites)
    counts, weight = region_sizes(index, w, labels.size)

    posterior = mcmc.get_samples()
    beta = np.asarray(posterior["beta"], dtype=np.float32)    # (n, S, Ks+1)
    alpha = np.asarray(posterior["alpha"], dtype=np.float32)  # (n, S, Ko+1)
    n, n_species = beta.shape[0], beta.shape[1]
    if n == 0:
        raise ValueError("regional_totals(): the posterior holds no draws")

    # the handles are predict()'s: the model is called with the observations withheld (an all-missing array of the fitted species count)
    arguments = dict(site_covs=site_covs, obs_covs=obs_covs, session_duration=session_duration)
    valid = {k: v for k, v in arguments.items() if v is not None}
    blank = np.full((n_species,) + np.shape(obs_covs)[:3], np.nan, dtype=np.float32)
    spec = model_fn(**valid, obs=blank, **kwargs)
    if beta.shape[2] != spec.site_covs.shape[1] + 1 or alpha.shape[2] != spec.obs_covs.shape[3] + 1:
        raise ValueError("regional_totals(): covariate counts differ from the fitted model's coefficients")
    N, T, J = spec.obs_covs.shape[:3]
    layout = layout_for(spec, N=N, T=T, J=J, Ks=beta.shape[2] - 1, Ko=alpha.shape[2] - 1)

    per_species = []
    with time_limit(timeout):
        for sp in range(n_species):
            ds, draws = species_dataset(spec, sp, device), draws_from_sites(layout, posterior, sp)
            per_species.append(ds.regional_totals(draws, index, labels.size, weight=w, seed=(int(random_seed) + (sp << 32)) & (2 ** 64 - 1),
                                                  site=True, latent=bool(latent)))
            ds.close()

    first, second = total_names(name)
    out = {"regions": labels, "n_sites": counts, "weight": weight, "probs": q, "n_draws": int(n)}
    out[first] = summarise(np.stack([res[0] for res in per_species], axis=-1), q)        # (n, G, S)
    if latent:
        out[second] = summarise(np.stack([res[1] for res in per_species], axis=-1), q)   # (n, T, G, S)
    return out
