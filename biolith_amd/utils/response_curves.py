"""``response_curves`` -- the posterior of a covariate's average response curve, fused on the HIP engine.

How do occupancy and detection respond to a covariate?  For a logit-link model the honest answer is the *average* response curve
(partial dependence, marginal standardisation): for each grid value ``v`` of one covariate, set that covariate to ``v`` at every site,
leave everything else at each site as it is, and average ``psi`` over the sites, per posterior draw.  (A curve "at the means of the
other covariates" is a different and usually misleading quantity, and needs no device.)  The band around the curve needs the joint
draws.  On the host that is ``V`` modified copies of the data, ``V`` calls of ``predict()`` and a reduction of ``V`` arrays of shape
(n, T, N, S), which a prediction grid of 10^6 cells and thousands of draws cannot form.  A term is a handful of FMAs and one
transcendental, so here one C-ABI call per species -- ``bl_response_curves`` (``include/biolith_hip.h``) -- recomputes every term with
the covariate replaced and reduces it in place: ``n_draws x V`` doubles come back.  BUILDER-DEFINED: the reference has no counterpart.
No NumPyro/JAX, no CPU fallback.
"""
from __future__ import annotations

from typing import Callable, Optional, Sequence

import numpy as np

from .data import prepare_data, species_dataset
from .layout import draws_from_sites, layout_for
from .misc import time_limit
from .regional_totals import checked_weights, summarise
from .site_summary import _checked_probs

_HOST_PATH = "predict() on copies of the data with the covariate set to each value, averaged over the sites per draw, is the host path"
_SIDES = {"site": 0, "obs": 1}


def curve_name(name: str, side: str) -> str:
    """The ``predict()`` name of the site a side's curve is about."""
    if side == "site":
        return "abundance" if name in ("occu_rn", "nmixture") else "psi"
    return "rate_detection" if name == "occu_cop" else "prob_detection"


def checked_side(side) -> str:
    if not isinstance(side, str) or side not in _SIDES:
        raise ValueError(f"response_curves(): side={side!r}, \"site\" or \"obs\"")
    return side


def checked_column(covs, covariate, side: str):
    """Column ``covariate`` of the last axis of the side's prepared covariates, flattened; the index as an int."""
    if covs is None or np.shape(covs)[-1] == 0:
        raise ValueError(f"response_curves(): the {side} side has no covariates")
    K = int(np.shape(covs)[-1])
    if isinstance(covariate, (bool, np.bool_)) or not isinstance(covariate, (int, np.integer)):
        raise ValueError(f"response_curves(): covariate={covariate!r} must be an integer index of the last axis of {side}_covs")
    k = int(covariate)
    if not 0 <= k < K:
        raise ValueError(f"response_curves(): covariate={k} outside 0 .. {K - 1}, the {side} covariates")
    return k, np.asarray(covs)[..., k].reshape(-1)


def grid_values(values, column, n_default: int = 25):
    """``values`` -> (V,) finite float32; ``None``: ``n_default`` points, ``np.linspace`` between the column's ``nanmin`` and ``nanmax``."""
    if values is None:
        finite = column[~np.isnan(column)]
        if finite.size == 0:
            raise ValueError("response_curves(): the covariate is NaN everywhere; pass `values`")
        values = np.linspace(float(finite.min()), float(finite.max()), n_default)
    with np.errstate(over="ignore"):
        v = np.ascontiguousarray(np.asarray(values, dtype=np.float64).reshape(-1).astype(np.float32))
    if v.size == 0:
        raise ValueError("response_curves(): `values` is empty")
    if not np.isfinite(v).all():
        bad = int(np.flatnonzero(~np.isfinite(v))[0])
        raise ValueError(f"response_curves(): values[{bad}]={v[bad]} is not finite as float32")
    return v


def normaliser(side: str, average: bool, weight_sum: float, n_visits: int) -> float:
    """What the totals are divided by: 1 without ``average``; the sum of the weights on the site side, ``T J`` times it on the obs side."""
    if not average:
        return 1.0
    if weight_sum == 0.0:
        raise ValueError("response_curves(): the weights sum to 0, so there is no average; pass average=False for the totals")
    return float(weight_sum) * (n_visits if side == "obs" else 1)


def response_curves(
    model_fn: Callable,
    mcmc,
    site_covs=None,
    obs_covs=None,
    obs=None,
    session_duration=None,
    covariate: int = 0,
    side: str = "site",
    values=None,
    weights=None,
    average: bool = True,
    probs: Sequence[float] = (0.05, 0.5, 0.95),
    timeout: Optional[int] = None,
    **kwargs,
) -> dict:
    """Posterior of the average response curve of one covariate: per posterior draw and grid value, the (weighted) average over the
    sites of ``psi`` (``occu_rn`` / ``nmixture``: ``abundance``) with site covariate ``covariate`` set to the value at every site --
    ``side="site"`` --, or of ``prob_detection`` (``occu_cop``: ``rate_detection``) over all sites and visits with observation
    covariate ``covariate`` set to the value at every visit -- ``side="obs"`` --, with the mean, standard deviation and quantiles over
    the draws.  Everything else at each site -- the other covariates, its random effects -- stays as it is.

    The data and the model's options are passed exactly as to :func:`biolith_amd.utils.predict` and ``regional_totals`` -- typically
    the surveyed sites or a prediction grid; ``obs`` is accepted and ignored, ``device=`` goes through ``kwargs``; ``mcmc`` is the
    ``FitResult.mcmc`` of the fit.  ``covariate`` indexes the last axis of the prepared ``site_covs`` (N, Ks) or ``obs_covs``
    (N, T, J, Ko).  ``values`` are in the units of the arrays as passed; they are rounded to float32 and returned as that.  ``None``:
    25 points, ``np.linspace`` between the column's ``nanmin`` and ``nanmax``.  The replacement applies at every site, one whose own
    value is NaN included.  ``weights`` is (N,) finite float64, may be zero (the site drops out) or negative, ``None`` = 1.

    ``average=True`` divides the totals by the sum of the weights (site side) or by ``T * J`` times it (obs side: every visit counts).
    ``average=False`` returns the totals, e.g. the expected total abundance along the gradient.

    A contrast between two grid values -- ``draws[:, g1] - draws[:, g0]`` -- has a posterior of its own, which the two marginal
    bands do not give: form it from the joint ``draws`` and summarise that.

    The contract, with ``k = covariate``, ``v = r["values"]`` and ``w`` the weights::

        X = site_covs.copy(); X[:, k] = v[g]                              # side="site"
        preds = predict(m, mcmc, site_covs=X, obs_covs=obs_covs, ...)
        r["psi"]["draws"][:, g, :] ~ np.einsum("i,nis->ns", w, preds["psi"][:, 0].astype(np.float64)) / w.sum()

        W = obs_covs.copy(); W[..., k] = v[g]                             # side="obs"
        preds = predict(m, mcmc, site_covs=site_covs, obs_covs=W, ...)
        p = preds["prob_detection"].astype(np.float64)                    # (n, J, T, N, S)
        s = p[:, 0, 0] + p[:, 1, 0] + ... + p[:, J - 1, T - 1]            # (n, N, S): the visits one by one, replicates within periods
        r["prob_detection"]["draws"][:, g, :] ~ np.einsum("i,nis->ns", w, s) / (T * J * w.sum())

    The terms are ``predict()``'s values bit for bit, a site's visits are added in float64 in exactly that order, and the products and
    the sums over the sites are float64 in one fixed order without atomics (``regional_totals``' for one region), so the two differ
    by the rounding of two float64 sums over the sites -- at most ``2 (N - 1) 2^-53 sum_i |w_i v_i|`` over the normaliser, ``v_i`` the
    site's value or its sum over the visits.  A value's column depends on that value alone, not on the other values or their
    number.  The same call returns the same bytes.  Nothing of size (n, V, N) is formed.

    Returns
    -------
    dict
        ``side``, ``covariate``, ``values`` (V,) float32, ``n_sites``, ``weight`` (the sum of the weights), ``probs``, ``n_draws``;
        under the site's ``predict()`` name -- ``psi`` / ``abundance``, ``prob_detection`` / ``rate_detection`` -- ``{"draws":
        (n, V, S), "mean": (V, S), "sd": (V, S), "quantiles": (len(probs), V, S)}`` float64, the species plate last.  ``sd`` uses ddof
        1 (NaN for one draw), ``quantiles`` NumPy's linear method; both are computed on the host from ``draws``.

    Raises
    ------
    TypeError
        ``model_fn`` is not a biolith_amd model.
    NotImplementedError
        ``occu_comb`` and ``occu_dyn`` (their sites are formed on the host).
    ValueError
        ``side`` other than ``"site"`` / ``"obs"``; ``covariate`` not an index of the side's covariates, or a side without covariates;
        ``values`` empty or not finite as float32; ``probs`` outside [0, 1] or empty; ``weights`` of another length than the sites or
        not finite; weights that sum to 0 under ``average=True``; covariate counts that differ from the fitted coefficients.

    Examples
    --------
    >>> from biolith_amd.models import simulate, occu
    >>> from biolith_amd.utils import fit, response_curves
    >>> data, _ = simulate()
    >>> results = fit(occu, **data, num_samples=100, num_warmup=100, num_chains=1)
    >>> r = response_curves(occu, results.mcmc, **data, covariate=0)
    >>> r["values"], r["psi"]["quantiles"][:, :, 0]                        # the grid; 5 %, median, 95 % of the average psi along it
    """
    name = getattr(model_fn, "__biolith_amd_model__", None) if callable(model_fn) else None
    if name is None:
        raise TypeError("response_curves(): model_fn must be a biolith_amd model (biolith_amd.models.occu / occu_rn / ...)")
    if name in ("occu_comb", "occu_dyn"):
        raise NotImplementedError(f"response_curves(): not built for {name} (its sites are formed on the host); {_HOST_PATH}")
    side = checked_side(side)
    q = _checked_probs(probs)
    device = int(kwargs.pop("device", 0))

    site_covs, obs_covs, obs, session_duration, _, _ = prepare_data(site_covs, obs_covs, obs, session_duration)
    n_sites, n_visits = int(np.shape(obs_covs)[0]), int(np.shape(obs_covs)[1]) * int(np.shape(obs_covs)[2])
    k, column = checked_column(site_covs if side == "site" else obs_covs, covariate, side)
    v = grid_values(values, column)
    w = checked_weights(weights, n_sites)
    weight = float(n_sites) if w is None else float(w.sum())
    scale = normaliser(side, bool(average), weight, n_visits)

    posterior = mcmc.get_samples()
    beta = np.asarray(posterior["beta"], dtype=np.float32)    # (n, S, Ks+1)
    alpha = np.asarray(posterior["alpha"], dtype=np.float32)  # (n, S, Ko+1)
    n, n_species = beta.shape[0], beta.shape[1]
    if n == 0:
        raise ValueError("response_curves(): the posterior holds no draws")

    # the handles are predict()'s: the model is called with the observations withheld (an all-missing array of the fitted species count)
    arguments = dict(site_covs=site_covs, obs_covs=obs_covs, session_duration=session_duration)
    valid = {key: a for key, a in arguments.items() if a is not None}
    blank = np.full((n_species,) + np.shape(obs_covs)[:3], np.nan, dtype=np.float32)
    spec = model_fn(**valid, obs=blank, **kwargs)
    if beta.shape[2] != spec.site_covs.shape[1] + 1 or alpha.shape[2] != spec.obs_covs.shape[3] + 1:
        raise ValueError("response_curves(): covariate counts differ from the fitted model's coefficients")
    N, T, J = spec.obs_covs.shape[:3]
    layout = layout_for(spec, N=N, T=T, J=J, Ks=beta.shape[2] - 1, Ko=alpha.shape[2] - 1)

    per_species = []
    with time_limit(timeout):
        for sp in range(n_species):
            ds, draws = species_dataset(spec, sp, device), draws_from_sites(layout, posterior, sp)
            per_species.append(ds.response_curves(draws, _SIDES[side], k, v, weight=w))
            ds.close()

    totals = np.stack(per_species, axis=-1)                                  # (n, V, S)
    out = {"side": side, "covariate": k, "values": v, "n_sites": n_sites, "weight": weight, "probs": q, "n_draws": int(n)}
    out[curve_name(name, side)] = summarise(totals / scale if average else totals, q)
    return out
