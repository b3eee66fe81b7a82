"""``site_summary`` -- the posterior mean, spread and quantiles of a fitted model's deterministic sites, fused on the HIP engine.

The table every user builds after a fit -- ``psi`` per site, ``prob_detection`` per visit, each with its mean, its standard deviation
and a credible interval -- is, on the host, ``predict()`` followed by ``np.mean``, ``np.std`` and ``np.quantile`` over the draw axis:
an (n, J, T, N) float32 array written to the host and sorted along its strided axis.  A deterministic site's value at (draw, cell) is a
handful of FMAs, so here one C-ABI call per species -- ``bl_site_summary`` (``include/biolith_hip.h``) -- recomputes it as often as the
reductions want and stores nothing: two passes in float64 for the mean and the standard deviation, and a select that finds the order
statistics the quantiles interpolate between.  Nothing of size (n, T, N) or (n, J, T, N) exists on the device or on the host, and the
draw count is not limited.  BUILDER-DEFINED: the reference has no counterpart.  ``evaluation.summary`` is the host function for
*sampled* sites shaped (chains, draws, ...).  No NumPyro/JAX, no CPU fallback.
"""
from __future__ import annotations

from typing import Callable, Optional, Sequence

import numpy as np

from .. import _ffi
from .data import prepare_data, species_dataset
from .layout import draws_from_sites, layout_for
from .misc import time_limit

_HOST_PATH = "predict() followed by np.mean / np.std / np.quantile over the draw axis is the host path"


def site_names(name: str):
    """The model's two deterministic sites under ``predict()``'s names: per (period, site), and per (replicate, period, site)."""
    return ("abundance" if name in ("occu_rn", "nmixture") else "psi", "rate_detection" if name == "occu_cop" else "prob_detection")


def quantile_ranks(probs, n: int):
    """The order statistics that the quantiles ``probs`` of ``n`` values interpolate between (NumPy's ``method="linear"``):
    ``lo = floor((n - 1) q)``, ``hi = min(lo + 1, n - 1)`` and the weight ``g = (n - 1) q - lo`` of ``hi``, each (len(probs),); and
    ``ranks``, the distinct values of ``lo`` and ``hi``, ascending.  ``probs`` outside [0, 1], empty, or needing more than
    ``SUMMARY_MAX_RANKS`` ranks: ``ValueError``."""
    q = _checked_probs(probs)
    pos = (n - 1) * q
    lo = np.minimum(np.floor(pos).astype(np.int64), n - 1)
    hi = np.minimum(lo + 1, n - 1)
    ranks = np.unique(np.concatenate([lo, hi]))
    if ranks.size > _ffi.SUMMARY_MAX_RANKS:
        raise ValueError(f"site_summary(): `probs` needs {ranks.size} order statistics of {n} draws, at most {_ffi.SUMMARY_MAX_RANKS} "
                         "(eight quantiles in general); ask for fewer at a time")
    return lo, hi, pos - lo, ranks


def interpolate(order, ranks, lo, hi, g):
    """The quantiles from the order statistics: ``order`` (len(ranks), ...) holds the values of ``ranks``; ``a + (b - a) g`` in float64
    with ``a``, ``b`` the values of ranks ``lo`` and ``hi`` -> (len(lo), ...)."""
    order = np.asarray(order, dtype=np.float64)
    a, b = order[np.searchsorted(ranks, lo)], order[np.searchsorted(ranks, hi)]
    return a + (b - a) * np.asarray(g, dtype=np.float64).reshape((-1,) + (1,) * (order.ndim - 1))


def _checked_probs(probs):
    q = np.asarray(probs, dtype=np.float64).reshape(-1)
    if q.size == 0:
        raise ValueError("site_summary(): `probs` is empty")
    if not (np.isfinite(q).all() and (q >= 0).all() and (q <= 1).all()):
        raise ValueError("site_summary(): `probs` must lie in [0, 1]")
    return q


def site_summary(
    model_fn: Callable,
    mcmc,
    site_covs=None,
    obs_covs=None,
    obs=None,
    session_duration=None,
    probs: Sequence[float] = (0.05, 0.5, 0.95),
    sites: Optional[Sequence[str]] = None,
    timeout: Optional[int] = None,
    **kwargs,
) -> dict:
    """Posterior mean, standard deviation and quantiles of a fitted model's deterministic sites, per cell, over all posterior draws.

    The data and the model's options are passed exactly as to :func:`biolith_amd.utils.predict` -- possibly new sites' covariates;
    ``obs`` is accepted and ignored, ``device=`` goes through ``kwargs``; ``mcmc`` is the ``FitResult.mcmc`` of the fit.  ``sites``
    names a subset of the model's two deterministic sites under ``predict()``'s names (default: both): ``psi`` and
    ``prob_detection``; for ``occu_rn`` and ``nmixture`` the first is ``abundance``, for ``occu_cop`` the second is
    ``rate_detection``.

    The contract::

        preds = predict(m, mcmc, **data);  v = preds[name].astype(np.float64)    # (n, ...)
        s = site_summary(m, mcmc, **data, probs=P)[name]
        s["mean"]       ~ v.mean(0)
        s["sd"]         ~ v.std(0, ddof=1)
        s["quantiles"]  ~ np.quantile(v, P, axis=0)

    The values summarised are ``predict()``'s float32 values bit for bit.  The mean and the standard deviation are float64 sums in draw
    order (two passes; NaN standard deviation for a single draw, as ``np.std(ddof=1)``); the order statistics are exact, and the host
    interpolates ``a + (b - a) ((n - 1) q - lo)`` between ranks ``lo = floor((n - 1) q)`` and ``min(lo + 1, n - 1)`` in float64, which
    is NumPy's ``method="linear"`` up to one rounding.  One call serves at most 16 distinct ranks: eight quantiles in general.  The
    equal-tailed quantiles are the promise; the narrowest (HPD) interval is not built.

    Returns
    -------
    dict
        ``{name: {"mean", "sd", "quantiles"}, "probs": (len(probs),) float64, "n_draws": n}``.  The arrays are float64 in ``predict()``'s
        shapes without the draw axis, the species plate last: the first site (T, N, S) -- constant over T --, the second (J, T, N, S);
        ``quantiles`` has a leading axis of length ``len(probs)``.  ``site_names`` / ``obs_names`` renaming does not apply (no
        coefficient is returned).  The same call returns the same bytes.

    Raises
    ------
    NotImplementedError
        ``occu_comb`` and ``occu_dyn`` (their sites are formed on the host).
    ValueError
        Non-finite posterior sites; ``probs`` outside [0, 1], empty, or needing more than 16 ranks; unknown ``sites``; covariate counts
        that differ from the fitted coefficients.

    Examples
    --------
    >>> from biolith_amd.models import simulate, occu
    >>> from biolith_amd.utils import fit, site_summary
    >>> data, _ = simulate()
    >>> results = fit(occu, **data, num_samples=100, num_warmup=100, num_chains=1)
    >>> site_summary(occu, results.mcmc, **data)["psi"]["quantiles"].shape
    """
    name = getattr(model_fn, "__biolith_amd_model__", None) if callable(model_fn) else None
    if name is None:
        raise TypeError("site_summary(): model_fn must be a biolith_amd model (biolith_amd.models.occu / occu_rn / ...)")
    if name in ("occu_comb", "occu_dyn"):
        raise NotImplementedError(f"site_summary(): not built for {name} (its sites are formed on the host); {_HOST_PATH}")
    q = _checked_probs(probs)
    names = site_names(name)
    wanted = names if sites is None else tuple([sites] if isinstance(sites, str) else sites)
    if not wanted or any(s not in names for s in wanted):
        raise ValueError(f"site_summary(): `sites` must name some of {names} for {name}, got {tuple(wanted)}")
    device = int(kwargs.pop("device", 0))

    site_covs, obs_covs, obs, session_duration, _, _ = prepare_data(site_covs, obs_covs, obs, session_duration)
    posterior = mcmc.get_samples()
    for k, val in posterior.items():
        if not np.isfinite(np.asarray(val, dtype=np.float64)).all():
            raise ValueError(f"site_summary(): the posterior site {k!r} holds non-finite draws (the order statistics are not defined for them)")
    beta = np.asarray(posterior["beta"], dtype=np.float32)    # (n, S, Ks+1)
    alpha = np.asarray(posterior["alpha"], dtype=np.float32)  # (n, S, Ko+1)
    n, n_species = beta.shape[0], beta.shape[1]
    if n == 0:
        raise ValueError("site_summary(): the posterior holds no draws")
    lo, hi, g, ranks = quantile_ranks(q, n)

    # the handles are predict()'s: the model is called with the observations withheld (an all-missing array of the fitted species count)
    arguments = dict(site_covs=site_covs, obs_covs=obs_covs, session_duration=session_duration)
    valid = {k: v for k, v in arguments.items() if v is not None}
    blank = np.full((n_species,) + np.shape(obs_covs)[:3], np.nan, dtype=np.float32)
    spec = model_fn(**valid, obs=blank, **kwargs)
    if beta.shape[2] != spec.site_covs.shape[1] + 1 or alpha.shape[2] != spec.obs_covs.shape[3] + 1:
        raise ValueError("site_summary(): covariate counts differ from the fitted model's coefficients")
    N, T, J = spec.obs_covs.shape[:3]
    layout = layout_for(spec, N=N, T=T, J=J, Ks=beta.shape[2] - 1, Ko=alpha.shape[2] - 1)

    first, second = names[0] in wanted, names[1] in wanted
    per_species = []
    with time_limit(timeout):
        for sp in range(n_species):
            ds, draws = species_dataset(spec, sp, device), draws_from_sites(layout, posterior, sp)
            per_species.append(ds.site_summary(draws, ranks=ranks, psi=first, prob_detection=second))
            ds.close()

    out = {"probs": q, "n_draws": int(n)}
    for k, (site, want) in enumerate(zip(names, (first, second))):
        if not want:
            continue
        mean, sd, order = (np.stack([res[3 * k + m] for res in per_species], axis=-1) for m in range(3))   # (..., S)
        quantiles = interpolate(order, ranks, lo, hi, g)
        if k == 0:   # the first site is constant over the periods: (N, S) -> (T, N, S)
            mean, sd = (np.broadcast_to(a[None], (T,) + a.shape).copy() for a in (mean, sd))
            quantiles = np.broadcast_to(quantiles[:, None], (q.size, T) + quantiles.shape[1:]).copy()
        out[site] = {"mean": mean, "sd": sd, "quantiles": quantiles}
    return out
