"""``site_diagnostics`` -- effective sample size and split R-hat of a fitted model's deterministic sites, fused on the HIP engine.

"Did psi converge, and where not" is the first question after a fit.  On the host it is ``predict()`` followed by
``evaluation.effective_sample_size`` / ``split_gelman_rubin`` (the reference: ``numpyro.diagnostics.summary`` over ``psi`` and
``prob_detection``): an (n, J, T, N) float32 array written to the host, widened to float64 and put through FFTs.  A deterministic site's
value at (draw, cell) is a handful of FMAs, so here one C-ABI call per species -- ``bl_site_diagnostics`` (``include/biolith_hip.h``) --
recomputes it wherever a sum wants it and stores nothing per draw: the chains' means and variances, then the autocovariances by direct
lagged sums in float64, a block of lags a pass, for as long as Geyer's sequence of any cell of a wave is still positive.  Nothing of size
(n, T, N) or (n, J, T, N) exists on the device or on the host.  BUILDER-DEFINED: the reference has no counterpart.
``evaluation.summary`` is the host function for *sampled* sites shaped (chains, draws, ...).  No NumPyro/JAX, no CPU fallback.
"""
from __future__ import annotations

from typing import Callable, Optional, Sequence

import numpy as np

from .data import prepare_data, species_dataset
from .layout import draws_from_sites, layout_for
from .misc import time_limit
from .site_summary import site_names

_HOST_PATH = "predict() followed by evaluation.effective_sample_size / split_gelman_rubin over (chains, draws, ...) is the host path"
_KEYS = ("n_eff", "r_hat", "mean", "sd")


def site_diagnostics(
    model_fn: Callable,
    mcmc,
    site_covs=None,
    obs_covs=None,
    obs=None,
    session_duration=None,
    sites: Optional[Sequence[str]] = None,
    num_chains: Optional[int] = None,
    timeout: Optional[int] = None,
    **kwargs,
) -> dict:
    """Effective sample size, split R-hat, mean, standard deviation and Monte Carlo standard error of a fitted model's deterministic
    sites, per cell, over the posterior draws of all chains.

    The data and the model's options are passed exactly as to :func:`biolith_amd.utils.predict` -- possibly new sites' covariates;
    ``obs`` is accepted and ignored, ``device=`` goes through ``kwargs``; ``mcmc`` is the ``FitResult.mcmc`` of the fit.  ``sites``
    names a subset of the model's two deterministic sites under ``predict()``'s names (default: both): ``psi`` and
    ``prob_detection``; for ``occu_rn`` and ``nmixture`` the first is ``abundance``, for ``occu_cop`` the second is
    ``rate_detection``.  The chain structure is ``mcmc.num_chains`` unless ``num_chains=`` says otherwise: ``mcmc.get_samples()`` is
    flat and chain-major, chain ``c`` owns draws ``c n .. c n + n - 1``.  Only the sampled sites of the posterior are read: a fit's
    lazy deterministic sites (``psi``, ``prob_detection``, ...) are not materialised.

    The contract::

        preds = predict(m, mcmc, **data);  v = preds[name].reshape((C, n) + preds[name].shape[1:])
        d = site_diagnostics(m, mcmc, **data)[name]
        d["n_eff"]  ~ evaluation.effective_sample_size(v)
        d["r_hat"]  ~ evaluation.split_gelman_rubin(v)
        d["mean"], d["sd"]  == site_summary(m, mcmc, **data)[name]["mean"], ["sd"]
        d["mcse_mean"]      == d["sd"] / sqrt(d["n_eff"])

    The values diagnosed are ``predict()``'s float32 values bit for bit, widened to float64.  ``n_eff`` is numpyro's estimator (Geyer's
    initial monotone sequence on the chain-averaged biased autocovariances, as ``evaluation/diagnostics.py`` states it) with the
    autocovariances summed directly instead of through an FFT; ``r_hat`` is the split R-hat over the 2 C half chains.  A cell whose
    values are all equal has NaN for both, as the host's 0 / 0; ``r_hat`` is NaN below 4 draws per chain; for very short chains
    ``n_eff`` may be negative (``mcse_mean`` is then NaN): that is the definition.

    Returns
    -------
    dict
        ``{name: {"n_eff", "r_hat", "mean", "sd", "mcse_mean"}, "n_chains": C, "n_draws": n}`` -- ``n_draws`` per chain.  The arrays
        are float64 in ``predict()``'s shapes without the draw axis, the species plate last: the first site (T, N, S) -- constant over
        T --, the second (J, T, N, S).  The same call returns the same bytes.

    Raises
    ------
    NotImplementedError
        ``occu_comb`` and ``occu_dyn`` (their sites are formed on the host).
    ValueError
        A draw count that the chain count does not divide; fewer than 2 draws per chain; non-finite posterior sites; unknown ``sites``;
        covariate counts that differ from the fitted coefficients.

    Examples
    --------
    >>> from biolith_amd.models import simulate, occu
    >>> from biolith_amd.utils import fit, site_diagnostics
    >>> data, _ = simulate()
    >>> results = fit(occu, **data, num_samples=100, num_warmup=100, num_chains=2)
    >>> site_diagnostics(occu, results.mcmc, **data)["psi"]["n_eff"].shape
    """
    name = getattr(model_fn, "__biolith_amd_model__", None) if callable(model_fn) else None
    if name is None:
        raise TypeError("site_diagnostics(): model_fn must be a biolith_amd model (biolith_amd.models.occu / occu_rn / ...)")
    if name in ("occu_comb", "occu_dyn"):
        raise NotImplementedError(f"site_diagnostics(): not built for {name} (its sites are formed on the host); {_HOST_PATH}")
    names = site_names(name)
    wanted = names if sites is None else tuple([sites] if isinstance(sites, str) else sites)
    if not wanted or any(s not in names for s in wanted):
        raise ValueError(f"site_diagnostics(): `sites` must name some of {names} for {name}, got {tuple(wanted)}")
    if num_chains is not None and int(num_chains) < 1:
        raise ValueError(f"site_diagnostics(): num_chains={num_chains}, at least 1")
    device = int(kwargs.pop("device", 0))

    site_covs, obs_covs, obs, session_duration, _, _ = prepare_data(site_covs, obs_covs, obs, session_duration)
    if num_chains is None and getattr(mcmc, "num_chains", None) is None:
        raise ValueError("site_diagnostics(): `mcmc` has no num_chains; pass num_chains=")
    n_chains = int(mcmc.num_chains if num_chains is None else num_chains)
    posterior = mcmc.get_samples()
    # A fit's deterministic sites are lazy (LazySamples: the device forms psi, prob_detection, ... on first access, and the fit keeps
    # them): they are functions of the sampled sites, which are what is read here -- reading them would build the very (n, J, T, N)
    # arrays this call exists to avoid.  So they are neither touched nor checked.
    lazy = getattr(posterior, "_lazy", ())
    for k in posterior:
        if k not in lazy and not np.isfinite(np.asarray(posterior[k])).all():
            raise ValueError(f"site_diagnostics(): the posterior site {k!r} holds non-finite draws")
    beta = np.asarray(posterior["beta"], dtype=np.float32)    # (C n, S, Ks+1)
    alpha = np.asarray(posterior["alpha"], dtype=np.float32)  # (C n, S, Ko+1)
    total, n_species = beta.shape[0], beta.shape[1]
    if n_chains < 1 or total == 0 or total % n_chains:
        raise ValueError(f"site_diagnostics(): the posterior's {total} draws are not {n_chains} chains of equal length")
    n = total // n_chains
    if n < 2:
        raise ValueError(f"site_diagnostics(): {n} draws per chain, at least 2")

    # the handles are predict()'s: the model is called with the observations withheld (an all-missing array of the fitted species count)
    arguments = dict(site_covs=site_covs, obs_covs=obs_covs, session_duration=session_duration)
    valid = {k: v for k, v in arguments.items() if v is not None}
    blank = np.full((n_species,) + np.shape(obs_covs)[:3], np.nan, dtype=np.float32)
    spec = model_fn(**valid, obs=blank, **kwargs)
    if beta.shape[2] != spec.site_covs.shape[1] + 1 or alpha.shape[2] != spec.obs_covs.shape[3] + 1:
        raise ValueError("site_diagnostics(): covariate counts differ from the fitted model's coefficients")
    N, T, J = spec.obs_covs.shape[:3]
    layout = layout_for(spec, N=N, T=T, J=J, Ks=beta.shape[2] - 1, Ko=alpha.shape[2] - 1)

    first, second = names[0] in wanted, names[1] in wanted
    per_species = []
    with time_limit(timeout):
        for sp in range(n_species):
            ds, draws = species_dataset(spec, sp, device), draws_from_sites(layout, posterior, sp)
            per_species.append(ds.site_diagnostics(draws, n_chains, psi=first, prob_detection=second))
            ds.close()

    out = {"n_chains": n_chains, "n_draws": int(n)}
    for k, (site, want) in enumerate(zip(names, (first, second))):
        if not want:
            continue
        table = {key: np.stack([res[4 * k + m] for res in per_species], axis=-1) for m, key in enumerate(_KEYS)}   # (..., S)
        if k == 0:   # the first site is constant over the periods: (N, S) -> (T, N, S)
            table = {key: np.broadcast_to(a[None], (T,) + a.shape).copy() for key, a in table.items()}
        with np.errstate(invalid="ignore", divide="ignore"):
            table["mcse_mean"] = table["sd"] / np.sqrt(table["n_eff"])
        out[site] = table
    return out
