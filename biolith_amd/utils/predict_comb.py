"""``predict_comb`` -- the posterior predictive of ``occu_comb`` on the HIP engine.  BUILDER-DEFINED, under a name of its own.

The reference's ``predict`` cannot serve this model the way it serves the others: ``scores_obs`` is a required positional argument of
``occu_comb`` (models/occu_comb.py:19-24, 340-349), so it cannot be withheld, and under numpyro's ``Predictive`` the ``scores`` site
stays pinned to the data while ``y_pc`` / ``y_aru`` are drawn.  [UPSTREAM behaviour of numpyro's ``Predictive``; not executable here.]
``predict(occu_comb, ...)`` therefore keeps refusing, and ``predict_comb`` draws ALL three observed sites -- a replicate data set per
posterior draw, which is what ``posterior_predictive_check``, ``residuals`` and ``log_likelihood_comb`` / ``waic_comb`` need.  The sites
come from two C-ABI calls per species, ``bl_deterministic_comb`` and ``bl_predict_comb`` (``include/biolith_hip.h``).  No NumPyro/JAX,
no CPU fallback.
"""
from __future__ import annotations

from typing import Callable, Optional

import numpy as np

from .data import species_dataset
from .layout import draws_from_sites, layout_for
from .mcmc import LazySamples
from .misc import time_limit

_RATES = ("ARU_prob_fp_constant", "ARU_fp_unoccupied", "mu0", "mu1", "sigma0", "sigma1")


def predict_comb(
    model_fn: Callable,
    mcmc,
    site_covs,
    PC_obs_covs,
    ARU_obs_covs,
    scores_obs=None,
    scores_replicates: Optional[int] = None,
    random_seed: int = 0,
    timeout: Optional[int] = None,
    **kwargs,
) -> dict:
    """Posterior predictive samples of a fitted ``occu_comb``: one replicate of the point counts, the ARU detections and the scores per
    posterior draw, at the fitted sites or at new ones (any number of sites, periods and replicates; the covariate counts are the fit's).

    ``mcmc`` is the ``FitResult.mcmc`` that :func:`biolith_amd.utils.fit` returned.  ``**simulate_comb()[0]`` is accepted as it is:
    ``PC_obs``, ``ARU_obs``, ``coords=None`` and ``ell`` are accepted and ignored, and ``scores_obs`` supplies only the species count and
    the number of scores per period -- all three observed sites are withheld.  Without ``scores_obs``, ``scores_replicates`` says how many
    scores to draw per (site, period) and the species count is the posterior's.  NaN covariates read as 0 and no replicate is masked, as
    the reference's models read them with the observations withheld.  Other keyword arguments go to ``model_fn``.

    Returns
    -------
    LazySamples
        Species plate last.  ``psi`` (n, T, N, S); ``z`` (n, T, N, S) int32; ``PC_prob_detection`` (n, Jpc, T, N, S);
        ``ARU_prob_detection`` and ``ARU_prob_detection_fp`` (n, Jaru, T, N, S), the latter at the sampled ``z``:
        ``1 - (1 - z p)(1 - fc)(1 - (1 - z) fu)``; ``y_pc`` (n, Jpc, T, N, S) and ``y_aru`` (n, Jaru, T, N, S) int32; ``scores``
        (n, Js, T, N, S) float32; and the posterior's own ``ARU_prob_fp_constant``, ``ARU_fp_unoccupied``, ``mu0``, ``mu1``, ``sigma0``,
        ``sigma1`` (n, S), so that ``log_likelihood_comb`` / ``waic_comb`` need no merging.  The replicate-level arrays are materialised
        on first access.  The sample is a function of (``random_seed``, species, draw, period, site).

    Examples
    --------
    >>> from biolith_amd.models import occu_comb, simulate_comb
    >>> from biolith_amd.utils import fit, predict_comb
    >>> from biolith_amd.evaluation import posterior_predictive_check, waic_comb
    >>> data, _ = simulate_comb()
    >>> results = fit(occu_comb, **data, num_samples=100, num_warmup=100, num_chains=1)
    >>> preds = predict_comb(occu_comb, results.mcmc, **data)
    >>> waic_comb(preds, **data)
    >>> # the point counts are the block without false positives, the one the check and the residuals are valid for
    >>> pc = {"psi": preds["psi"], "prob_detection": preds["PC_prob_detection"], "y": preds["y_pc"], "z": preds["z"]}
    >>> posterior_predictive_check(pc, data["PC_obs"])
    """
    name = getattr(model_fn, "__biolith_amd_model__", None) if callable(model_fn) else None
    if name is None:
        raise TypeError("predict_comb(): model_fn must be a biolith_amd model (biolith_amd.models.occu_comb)")
    if name != "occu_comb":
        raise NotImplementedError(f"predict_comb(): not built for {name} (built: occu_comb); use predict")
    for ignored in ("PC_obs", "ARU_obs", "coords", "ell"):   # (withheld / not part of the built model)
        kwargs.pop(ignored, None)
    device = int(kwargs.pop("device", 0))

    posterior = mcmc.get_samples()
    beta = np.asarray(posterior["beta"], dtype=np.float32)            # (n, S, Ks + 1)
    alpha_pc = np.asarray(posterior["alpha_PC"], dtype=np.float32)    # (n, S, Kpc + 1)
    alpha_aru = np.asarray(posterior["alpha_ARU"], dtype=np.float32)  # (n, S, Karu + 1)
    n, n_species = beta.shape[:2]
    X = np.asarray(site_covs, dtype=np.float32)
    Wp = np.asarray(PC_obs_covs, dtype=np.float32)
    Wa = np.asarray(ARU_obs_covs, dtype=np.float32)
    if scores_obs is not None:
        sc = np.shape(scores_obs)
        if len(sc) != 4:
            raise ValueError("predict_comb(): scores_obs must be of shape (n_species, n_sites, n_periods, scores_replicates)")
        if scores_replicates is not None and int(scores_replicates) != sc[3]:
            raise ValueError("predict_comb(): scores_replicates differs from scores_obs")
        if sc[0] != n_species:
            raise ValueError(f"predict_comb(): scores_obs has {sc[0]} species, the posterior {n_species}")
        Js = int(sc[3])
    elif scores_replicates is not None:
        Js = int(scores_replicates)
        if Js < 0:
            raise ValueError("predict_comb(): scores_replicates must not be negative")
    else:
        raise ValueError("predict_comb(): give scores_obs or scores_replicates (how many scores to draw per site and period)")
    if X.ndim != 2 or Wp.ndim != 4 or Wa.ndim != 4:
        raise ValueError("predict_comb(): site_covs (N, Ks), PC_obs_covs (N, T, Jpc, Kpc) and ARU_obs_covs (N, T, Jaru, Karu) are required")
    if beta.shape[2] != X.shape[1] + 1 or alpha_pc.shape[2] != Wp.shape[3] + 1 or alpha_aru.shape[2] != Wa.shape[3] + 1:
        raise ValueError("predict_comb(): covariate counts differ from the fitted model's coefficients")

    # the model is called with all three observed sites blank: the validators want their shapes, nothing reads their values
    N, T, Jpc = Wp.shape[:3]
    Jaru = Wa.shape[2]
    blank = lambda J: np.full((n_species, N, T, J), np.nan, dtype=np.float32)
    spec = model_fn(X, Wp, Wa, blank(Js), PC_obs=blank(Jpc), ARU_obs=blank(Jaru), **kwargs)
    layout = layout_for(spec, N=N, T=T, J=Jpc, Ks=X.shape[1], Ko=Wp.shape[3], Ka=Wa.shape[3])

    handles, psi, z8, ypc8, yaru8, scores = [], [], [], [], [], []
    with time_limit(timeout):
        for sp in range(n_species):
            ds, draws = species_dataset(spec, sp, device), draws_from_sites(layout, posterior, sp)
            psi.append(ds.deterministic_comb(draws, psi=True, pc_prob=False, aru_prob=False)[0])
            # (the species' streams are separated as the conditional posteriors separate them)
            z, yp, ya, s = ds.predictive_comb(draws, seed=(int(random_seed) + (sp << 32)) & (2 ** 64 - 1))
            z8.append(z), ypc8.append(yp), yaru8.append(ya), scores.append(s)
            handles.append((ds, draws))

    def pc_prob():
        return np.stack([d.deterministic_comb(dr, psi=False, pc_prob=True, aru_prob=False)[1] for d, dr in handles], axis=-1)

    def aru_prob():
        return np.stack([d.deterministic_comb(dr, psi=False, pc_prob=False, aru_prob=True)[2] for d, dr in handles], axis=-1)

    rates = {k: np.asarray(posterior[k], dtype=np.float32).reshape(n, n_species) for k in _RATES}

    def aru_prob_fp():
        # occu_comb.py:325-331 at the sampled z:  1 - (1 - z p)(1 - fc)(1 - (1 - z) fu) = z p + (1 - z p) q,  q = fc + g - fc g,
        # g = (1 - z) fu -- the form that is z p exactly where both rates are 0
        zf = np.stack(z8, axis=-1)[:, None].astype(np.float32)
        zp = out["ARU_prob_detection"] * zf
        fc = rates["ARU_prob_fp_constant"][:, None, None, None, :]
        g = (np.float32(1.0) - zf) * rates["ARU_fp_unoccupied"][:, None, None, None, :]
        return zp + (np.float32(1.0) - zp) * (fc + g - fc * g)

    out = LazySamples()
    out["psi"] = np.stack(psi, axis=-1)                                               # (n, T, N, S)
    out["z"] = np.stack(z8, axis=-1).astype(np.int32)
    out.set_lazy("PC_prob_detection", pc_prob)                                        # (n, Jpc, T, N, S)
    out.set_lazy("ARU_prob_detection", aru_prob)                                      # (n, Jaru, T, N, S)
    out.set_lazy("ARU_prob_detection_fp", aru_prob_fp)
    out.set_lazy("y_pc", lambda: np.stack(ypc8, axis=-1).astype(np.int32))
    out.set_lazy("y_aru", lambda: np.stack(yaru8, axis=-1).astype(np.int32))
    out.set_lazy("scores", lambda: np.stack(scores, axis=-1))                         # (n, Js, T, N, S)
    for k, v in rates.items():   # (Predictive leaves the posterior's own sites out; the evaluation wants them next to z)
        out[k] = v
    return out
