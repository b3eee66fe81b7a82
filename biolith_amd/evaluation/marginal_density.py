"""lppd / WAIC from the z-marginalised site-period log-likelihood (host NumPy only).

BUILDER-DEFINED, no counterpart in the reference: its ``lppd`` / ``waic`` (lppd.py, waic.py) take the log-likelihood of each
replicate given a ``z`` drawn from the PRIOR, so the criterion carries the Monte Carlo noise of a latent the model's likelihood
sums out analytically.  Here the unit is the (site, period) -- the level at which the marginal likelihood factorises -- and the
pointwise term is ``latent["log_lik"]`` of :func:`biolith_amd.utils.conditional_occupancy`: log(psi p(obs | 1) + (1 - psi) p(obs | 0)).
Cells without an unmasked observation (``n_obs == 0``) carry no likelihood and are left out.

The result of :func:`biolith_amd.utils.conditional_dynamics` (``occu_dyn``) is accepted too: there the seasons of a site are dependent, the
marginal likelihood factorises over SITES only, and ``log_lik`` / ``n_obs`` are per site.  ``finite_sample_turnover`` reads its joint
path draws.

The result of :func:`biolith_amd.utils.conditional_abundance` (``occu_rn`` / ``nmixture``) is accepted too: its ``log_lik`` is the same
kind of term with the abundance N summed out, its ``n_obs`` the same count, so an ``occu`` and an ``occu_rn`` fit of the same detections
compare on the same cells.

The result of :func:`biolith_amd.utils.conditional_scores` (``occu_cs``) is accepted too: same keys, same shapes, the cell's unmasked
scores with z and every f summed out.  ``expected_true_positives`` reads its ``f_prob``.

So is the result of :func:`biolith_amd.utils.conditional_counts` (``occu_cop``): ``lppd_marginal``, ``waic_marginal`` and
``finite_sample_occupancy`` read its ``log_lik``, ``n_obs`` and ``z`` -- the cell's unmasked counts with z summed out, the Poisson
pmf's parameter-free part included, so a count model is compared with an occu or occu_rn fit on the same cells only where the data
are the same.  ``expected_true_detections`` reads its ``true_mean``.
"""
from __future__ import annotations

from typing import Dict

import numpy as np

from .predictive_density import _pointwise


def _cells(latent) -> np.ndarray:
    """(draws, cells with n_obs > 0) float64 of a ``conditional_occupancy`` / ``conditional_abundance`` result."""
    ll = np.asarray(latent["log_lik"], dtype=np.float64)
    n_obs = np.asarray(latent["n_obs"])
    if ll.shape[1:] != n_obs.shape:
        raise ValueError(f"log_lik {ll.shape} and n_obs {n_obs.shape} do not belong together")
    return ll[:, n_obs > 0]


def lppd_marginal(latent) -> float:
    """``sum_cells log mean_draws exp(log_lik)`` over the (period, site, species) cells with data; ``latent`` is the result of
    ``conditional_occupancy`` or of ``conditional_abundance``."""
    return _pointwise(_cells(latent))[0]


def waic_marginal(latent) -> Dict[str, float]:
    """``{"waic": -2 (lppd - p_waic), "p_waic", "lppd"}`` with the site-period as the unit (p_waic: the summed posterior variance);
    ``latent`` is the result of ``conditional_occupancy`` or of ``conditional_abundance``."""
    l, p = _pointwise(_cells(latent))
    return {"waic": -2 * (l - p), "p_waic": p, "lppd": l}


def finite_sample_occupancy(latent) -> np.ndarray:
    """(draws, T, S): the share of occupied sites in each conditional draw of ``z`` -- the finite-sample occupancy of Royle & Kery."""
    return np.asarray(latent["z"], dtype=np.float64).mean(axis=2)


def finite_sample_abundance(latent) -> np.ndarray:
    """(draws, T, S): the total of ``N_i`` over the sites in each conditional draw of a ``conditional_abundance`` result -- the
    finite-sample population size of the surveyed sites."""
    return np.asarray(latent["N_i"], dtype=np.float64).sum(axis=2)


def expected_true_positives(latent) -> np.ndarray:
    """(draws, T, N, S): the sum of ``f_prob`` over the visits of a ``conditional_scores`` result -- the posterior expected number of
    true-positive recordings in each (period, site), per posterior draw."""
    return np.asarray(latent["f_prob"], dtype=np.float64).sum(axis=1)


def expected_true_detections(latent) -> np.ndarray:
    """(draws, T, N, S): the sum of ``true_mean`` over the visits of a ``conditional_counts`` result -- the posterior expected number of
    a (period, site)'s counted detections that were real rather than false positives, per posterior draw."""
    return np.asarray(latent["true_mean"], dtype=np.float64).sum(axis=1)


def finite_sample_turnover(latent) -> Dict[str, np.ndarray]:
    """``{"colonisation": (draws, T - 1, S), "extinction": (draws, T - 1, S)}`` of a ``conditional_dynamics`` result: per conditional
    path draw the share of the sites unoccupied at t that are occupied at t + 1, and the share of the sites occupied at t that are
    unoccupied at t + 1 -- the realised colonisation and extinction rates of the surveyed sites.  NaN where no site is in the
    denominator."""
    z = np.asarray(latent["z"]) != 0                                      # (n, T, N, S)
    now, nxt = z[:, :-1], z[:, 1:]
    with np.errstate(invalid="ignore", divide="ignore"):
        col = (~now & nxt).sum(axis=2) / (~now).sum(axis=2).astype(np.float64)
        ext = (now & ~nxt).sum(axis=2) / now.sum(axis=2).astype(np.float64)
    return {"colonisation": col, "extinction": ext}
