"""Deviance, residuals and the posterior predictive check -- the remaining consumers of ``predict()``'s output
(biolith/evaluation/deviance.py:10-117, residuals.py:6-90, posterior_predictive_check.py:17-160) -- and the check's builder-defined
counterpart for the abundance and count models, ``posterior_predictive_check_counts``.

Host code: array reductions over the predictive sites (``psi``, ``z``, ``prob_detection``, ``y``), nothing here is on
the sampling path.  Layouts are the reference's: predictive sites are (draws, [J,] T, N, S), ``obs`` is (S, N, T, J).
"""
from __future__ import annotations

from typing import Callable, Dict, Tuple

import numpy as np
from scipy.special import logsumexp

from .predictive_density import _valid_obs, log_likelihood, log_likelihood_manual


def _deviance_of(ll_valid) -> float:
    """-2 log of the posterior-mean likelihood of the whole data set; ``ll_valid`` is (draws, n_valid)."""
    per_draw = ll_valid.sum(axis=1)
    return float(-2.0 * (logsumexp(per_draw) - np.log(per_draw.shape[0])))


def deviance(model_fn: Callable, posterior_samples: Dict[str, np.ndarray], **kwargs) -> float:
    """Deviance as a scoring rule, ``-2 log( mean_q prod_ij p(y_ij | z_i^q, p_ij^q) )`` over the valid
    observations (deviance.py:10-71; spOccupancy, Hooten & Hobbs 2015)."""
    valid = _valid_obs(kwargs["site_covs"], kwargs["obs_covs"], kwargs["obs"])
    ll = log_likelihood(model_fn, posterior_samples, **kwargs)["y"].transpose((0, 4, 3, 2, 1))
    return _deviance_of(ll[:, valid].astype(np.float64))


def deviance_manual(posterior_samples: Dict[str, np.ndarray], data: Dict[str, np.ndarray]) -> float:
    """Deviance from the marginal ``psi * p`` likelihood of the no-false-positive Bernoulli model (deviance.py:74-117)."""
    valid = _valid_obs(data["site_covs"], data["obs_covs"], data["obs"])
    return _deviance_of(log_likelihood_manual(posterior_samples, data)[:, valid])


def residuals(posterior_samples: Dict[str, np.ndarray], obs) -> Tuple[np.ndarray, np.ndarray]:
    """Occupancy and detection residuals of Wright et al. (2019) per predictive draw (residuals.py:6-90):
    ``o = z - psi`` of shape (draws, T, N, S), and ``d = y - p`` where the draw has the site occupied, NaN elsewhere,
    of shape (draws, S, N, T, J)."""
    z = np.asarray(posterior_samples["z"], dtype=np.float64)
    psi = np.asarray(posterior_samples["psi"], dtype=np.float64)
    p = np.asarray(posterior_samples["prob_detection"], dtype=np.float64)      # (draws, J, T, N, S)
    occupancy = z - psi
    y = np.asarray(obs, dtype=np.float64).transpose((3, 2, 1, 0))[None]        # (1, J, T, N, S)
    detection = np.where(z[:, None] == 1, y - p, np.nan)
    return occupancy, detection.transpose((0, 4, 3, 2, 1))


def _freeman_tukey(observed, expected):
    return (np.sqrt(observed) - np.sqrt(expected)) ** 2


def _chi_squared(observed, expected, eps: float = 1e-10):
    return (observed - expected) ** 2 / (expected + eps)


def posterior_predictive_check(posterior_samples: Dict[str, np.ndarray], obs, group_by: str = "site",
                               statistic: str = "freeman-tukey") -> float:
    """Bayesian p-value ``P(T(y_rep, theta) > T(y, theta) | y)`` with detections grouped by site or by revisit
    and the Freeman-Tukey or chi-squared discrepancy against ``E = psi * p`` (posterior_predictive_check.py:17-160;
    valid without false positives, as the reference notes)."""
    stats = {"freeman-tukey": _freeman_tukey, "chi-squared": _chi_squared}
    if statistic not in stats:
        raise ValueError(f"`statistic` must be one of {list(stats)}")
    if group_by not in ("site", "revisit"):
        raise ValueError("`group_by` must be either 'site' or 'revisit'")
    stat = stats[statistic]
    obs = np.asarray(obs, dtype=np.float64)                                     # (S, N, T, J)
    y_rep = np.asarray(posterior_samples["y"], dtype=np.float64)
    p = np.asarray(posterior_samples["prob_detection"], dtype=np.float64)
    psi = np.asarray(posterior_samples["psi"], dtype=np.float64)
    if y_rep.ndim == 5:
        y_rep = y_rep.transpose((0, 4, 3, 2, 1))                                # -> (draws, S, N, T, J)
    if p.ndim == 5:
        p = p.transpose((0, 4, 3, 2, 1))
    if psi.ndim == 3:
        psi = psi[:, None, ...]
    elif psi.ndim == 2:
        psi = psi[:, None, :, None]
    expected = psi.transpose((0, 3, 2, 1))[..., None] * p                       # (draws, S, N, T, J)
    seen = np.isfinite(obs)[None]
    axes_obs, axes_rep = ((2, 3), (3, 4)) if group_by == "site" else ((1,), (2,))
    obs_g = np.nansum(obs, axis=axes_obs)
    rep_g = np.where(seen, y_rep, 0.0).sum(axis=axes_rep)
    exp_g = np.where(seen, expected, 0.0).sum(axis=axes_rep)
    reduce_axes = tuple(range(1, exp_g.ndim))
    d_obs = stat(obs_g[None], exp_g).sum(axis=reduce_axes)
    d_rep = stat(rep_g, exp_g).sum(axis=reduce_axes)
    return float(np.mean(d_rep > d_obs))


def _restricted_poisson_sums(lam, K: int, q=None):
    """Sums over Poisson(``lam``) restricted to 0..K, float64, with ``w_n = lam^n / n!`` by the recursion ``w_n = w_{n-1} lam / n``:
    ``sum n w_n / sum w_n`` (its mean), or with ``q`` the ratio ``sum w_n q^n / sum w_n`` (its probability generating function at
    ``q``; ``lam`` broadcasts against ``q``).  ``exp(-lam)`` cancels and is never formed.  ``lam^n / n!`` overflows float64
    (lam = 3e4, K = 100), so wherever the running term passes 1e100 every accumulator is scaled by 1e-200: finite for any float32
    ``lam`` (an infinite one reads as the largest float32) and any K."""
    lam = np.minimum(np.asarray(lam, dtype=np.float64), float(np.finfo(np.float32).max))
    shape = lam.shape if q is None else np.broadcast_shapes(lam.shape, np.shape(q))
    w, a = np.ones(shape), np.ones(shape)
    b = np.zeros(shape) if q is None else np.ones(shape)
    v = None if q is None else np.ones(shape)
    for n in range(1, int(K) + 1):
        r = lam / n
        w = w * r
        a = a + w
        if q is None:
            b = b + n * w
        else:
            v = v * (r * q)
            b = b + v
        down = np.where(w > 1e100, 1e-200, 1.0)
        w, a, b = w * down, a * down, b * down
        if v is not None:
            v = v * down
    return b / a


def _expected_counts(name: str, ps: Dict[str, np.ndarray], session_duration, max_abundance: int, obs_shape) -> np.ndarray:
    """E[y | draw] with the latent state summed out, (draws, J, T, N, S) float64, from predict()'s deterministic sites."""
    col = (-1,) + (1,) * 4
    if name == "occu_cop":
        psi = np.asarray(ps["psi"], dtype=np.float64)[:, None]                      # (n, 1, T, N, S)
        rate = np.asarray(ps["rate_detection"], dtype=np.float64)                   # (n, J, T, N, S)
        dur = np.ones(obs_shape) if session_duration is None else np.asarray(session_duration, dtype=np.float64)
        if dur.ndim == 3:
            dur = dur[None]
        dur = np.broadcast_to(dur, obs_shape).transpose((3, 2, 1, 0))[None]         # (1, J, T, N, S)
        f_c = np.asarray(ps["rate_fp_constant"], np.float64).reshape(col) if "rate_fp_constant" in ps else 0.0
        f_u = np.asarray(ps["rate_fp_unoccupied"], np.float64).reshape(col) if "rate_fp_unoccupied" in ps else 0.0
        return dur * (psi * rate + (1.0 - psi) * f_u + f_c)
    lam = np.asarray(ps["abundance"], dtype=np.float64)                             # (n, T, N, S)
    p = np.asarray(ps["prob_detection"], dtype=np.float64)                          # (n, J, T, N, S)
    if name == "nmixture":
        return _restricted_poisson_sums(lam, max_abundance)[:, None] * p
    f = np.asarray(ps["prob_fp_constant"], np.float64).reshape(col) if "prob_fp_constant" in ps else 0.0
    return 1.0 - (1.0 - f) * _restricted_poisson_sums(lam[:, None], max_abundance, q=1.0 - p)


def _count_discrepancies(model_fn, posterior_samples, obs, group_by, statistic, session_duration, max_abundance, rates):
    """``d_obs``, ``d_rep`` (draws,) float64 of posterior_predictive_check_counts, summed over the species plate."""
    stats = {"freeman-tukey": _freeman_tukey, "chi-squared": _chi_squared}
    name = getattr(model_fn, "__biolith_amd_model__", None) if callable(model_fn) else None
    if name not in ("occu_rn", "nmixture", "occu_cop"):
        raise NotImplementedError(f"posterior_predictive_check_counts: not built for {name} (built: occu_rn, nmixture, occu_cop; occu "
                                  "is served by posterior_predictive_check)")
    if statistic not in stats:
        raise ValueError(f"`statistic` must be one of {list(stats)}")
    if group_by not in ("site", "revisit"):
        raise ValueError("`group_by` must be either 'site' or 'revisit'")
    stat = stats[statistic]
    ps = {**posterior_samples, **rates}
    obs = np.asarray(obs, dtype=np.float64)                                         # (S, N, T, J)
    expected = _expected_counts(name, ps, session_duration, max_abundance, obs.shape).transpose((0, 4, 3, 2, 1))
    y_rep = np.asarray(ps["y"], dtype=np.float64).transpose((0, 4, 3, 2, 1))        # -> (draws, S, N, T, J)
    seen = ~np.isnan(obs)[None]
    axes_obs, axes_rep = ((2, 3), (3, 4)) if group_by == "site" else ((1,), (2,))
    obs_g = np.nansum(obs, axis=axes_obs)
    rep_g = np.where(seen, y_rep, 0.0).sum(axis=axes_rep)
    exp_g = np.where(seen, expected, 0.0).sum(axis=axes_rep)
    reduce_axes = tuple(range(1, exp_g.ndim))
    return stat(obs_g[None], exp_g).sum(axis=reduce_axes), stat(rep_g, exp_g).sum(axis=reduce_axes)


def posterior_predictive_check_counts(model_fn: Callable, posterior_samples: Dict[str, np.ndarray], obs, group_by: str = "site",
                                      statistic: str = "freeman-tukey", session_duration=None, max_abundance: int = 100,
                                      **rates) -> float:
    """Bayesian p-value ``P(T(y_rep, theta) > T(y, theta) | y)`` for ``occu_rn``, ``nmixture`` and ``occu_cop`` (BUILDER-DEFINED: the
    reference's check is ``occu``'s), with the data grouped by site or by revisit and the Freeman-Tukey or chi-squared discrepancy
    against the model's mean of ``y`` with the latent state summed out -- the principle behind ``occu``'s ``psi * p``.

    ``posterior_samples`` is what :func:`biolith_amd.utils.predict` returned; ``obs`` is (S, N, T, J), NaN = not observed.  With
    ``lambda`` = ``abundance``, ``p`` = ``prob_detection``, K = ``max_abundance`` and ``pi`` the pmf of Poisson(lambda) restricted
    to 0..K::

        nmixture   E = p * sum_n n pi_n
        occu_rn    E = 1 - (1 - prob_fp_constant) * sum_n pi_n (1 - p)^n
        occu_cop   E = session_duration * (psi * rate_detection + (1 - psi) * rate_fp_unoccupied + rate_fp_constant)

    ``predict()`` returns predictive sites only, so a sampled false-positive site (``prob_fp_constant``, ``rate_fp_constant``,
    ``rate_fp_unoccupied``, (draws,)) is merged in by the caller -- into ``posterior_samples`` or as a keyword -- as
    ``log_likelihood(occu_cop, ...)`` asks; absent, it is 0.  ``session_duration`` (occu_cop) is (N, T, J) or (S, N, T, J), 1 if
    ``None``.  A visit counts where its observation is present; o, ``y`` and E are summed over a group's seen visits before the
    statistic.  The fused path is :func:`biolith_amd.utils.predictive_check_counts`.

    Examples
    --------
    >>> from biolith_amd.models import simulate_nmixture, nmixture
    >>> from biolith_amd.utils import fit, predict
    >>> from biolith_amd.evaluation import posterior_predictive_check_counts
    >>> data, _ = simulate_nmixture()
    >>> results = fit(nmixture, **data)
    >>> preds = predict(nmixture, results.mcmc, **data)
    >>> posterior_predictive_check_counts(nmixture, preds, data["obs"], "site", "chi-squared")
    """
    d_obs, d_rep = _count_discrepancies(model_fn, posterior_samples, obs, group_by, statistic, session_duration, max_abundance, rates)
    return float(np.mean(d_rep > d_obs))
