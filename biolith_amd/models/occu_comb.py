"""``occu_comb`` / ``simulate_comb`` -- host-side mirror of biolith/models/occu_comb.py for the HIP engine.

The combined occupancy model: point counts (PC, no false positives), autonomous recording units (ARU, both false-positive
rates) and classifier scores (a two-component Normal mixture keyed by z) share one enumerated occupancy state z per
(species, site, period) (occu_comb.py:150-349).  ``occu_comb`` keeps the reference's signature (occu_comb.py:19-45), runs its
assertions (occu_comb.py:111-160) and resolves to an ``OccuSpec``; the z-marginalised density, its gradient and the sampler run
in the random-effects kernels' framework (re_kernel.hpp, kind 8).  ``simulate_comb`` is the reference's generator
(occu_comb.py:352-600), bit-identical for equal arguments (tests/golden).
"""
from __future__ import annotations

from typing import Any

import numpy as np

from ..distributions import Beta, Gamma, HalfNormal, Normal, as_beta, as_gamma, as_normal
from ..regression import LinearRegression
from .occu import OccuSpec

MAX_COMB_COVS = 16  # covariates per block (the random-effects kernels' BL_RE_MAXK)


def occu_comb(
    site_covs,
    PC_obs_covs,
    ARU_obs_covs,
    scores_obs,
    coords=None,
    ell: float = 1.0,
    PC_obs=None,
    ARU_obs=None,
    n_species: int = 1,
    prior_beta: Any = Normal(),
    prior_alpha: Any = Normal(),
    regressor_occ=LinearRegression,
    regressor_PC_det=LinearRegression,
    regressor_ARU_det=LinearRegression,
    prior_ARU_prob_fp_constant: Any = Beta(2, 5),
    prior_ARU_prob_fp_unoccupied: Any = Beta(2, 5),
    prior_mu: Any = Normal(0, 10),
    prior_sigma: Any = Gamma(5, 1),
    prior_gp_sd: Any = HalfNormal(1.0),
    prior_gp_length: Any = HalfNormal(1.0),
    site_random_effects: bool = False,
    PC_obs_random_effects: bool = False,
    ARU_obs_random_effects: bool = False,
    prior_site_re_sd: Any = HalfNormal(1.0),
    prior_obs_re_sd: Any = HalfNormal(1.0),
) -> OccuSpec:
    """Combined point-count, ARU and score occupancy model on the HIP engine (parameters: occu_comb.py:19-45).

    Built: linear regressors, Normal / Laplace coefficient priors, Beta priors of the two ARU false-positive rates (both always
    sampled), ``prior_mu`` Normal and ``prior_sigma`` Gamma (one, or a pair for the z = 0 / z = 1 components; mu1 is truncated below
    at mu0), any number of species (nothing is shared across the species plate, so each species is its own chain).  Anything else
    raises ``NotImplementedError``.

    Examples
    --------
    >>> from biolith_amd.models import occu_comb, simulate_comb
    >>> from biolith_amd.utils import fit
    >>> data, _ = simulate_comb()
    >>> results = fit(occu_comb, **data)
    >>> print(results.samples['psi'].mean())
    """
    site_covs = np.asarray(site_covs, dtype=np.float32)
    PC_obs_covs = np.asarray(PC_obs_covs, dtype=np.float32)
    ARU_obs_covs = np.asarray(ARU_obs_covs, dtype=np.float32)
    scores_obs = np.asarray(scores_obs, dtype=np.float32)
    PC_obs = None if PC_obs is None else np.asarray(PC_obs, dtype=np.float32)
    ARU_obs = None if ARU_obs is None else np.asarray(ARU_obs, dtype=np.float32)
    # occu_comb.py:111-160
    assert PC_obs is None or PC_obs.ndim == 4, "PC_obs must be None or of shape (n_species, n_sites, n_periods, PC_replicates)"
    assert ARU_obs is None or ARU_obs.ndim == 4, "ARU_obs must be None or of shape (n_species, n_sites, n_periods, ARU_replicates)"
    assert scores_obs.ndim == 4, "scores_obs must be of shape (n_species, n_sites, n_periods, scores_replicates)"
    assert site_covs.ndim == 2, "site_covs must be of shape (n_sites, n_site_covs)"
    assert PC_obs_covs.ndim == 4, "PC_obs_covs must be of shape (n_sites, n_periods, PC_replicates, n_PC_obs_covs)"
    assert ARU_obs_covs.ndim == 4, "ARU_obs_covs must be of shape (n_sites, n_periods, ARU_replicates, n_ARU_obs_covs)"
    n_sites, n_periods = site_covs.shape[0], PC_obs_covs.shape[1]
    PC_replicates, ARU_replicates = PC_obs_covs.shape[2], ARU_obs_covs.shape[2]
    n_species = scores_obs.shape[0]
    assert n_sites == site_covs.shape[0] == PC_obs_covs.shape[0] == ARU_obs_covs.shape[0], \
        "site_covs, PC_obs_covs, and ARU_obs_covs must have the same number of sites"
    assert PC_obs_covs.shape[1] == ARU_obs_covs.shape[1], "PC_obs_covs and ARU_obs_covs must have the same number of periods"
    assert scores_obs.shape[1] == n_sites, "scores_obs must have n_sites in dimension 1"
    assert scores_obs.shape[2] == n_periods, "scores_obs must have n_periods in dimension 2"
    if PC_obs is not None:
        assert PC_obs.shape == (n_species, n_sites, n_periods, PC_replicates)
    if ARU_obs is not None:
        assert ARU_obs.shape == (n_species, n_sites, n_periods, ARU_replicates)

    unsupported = []
    if coords is not None:
        unsupported.append("coords (spatial HSGP effect, occu_comb.py:187-196)")
    if site_random_effects or PC_obs_random_effects or ARU_obs_random_effects:
        unsupported.append("random effects (site_random_effects / PC_obs_random_effects / ARU_obs_random_effects)")
    if any(r is not LinearRegression for r in (regressor_occ, regressor_PC_det, regressor_ARU_det)):
        unsupported.append("non-linear regressors (occu_comb.py:226-228)")
    if PC_obs is None or ARU_obs is None:
        unsupported.append("PC_obs=None / ARU_obs=None (prior predictive)")
    if max(site_covs.shape[1], PC_obs_covs.shape[3], ARU_obs_covs.shape[3]) > MAX_COMB_COVS:
        unsupported.append(f"more than {MAX_COMB_COVS} covariates per block")
    if unsupported:
        raise NotImplementedError("biolith_amd.occu_comb: not built: " + "; ".join(unsupported))
    mus = prior_mu if isinstance(prior_mu, tuple) else (prior_mu, prior_mu)
    sigmas = prior_sigma if isinstance(prior_sigma, tuple) else (prior_sigma, prior_sigma)
    prior_mus = tuple(as_normal(p, "prior_mu") for p in mus)
    if any(p.family != "normal" for p in prior_mus):
        raise NotImplementedError("prior_mu: Normal(loc, scale) only")
    spec = OccuSpec(site_covs, PC_obs_covs, PC_obs, n_species, as_normal(prior_beta, "prior_beta"), as_normal(prior_alpha, "prior_alpha"),
                    model="occu_comb")
    spec.extras.update(ARU_obs_covs=ARU_obs_covs, ARU_obs=ARU_obs, scores_obs=scores_obs,
                       prior_fc=as_beta(prior_ARU_prob_fp_constant, "prior_ARU_prob_fp_constant"),
                       prior_fu=as_beta(prior_ARU_prob_fp_unoccupied, "prior_ARU_prob_fp_unoccupied"),
                       prior_mu=tuple(tuple(p) for p in prior_mus), prior_sigma=tuple(as_gamma(p, "prior_sigma") for p in sigmas))
    return spec


occu_comb.__biolith_amd_model__ = "occu_comb"


def simulate_comb(
    n_site_covs: int = 1,
    n_PC_covs: int = 1,
    n_ARU_covs: int = 1,
    n_sites: int = 100,
    n_species: int = 1,
    n_periods: int = 1,
    PC_replicates: int = 3,
    ARU_replicates: int = 24,
    scores_replicates: int = 24,
    ARU_prob_fp_constant: float = 0.0,
    ARU_prob_fp_unoccupied: float = 0.0,
    min_occupancy: float = 0.25,
    max_occupancy: float = 0.75,
    min_PC_observation_rate: float = 0.1,
    max_PC_observation_rate: float = 0.9,
    simulate_missing: bool = False,
    random_seed: int = 0,
    spatial: bool = False,
    gp_sd: float = 1.0,
    gp_l: float = 0.2,
    site_random_effects: bool = False,
    PC_obs_random_effects: bool = False,
    ARU_obs_random_effects: bool = False,
    site_re_sd: float = 0.5,
    obs_re_sd: float = 0.3,
):
    """Synthetic dataset for :func:`occu_comb`; returns ``(data, true_params)`` (occu_comb.py:352-600), bit-identical to the
    reference for equal arguments: one PCG64 stream, the same draw order inside the rejection loop and the same missingness
    masks after it.  ``spatial=True`` is outside the built path.

    Examples
    --------
    >>> from biolith_amd.models import simulate_comb
    >>> data, params = simulate_comb()
    >>> list(data.keys())
    ['site_covs', 'PC_obs_covs', 'ARU_obs_covs', 'PC_obs', 'ARU_obs', 'scores_obs', 'coords', 'ell']
    """
    if spatial:
        raise NotImplementedError("simulate_comb(spatial=True): the spatial HSGP effect is not built")
    rng = np.random.default_rng(random_seed)
    S, N, T = n_species, n_sites, n_periods
    mu0, sigma0, mu1, sigma1 = -3.0, 5.0, 2.0, 3.0   # occu_comb.py:527-528

    def detections(alpha, covs, re_det, obs_re):
        # alpha (S, K + 1), covs (N, T, J, K) -> p (S, N, T, J)
        lin = alpha[:, 0][:, None, None, None] + np.tensordot(alpha[:, 1:], covs, axes=([1], [3])) + re_det[:, :, None, None] + obs_re
        return 1 / (1 + np.exp(-lin))

    def effect(flag, sd, shape):
        return rng.normal(0, sd, size=shape) if flag else np.zeros(shape)

    def pc_rate(y):
        return np.mean(y[np.isfinite(y)])

    z = PC_obs = None
    while z is None or not (min_occupancy <= z.mean() <= max_occupancy
                            and min_PC_observation_rate <= pc_rate(PC_obs) <= max_PC_observation_rate):
        # occupancy (occu_comb.py:410-446)
        beta = rng.normal(size=(S, n_site_covs + 1))
        site_covs = rng.normal(size=(N, n_site_covs))
        w, ell = np.zeros(N), 0.0
        site_re_occ = effect(site_random_effects, site_re_sd, (S, N))
        site_re_det = effect(site_random_effects, site_re_sd, (S, N))
        psi = 1 / (1 + np.exp(-(beta[:, 0][:, None] + np.tensordot(beta[:, 1:], site_covs, axes=([1], [1])) + w[None, :] + site_re_occ)))
        z = rng.binomial(n=1, p=psi[:, None, :], size=(S, T, N))
        zs = z.transpose(0, 2, 1)[..., None]   # (S, N, T, 1)
        # point counts: no false positives (occu_comb.py:452-482)
        alpha_PC = rng.normal(size=(S, n_PC_covs + 1))
        PC_obs_covs = rng.normal(size=(N, T, PC_replicates, n_PC_covs))
        PC_obs_re = effect(PC_obs_random_effects, obs_re_sd, (S, N, T, PC_replicates))
        p_pc = detections(alpha_PC, PC_obs_covs, site_re_det, PC_obs_re)
        PC_obs = rng.binomial(1, zs * p_pc, size=(S, N, T, PC_replicates)).astype(float)
        # ARU: both false-positive rates (occu_comb.py:488-521)
        alpha_ARU = rng.normal(size=(S, n_ARU_covs + 1))
        ARU_obs_covs = rng.normal(size=(N, T, ARU_replicates, n_ARU_covs))
        ARU_obs_re = effect(ARU_obs_random_effects, obs_re_sd, (S, N, T, ARU_replicates))
        p_aru = detections(alpha_ARU, ARU_obs_covs, site_re_det, ARU_obs_re)
        p_aru_fp = 1 - ((1 - zs * p_aru) * (1 - ARU_prob_fp_constant) * (1 - (1 - zs) * ARU_prob_fp_unoccupied))
        ARU_obs = rng.binomial(1, p_aru_fp, size=(S, N, T, ARU_replicates)).astype(float)
        # scores (occu_comb.py:527-535)
        scores_obs = rng.normal(loc=(1 - zs) * mu0 + zs * mu1, scale=(1 - zs) * sigma0 + zs * sigma1,
                                size=(S, N, T, scores_replicates))

    print(f"True occupancy: {z.mean():.4f}")
    print(f"Proportion of PC timesteps with detection: {pc_rate(PC_obs):.4f}")

    if simulate_missing:   # occu_comb.py:542-556: the masks in this order
        for a, p in ((PC_obs, [0.2, 0.8]), (ARU_obs, [0.2, 0.8]), (scores_obs, [0.2, 0.8]), (PC_obs_covs, [0.05, 0.95]),
                     (ARU_obs_covs, [0.05, 0.95]), (site_covs, [0.05, 0.95])):
            a[rng.choice([True, False], size=a.shape, p=p)] = np.nan

    true_params = dict(z=z, beta=beta, alpha_PC=alpha_PC, alpha_ARU=alpha_ARU, mu0=mu0, sigma0=sigma0, mu1=mu1, sigma1=sigma1,
                       w=w, gp_sd=gp_sd, gp_l=gp_l)
    if site_random_effects:
        true_params.update(site_re_occ=site_re_occ, site_re_det=site_re_det, site_re_sd=site_re_sd)
    if PC_obs_random_effects:
        true_params.update(PC_obs_re=PC_obs_re, obs_re_sd=obs_re_sd)
    if ARU_obs_random_effects:
        true_params.update(ARU_obs_re=ARU_obs_re, obs_re_sd=obs_re_sd)
    return dict(site_covs=site_covs, PC_obs_covs=PC_obs_covs, ARU_obs_covs=ARU_obs_covs, PC_obs=PC_obs, ARU_obs=ARU_obs,
                scores_obs=scores_obs, coords=None, ell=ell), true_params
